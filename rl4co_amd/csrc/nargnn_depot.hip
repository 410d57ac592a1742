// nargnn_depot.hip — DeepACO's heatmap encoder for the depot graphs of CVRP, OP and PCTSP (the reference's NARGNNEncoder in
// inference with VRP / OP / PCTSPInitEmbedding and CVRPEdgeEmbedding, env_embeddings/edge.py:119-176) as one launch for
// gfx950, fp32 throughout. The scheme is nargnn.hip's: one workgroup of eight waves per INSTANCE, persistent over the
// layers, grid-stride over the instances, the 64-long dot products on nargnn_tile.h's MFMA tiles.
//
// The graph is not regular. Node 0 is the depot, nodes 1 .. C = N - 1 the customers. Edge rows, R = C (K + 2) of them:
//   customer u owns the K + 1 contiguous rows (u - 1)(K + 1) ..: its K customer neighbours neighbors[u - 1][0 .. K-1], then
//   its depot edge (u -> 0); the depot owns the last C rows, row D0 + i - 1 being (0 -> i), D0 = C (K + 1).
// gnn.py:55 pools by SOURCE: a customer's mean is over its K + 1 rows, the depot's over its C rows.
//   x = silu(init(locs, feats)) (row 0 from the depot linear); w = silu(edge_embed(cost))
//   per layer   -- workgroup barrier 1 --
//               A  x1 .. x4 = v_lin1 .. v_lin4 (x) for all N nodes      (MFMA; wave = one matrix, every other node tile)
//               -- workgroup barrier 2 --
//               B1 node sums over the layer's incoming w, split evenly: wave q takes the customers [c0, c1) of C / 8 each
//                    (x[u] += silu(bn_v(x1[u] + sum / (K + 1))), lane = channel) and the depot rows of the same [c0, c1),
//                    whose gated partial sum it leaves in `part[q]`
//               -- workgroup barrier 3 --
//               B2 wave 0 adds the eight partials in wave order: x[0] += silu(bn_v(x1[0] + sum / C)); every wave updates
//                    its OWN rows [e0, e1) of R / 8 each, w[e] += silu(bn_e((e_lin(w[e]) + x3[u]) + x4[v])), in 16-row
//                    MFMA tiles that start at e0 (clamped on load, masked on store at e1): in place, a row is read by its
//                    own tile only
// THREE workgroup barriers per layer. The depot hazard is settled by ordering: every node sum of a layer (the customers'
// and the depot's partials) is taken before barrier 3, every edge update of that layer runs behind it, so both updates
// read the layer's incoming w; x1 .. x4 were taken from the incoming x in A, and x[0] is next read behind barrier 1.
// Load balance: the waves split ROWS, not nodes, in every phase that walks the edge state (B1 reads (K + 2) C / 8 rows
// per wave, B2 and the MLP R / 8); node boundaries and tile boundaries are unrelated, (u, v) come from the row number.
// The depot's mean over up to 1023 terms is eight partial sums of at most 128 terms, added once.
//   heatmap MLP on the own rows, layer by layer in place (wave-local: no workgroup barrier), the 64 -> 1 output as a wave
//   reduction per row. The workgroup fills the instance's heatmap with fill_value, meets at one workgroup barrier (which
//   drains the stores), then each wave scatters log(sigmoid(out) + small_value) of its own rows to heatmap[u][v]: row 0
//   receives C stores, column 0 one from every customer's depot row, and no entry is written by two rows as long as a
//   neighbour list holds no 0 and no repeat.
//
// Where the state lives (rows of kRS = 68 floats):
//   tier 0  N <= rl4co_nargnn_depot_lds_nodes(K): x2, x4 and the edge state in LDS; x, x1, x3, part in `scratch`
//   tier 1  N <= 300: x2, x4 in LDS; the edge state and x, x1, x3, part in `scratch`
//   tier 2  up to 1024 nodes: everything in `scratch`
// `scratch` is sized by the grid, not by B; a workgroup's slice is its own, so workgroup barriers order it.
// LDS budget (bytes, all dynamic; the launcher checks that the compiler added no static LDS beyond kStaticLds):
//   head 64 (the bad-index flag) + 272 (2 N + C (K + 2)) in tier 0 | 272 * 2 N in tier 1 | nothing more in tier 2.
//   tier 0 at K = 10: N <= 43; at K = 20: N <= 25.
// scratch rows per workgroup: 3 N + 8 (part) + C (K + 2) in tiers 1 and 2 + 2 N in tier 2.
// A neighbour index outside [1, N) raises RL4CO_EBIT_TOUR_INDEX and the instance is left untouched: the lists are checked
// before anything is read through them. 0 is refused as well: it would repeat the depot edge, and two rows would write one
// heatmap entry.
#include <hip/hip_runtime.h>

#include "common.h"
#include "nargnn_tile.h"

namespace {

using namespace rl4co::nargnn;  // kD, kRS, f32x4, sigmoidf, siluf, load_wfrags, gemm_tile, node_gemm

constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;
constexpr int kCuLds = 160 * 1024;
constexpr int kStaticLds = 64;
constexpr int kHeadBytes = 64;
constexpr int kNodeLdsMax = 300;  // tier 1: 64 + 2 * 300 * 272 + 64 <= 160 KiB

__host__ __device__ constexpr int64_t edge_rows(int N, int K) { return (int64_t)(N - 1) * (K + 2); }
__host__ __device__ constexpr int64_t lds_bytes(int tier, int N, int K) {
  const int64_t rows = tier == 0 ? 2 * (int64_t)N + edge_rows(N, K) : (tier == 1 ? 2 * (int64_t)N : 0);
  return kHeadBytes + rows * kRS * 4;
}
__host__ __device__ constexpr int64_t scratch_floats(int tier, int N, int K) {
  const int64_t rows = 3 * (int64_t)N + kWaves + (tier >= 1 ? edge_rows(N, K) : 0) + (tier == 2 ? 2 * (int64_t)N : 0);
  return rows * kRS;
}
inline int tier_of(int N, int K) {
  if (lds_bytes(0, N, K) + kStaticLds <= kCuLds) return 0;
  return N <= kNodeLdsMax ? 1 : 2;
}

template <int TIER>
__global__ void __launch_bounds__(kThreads) nargnn_depot_kernel(const rl4co_nargnn_depot_args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint32_t* bad_flag = reinterpret_cast<uint32_t*>(smem);
  float* lds = reinterpret_cast<float*>(smem + kHeadBytes);

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 15, g = lane >> 4;
  const int N = a.N, K = a.K, F = a.F, C = N - 1, K1 = K + 1, CK = C * K;
  const int D0 = C * K1, R = D0 + C;  // the depot's first row, all rows

  float* gs = a.scratch + (int64_t)blockIdx.x * scratch_floats(TIER, N, K);
  float* X = gs;
  float* X1 = gs + N * kRS;
  float* X3 = gs + 2 * N * kRS;
  float* PART = gs + 3 * N * kRS;
  float* after = PART + kWaves * kRS;
  float *X2, *X4, *E;
  if constexpr (TIER == 0) {
    X2 = lds;
    X4 = lds + N * kRS;
    E = lds + 2 * N * kRS;
  } else if constexpr (TIER == 1) {
    X2 = lds;
    X4 = lds + N * kRS;
    E = after;
  } else {
    E = after;
    X2 = E + (int64_t)R * kRS;
    X4 = X2 + N * kRS;
  }

  // the wave's customers (and depot rows) in B1 and its edge rows everywhere else, for every layer
  const int cpw = (C + kWaves - 1) / kWaves;
  const int c0 = min(C, w * cpw), c1 = min(C, c0 + cpw);
  const int rpw = (R + kWaves - 1) / kWaves;
  const int e0 = min(R, w * rpw), e1 = min(R, e0 + rpw);

  for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
    const int32_t* nbr = a.neighbors + (int64_t)b * CK;

    // ---- the neighbour lists: range check before anything is read through them ------------------------------------------
    if (tid == 0) *bad_flag = 0u;
    __syncthreads();
    bool bad = false;
    for (int e = tid; e < CK; e += kThreads) {
      const int v = nbr[e];
      bad |= v < 1 || v >= N;
    }
    if (bad) *bad_flag = 1u;
    __syncthreads();
    const bool refused = *bad_flag != 0u;  // (uniform: one LDS word)
    __syncthreads();                       // the word is reset at the top of the next instance
    if (refused) {
      if (tid == 0) atomicOr(a.err, RL4CO_EBIT_TOUR_INDEX);
      continue;
    }

    // ---- x = silu(init(locs, feats)), w = silu(edge_embed(cost)): lane = channel ---------------------------------------------
    {
      const float* loc = a.locs + (int64_t)b * N * 2;
      const float* feat = a.feats + (int64_t)b * C * F;
      float* emb = a.node_embed + (int64_t)b * N * kD;
      const int IW = 2 + F;
      const float wx = a.init_w[IW * lane], wy = a.init_w[IW * lane + 1], wf0 = a.init_w[IW * lane + 2];
      const float wf1 = F == 2 ? a.init_w[IW * lane + 3] : 0.0f, bi = a.init_b[lane];
      for (int ci = c0; ci < c1; ++ci) {
        const int u = ci + 1;
        float h = fmaf(wy, loc[2 * u + 1], wx * loc[2 * u]);
        h = fmaf(wf0, feat[ci * F], h);
        if (F == 2) h = fmaf(wf1, feat[ci * F + 1], h);
        h += bi;
        emb[u * kD + lane] = h;
        X[u * kRS + lane] = siluf(h);
      }
      if (w == 0) {
        const float h = fmaf(a.depot_w[2 * lane + 1], loc[1], a.depot_w[2 * lane] * loc[0]) + a.depot_b[lane];
        emb[lane] = h;
        X[lane] = siluf(h);
      }
      const float we = a.edge_w[lane], be = a.edge_b[lane];
      const float* cost = a.edge_cost + (int64_t)b * CK;
      const float* dcost = a.depot_cost + (int64_t)b * C;
      for (int e = e0; e < e1; ++e) {
        float d;
        if (e < D0) {
          const int ci = e / K1, k = e - ci * K1;
          d = k < K ? cost[ci * K + k] : dcost[ci];
        } else {
          d = dcost[e - D0];
        }
        E[e * kRS + lane] = siluf(d * we + be);
      }
    }

    for (int l = 0; l < a.L; ++l) {
      const float* LW = a.lin_w + (int64_t)l * 5 * kD * kD;
      const float* LB = a.lin_b + (int64_t)l * 5 * kD;
      const float* BN = a.bn + (int64_t)l * 4 * kD;
      __syncthreads();  // 1: x of every node is this layer's; the layer before has finished with x1 .. x4 and part

      // ---- A. x1 .. x4 of every node ---------------------------------------------------------------------------------
      {
        const int m = w & 3, tile0 = w >> 2;  // (wave-uniform)
        const float* Wm = LW + m * kD * kD;
        const float* bm = LB + m * kD;
        if (m == 0) node_gemm(X1, X, Wm, bm, N, tile0, lane);
        else if (m == 1) node_gemm(X2, X, Wm, bm, N, tile0, lane);
        else if (m == 2) node_gemm(X3, X, Wm, bm, N, tile0, lane);
        else node_gemm(X4, X, Wm, bm, N, tile0, lane);
      }
      __syncthreads();  // 2

      // ---- B1. the node sums: the wave's customers, then its share of the depot's rows (lane = channel) --------------------
      const float vsc = BN[lane], vsh = BN[kD + lane];
      {
        const float x2d = X2[lane];  // the depot's x2: every customer's last row gathers it
        for (int ci = c0; ci < c1; ++ci) {
          const int u = ci + 1, r0 = ci * K1;
          float s = 0.0f;
          for (int k = 0; k < K; ++k) {
            const int v = nbr[ci * K + k];
            s += sigmoidf(E[(r0 + k) * kRS + lane]) * X2[v * kRS + lane];
          }
          s += sigmoidf(E[(r0 + K) * kRS + lane]) * x2d;
          const float y = (X1[u * kRS + lane] + s / (float)K1) * vsc + vsh;
          X[u * kRS + lane] += siluf(y);
        }
        float s = 0.0f;
        for (int ci = c0; ci < c1; ++ci) s += sigmoidf(E[(D0 + ci) * kRS + lane]) * X2[(ci + 1) * kRS + lane];
        PART[w * kRS + lane] = s;
      }
      __syncthreads();  // 3: every node sum has read the incoming w; the partials are visible

      // ---- B2. the depot's node update (wave 0), then the edge update of the own rows, in place -------------------------------
      if (w == 0) {
        float s = 0.0f;
#pragma unroll
        for (int q = 0; q < kWaves; ++q) s += PART[q * kRS + lane];
        const float y = (X1[lane] + s / (float)C) * vsc + vsh;
        X[lane] += siluf(y);
      }
      {
        f32x4 wf[4][4];
        load_wfrags(wf, LW + 4 * kD * kD, lane);
        float bcol[4], sc[4], sh[4];
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
          bcol[ct] = LB[4 * kD + 16 * ct + c];
          sc[ct] = BN[2 * kD + 16 * ct + c];
          sh[ct] = BN[3 * kD + 16 * ct + c];
        }
        for (int t0 = e0; t0 < e1; t0 += 16) {
          const int row = min(t0 + c, e1 - 1);  // rows past the wave's last repeat it and are not stored
          f32x4 acc[4];
          gemm_tile(acc, wf, E + row * kRS + 4 * g);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int e = t0 + 4 * g + r;
            if (e < e1) {
              int u, v;
              if (e < D0) {
                const int ci = e / K1, k = e - ci * K1;
                u = ci + 1;
                v = k < K ? nbr[ci * K + k] : 0;
              } else {
                u = 0;
                v = e - D0 + 1;
              }
#pragma unroll
              for (int ct = 0; ct < 4; ++ct) {
                const int col = 16 * ct + c;
                float y = ((acc[ct][r] + bcol[ct]) + X3[u * kRS + col]) + X4[v * kRS + col];
                y = y * sc[ct] + sh[ct];
                E[e * kRS + col] += siluf(y);
              }
            }
          }
        }
      }
    }

    // ---- the heatmap MLP on the own rows: layer by layer in place, wave-local ----------------------------------------------
    for (int h = 0; h + 1 < a.H; ++h) {
      rl4co::lds_barrier_wave();  // rows written in one lane layout are read in another, by this wave only
      f32x4 wf[4][4];
      load_wfrags(wf, a.mlp_w + (int64_t)h * kD * kD, lane);
      float bcol[4];
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) bcol[ct] = a.mlp_b ? a.mlp_b[h * kD + 16 * ct + c] : 0.0f;
      for (int t0 = e0; t0 < e1; t0 += 16) {
        const int row = min(t0 + c, e1 - 1);
        f32x4 acc[4];
        gemm_tile(acc, wf, E + row * kRS + 4 * g);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int e = t0 + 4 * g + r;
          if (e < e1) {
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) E[e * kRS + 16 * ct + c] = siluf(acc[ct][r] + bcol[ct]);
          }
        }
      }
    }
    rl4co::lds_barrier_wave();

    // ---- the fill, then the output layer and the scatter of the own rows -------------------------------------------------------
    {
      float* hm = a.heatmap + (int64_t)b * N * N;
      for (int j = tid; j < N * N; j += kThreads) hm[j] = a.fill_value;
      // a heatmap row is filled by many waves and scattered into by others: the barrier waits for every fill store
      __syncthreads();
      const float wo = a.out_w[lane];
      const float bo = a.out_b ? a.out_b[0] : 0.0f;
      for (int e = e0; e < e1; ++e) {
        const float p = rl4co::bfly_sum<1, 64>(E[e * kRS + lane] * wo);
        if (lane == 0) {
          int u, v;
          if (e < D0) {
            const int ci = e / K1, k = e - ci * K1;
            u = ci + 1;
            v = k < K ? nbr[ci * K + k] : 0;
          } else {
            u = 0;
            v = e - D0 + 1;
          }
          hm[u * N + v] = logf(sigmoidf(p + bo) + a.small_value);
        }
      }
    }
  }
}

template <int TIER>
int launch(const rl4co_nargnn_depot_args& a, hipStream_t stream) {
  const int lds = (int)lds_bytes(TIER, a.N, a.K);
  hipFuncAttributes fa;
  RL4CO_HIP_TRY(hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(nargnn_depot_kernel<TIER>)));
  RL4CO_REQUIRE((int64_t)fa.sharedSizeBytes <= kStaticLds);  // the budget of rl4co_nargnn_depot_lds_nodes holds
  if (lds > 64 * 1024) {
    RL4CO_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(nargnn_depot_kernel<TIER>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  }
  hipLaunchKernelGGL((nargnn_depot_kernel<TIER>), dim3(a.n_workgroups), dim3(kThreads), lds, stream, a);
  RL4CO_HIP_TRY(hipGetLastError());
  return RL4CO_OK;
}

}  // namespace

extern "C" int rl4co_nargnn_depot_lds_nodes(int K) {
  if (K < 1) return 0;
  int n = 1024;
  while (n > 0 && lds_bytes(0, n, K) + kStaticLds > kCuLds) --n;
  return n;
}

extern "C" int64_t rl4co_nargnn_depot_scratch_bytes(int N, int K) {
  if (N < 3 || N > 1024 || K < 1 || K > 256 || K > N - 2) return 0;
  return scratch_floats(tier_of(N, K), N, K) * 4;
}

extern "C" int rl4co_nargnn_depot_heatmap(const rl4co_nargnn_depot_args* args, void* stream) {
  static_assert(lds_bytes(1, kNodeLdsMax, 1) + kStaticLds <= kCuLds, "the node planes of tier 1 fit the LDS");
  static_assert(edge_rows(1024, 256) * kRS < (int64_t)1 << 31, "row offsets fit an int");
  RL4CO_REQUIRE(args != nullptr);
  const rl4co_nargnn_depot_args& a = *args;
  RL4CO_REQUIRE(a.D == kD);
  RL4CO_REQUIRE(a.B >= 1);
  RL4CO_REQUIRE(a.N >= 3 && a.N <= 1024);
  RL4CO_REQUIRE(a.K >= 1 && a.K <= 256 && a.K <= a.N - 2);
  RL4CO_REQUIRE(a.F == 1 || a.F == 2);
  RL4CO_REQUIRE(a.L >= 0 && a.L <= (1 << 20));
  RL4CO_REQUIRE(a.H >= 1 && a.H <= (1 << 20));
  RL4CO_REQUIRE(a.n_workgroups >= 1 && a.n_workgroups <= a.B);
  RL4CO_REQUIRE(a.locs != nullptr && a.feats != nullptr && a.neighbors != nullptr && a.edge_cost != nullptr && a.depot_cost != nullptr);
  RL4CO_REQUIRE(a.init_w != nullptr && a.init_b != nullptr && a.depot_w != nullptr && a.depot_b != nullptr);
  RL4CO_REQUIRE(a.edge_w != nullptr && a.edge_b != nullptr);
  RL4CO_REQUIRE(a.L == 0 || (a.lin_w != nullptr && a.lin_b != nullptr && a.bn != nullptr));
  RL4CO_REQUIRE(a.H == 1 || a.mlp_w != nullptr);
  RL4CO_REQUIRE(a.out_w != nullptr);
  RL4CO_REQUIRE(((reinterpret_cast<uintptr_t>(a.lin_w) | reinterpret_cast<uintptr_t>(a.mlp_w)) & 15) == 0);  // 16-byte fragments
  RL4CO_REQUIRE(a.scratch != nullptr);
  RL4CO_REQUIRE((reinterpret_cast<uintptr_t>(a.scratch) & 15) == 0);
  RL4CO_REQUIRE(a.scratch_bytes >= (int64_t)a.n_workgroups * rl4co_nargnn_depot_scratch_bytes(a.N, a.K));
  RL4CO_REQUIRE(a.heatmap != nullptr && a.node_embed != nullptr && a.err != nullptr);
  hipStream_t s = rl4co::as_stream(stream);
  switch (tier_of(a.N, a.K)) {
    case 0: return launch<0>(a, s);
    case 1: return launch<1>(a, s);
    default: return launch<2>(a, s);
  }
}

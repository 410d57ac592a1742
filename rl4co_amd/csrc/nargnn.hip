// nargnn.hip — DeepACO's heatmap encoder for TSP (the reference's NARGNNEncoder in inference: models/zoo/nargnn/encoder.py,
// models/nn/graph/gnn.py, env_embeddings/edge.py) as one launch for gfx950, fp32 throughout.
//
// One workgroup of eight waves per INSTANCE, persistent over the layers, grid-stride over the instances. The TSP graph is
// regular (node u has exactly K out-edges, to neighbors[u][0 .. K-1]), so the edge state is a dense [N K][64] array whose
// rows u K .. u K + K - 1 belong to node u, and gnn.py's pooling by edge_index[0] is a sum over a node's own K rows.
//   x = silu(init(locs)); w = silu(edge_embed(cost))
//   per layer   A  x1 .. x4 = v_lin1 .. v_lin4 (x) for every node      (MFMA; wave = one matrix, every other node tile)
//               -- workgroup barrier --
//               B  for the wave's OWN nodes [n0, n1):
//                    x[u] += silu(bn_v(x1[u] + sum_k(sigmoid(w[u][k]) * x2[v_k]) / K))      (lane = channel)
//                    w[e] += silu(bn_e((e_lin(w[e]) + x3[u]) + x4[v])) for the own rows e in [n0 K, n1 K), in 16-row
//                    MFMA tiles that start at n0 K: in place, a row is read by its own tile only
//               -- workgroup barrier (top of the next layer) --
//   heatmap MLP on the own rows, layer by layer in place (wave-local: no workgroup barrier), the 64 -> 1 output as a wave
//   reduction per row, then heatmap[u][:] = fill_value and heatmap[u][v_k] = log(sigmoid(out) + small_value).
// Both updates of a layer read the layer's incoming x and w: the node update of a wave's nodes runs before the edge update
// of the same nodes' rows, and x1 .. x4 were taken from x in A.
//
// MFMA v_mfma_f32_16x16x4_f32: the operand layout, the tile product and the node GEMM are nargnn_tile.h's, shared with
// nargnn_depot.hip.
//
// Where the state lives (rows of kRS = 68 floats: the 16 lanes of one g read 16 distinct bank quads):
//   tier 0  N <= rl4co_nargnn_lds_nodes(K): x2, x4 and the edge state in LDS; x, x1, x3 in `scratch`
//   tier 1  N <= 300: x2, x4 in LDS; the edge state and x, x1, x3 in `scratch`
//   tier 2  up to 1024 nodes: everything in `scratch`
// `scratch` is sized by the grid, not by B; a workgroup's slice is read and written by that workgroup only, so workgroup
// barriers (and, inside a wave, a workgroup-scope fence) order it. x, x1 and x3 are read by the node that owns them or as
// MFMA rows once per layer; only x2 and x4 are gathered through the neighbour lists.
// LDS budget (bytes, all dynamic; the launcher checks that the compiler added no static LDS beyond kStaticLds):
//   head 64 (the bad-index flag) + 272 (2 N + N K) in tier 0 | 272 * 2 N in tier 1 | nothing more in tier 2.
//   tier 0 at K = 10: N <= 50 (163 264 bytes); at K = 20: N <= 27.
// A neighbour index outside [0, N) raises RL4CO_EBIT_TOUR_INDEX and the instance is left untouched: the lists are checked
// before anything is read through them.
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

__host__ __device__ constexpr int64_t lds_bytes(int tier, int N, int K) {
  const int64_t rows = tier == 0 ? 2 * (int64_t)N + (int64_t)N * K : (tier == 1 ? 2 * (int64_t)N : 0);
  return kHeadBytes + rows * kRS * 4;
}
__host__ __device__ constexpr int64_t scratch_floats(int tier, int N, int K) {
  const int64_t rows = 3 * (int64_t)N + (tier >= 1 ? (int64_t)N * K : 0) + (tier == 2 ? 2 * (int64_t)N : 0);
  return rows * kRS;
}
inline int tier_of(int N, int K) {
  if (lds_bytes(0, N, K) + kStaticLds <= kCuLds) return 0;
  return N <= kNodeLdsMax ? 1 : 2;
}

template <int TIER>
__global__ void __launch_bounds__(kThreads) nargnn_kernel(const rl4co_nargnn_args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint32_t* bad_flag = reinterpret_cast<uint32_t*>(smem);
  float* lds = reinterpret_cast<float*>(smem + kHeadBytes);

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c = lane & 15, g = lane >> 4;
  const int N = a.N, K = a.K, NK = N * K;
  const float count = (float)K;

  float* gs = a.scratch + (int64_t)blockIdx.x * scratch_floats(TIER, N, K);
  float* X = gs;
  float* X1 = gs + N * kRS;
  float* X3 = gs + 2 * N * kRS;
  float *X2, *X4, *E;
  if constexpr (TIER == 0) {
    X2 = lds;
    X4 = lds + N * kRS;
    E = lds + 2 * N * kRS;
  } else if constexpr (TIER == 1) {
    X2 = lds;
    X4 = lds + N * kRS;
    E = gs + 3 * N * kRS;
  } else {
    E = gs + 3 * N * kRS;
    X2 = E + (int64_t)NK * kRS;
    X4 = X2 + N * kRS;
  }

  // the wave's own nodes and edge rows, for every layer
  const int npw = (N + kWaves - 1) / kWaves;
  const int n0 = min(N, w * npw), n1 = min(N, n0 + npw);
  const int e0 = n0 * K, e1 = n1 * K;

  for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
    const int32_t* nbr = a.neighbors + (int64_t)b * NK;

    // ---- the neighbour lists: range check before anything is read through them ------------------------------------------
    if (tid == 0) *bad_flag = 0u;
    __syncthreads();
    bool bad = false;
    for (int e = tid; e < NK; e += kThreads) {
      const int v = nbr[e];
      bad |= v < 0 || v >= N;
    }
    if (bad) *bad_flag = 1u;
    __syncthreads();
    const bool refused = *bad_flag != 0u;  // (uniform: one LDS word)
    __syncthreads();                       // the word is reset at the top of the next instance
    if (refused) {
      if (tid == 0) atomicOr(a.err, RL4CO_EBIT_TOUR_INDEX);
      continue;
    }

    // ---- x = silu(init(locs)), w = silu(edge_embed(cost)): lane = channel, the wave's own rows ---------------------------
    {
      const float* loc = a.locs + (int64_t)b * N * 2;
      const float wx = a.init_w[2 * lane], wy = a.init_w[2 * lane + 1], bi = a.init_b[lane];
      float* emb = a.node_embed + (int64_t)b * N * kD;
      for (int u = n0; u < n1; ++u) {
        const float h = fmaf(wy, loc[2 * u + 1], wx * loc[2 * u]) + bi;
        emb[u * kD + lane] = h;
        X[u * kRS + lane] = siluf(h);
      }
      const float we = a.edge_w[lane], be = a.edge_b[lane];
      const float* cost = a.edge_cost + (int64_t)b * NK;
      for (int e = e0; e < e1; ++e) E[e * kRS + lane] = siluf(cost[e] * we + be);
    }

    for (int l = 0; l < a.L; ++l) {
      const float* LW = a.lin_w + (int64_t)l * 5 * kD * kD;
      const float* LB = a.lin_b + (int64_t)l * 5 * kD;
      const float* BN = a.bn + (int64_t)l * 4 * kD;
      __syncthreads();  // x of every node is this layer's; the layer before has finished with x1 .. x4

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
      __syncthreads();

      // ---- B1. the node update of the own nodes (lane = channel) -------------------------------------------------------
      {
        const float sc = BN[lane], sh = BN[kD + lane];
        for (int u = n0; u < n1; ++u) {
          float s = 0.0f;
          for (int k = 0; k < K; ++k) {
            const int e = u * K + k;
            const int v = nbr[e];
            s += sigmoidf(E[e * kRS + lane]) * X2[v * kRS + lane];
          }
          const float y = (X1[u * kRS + lane] + s / count) * sc + sh;
          X[u * kRS + lane] += siluf(y);
        }
      }

      // ---- B2. the edge update of the own rows, in place ------------------------------------------------------------------
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
              const int u = e / K, v = nbr[e];
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

    // ---- the output layer and the heatmap rows of the own nodes -------------------------------------------------------------
    {
      float* hm = a.heatmap + (int64_t)b * N * N;
      for (int u = n0; u < n1; ++u)
        for (int j = lane; j < N; j += 64) hm[u * N + j] = a.fill_value;
      // the fill has reached memory before a neighbour entry of the same row is stored over it
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      const float wo = a.out_w[lane];
      const float bo = a.out_b ? a.out_b[0] : 0.0f;
      for (int e = e0; e < e1; ++e) {
        const float p = rl4co::bfly_sum<1, 64>(E[e * kRS + lane] * wo);
        if (lane == 0) hm[(e / K) * N + nbr[e]] = logf(sigmoidf(p + bo) + a.small_value);
      }
    }
  }
}

template <int TIER>
int launch(const rl4co_nargnn_args& a, hipStream_t stream) {
  const int lds = (int)lds_bytes(TIER, a.N, a.K);
  hipFuncAttributes fa;
  RL4CO_HIP_TRY(hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(nargnn_kernel<TIER>)));
  RL4CO_REQUIRE((int64_t)fa.sharedSizeBytes <= kStaticLds);  // the budget of rl4co_nargnn_lds_nodes holds
  if (lds > 64 * 1024) {
    RL4CO_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(nargnn_kernel<TIER>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  }
  hipLaunchKernelGGL((nargnn_kernel<TIER>), dim3(a.n_workgroups), dim3(kThreads), lds, stream, a);
  RL4CO_HIP_TRY(hipGetLastError());
  return RL4CO_OK;
}

}  // namespace

extern "C" int rl4co_nargnn_lds_nodes(int K) {
  if (K < 1) return 0;
  int n = 1024;
  while (n > 0 && lds_bytes(0, n, K) + kStaticLds > kCuLds) --n;
  return n;
}

extern "C" int64_t rl4co_nargnn_scratch_bytes(int N, int K) {
  if (N < 2 || N > 1024 || K < 1 || K > 256) return 0;
  return scratch_floats(tier_of(N, K), N, K) * 4;
}

extern "C" int rl4co_nargnn_heatmap(const rl4co_nargnn_args* args, void* stream) {
  static_assert(lds_bytes(1, kNodeLdsMax, 1) + kStaticLds <= kCuLds, "the node planes of tier 1 fit the LDS");
  RL4CO_REQUIRE(args != nullptr);
  const rl4co_nargnn_args& a = *args;
  RL4CO_REQUIRE(a.D == kD);
  RL4CO_REQUIRE(a.B >= 1);
  RL4CO_REQUIRE(a.N >= 2 && a.N <= 1024);
  RL4CO_REQUIRE(a.K >= 1 && a.K <= 256 && a.K <= a.N - 1);
  RL4CO_REQUIRE(a.L >= 0 && a.L <= (1 << 20));
  RL4CO_REQUIRE(a.H >= 1 && a.H <= (1 << 20));
  RL4CO_REQUIRE(a.n_workgroups >= 1 && a.n_workgroups <= a.B);
  RL4CO_REQUIRE(a.reserved0 == 0);
  RL4CO_REQUIRE(a.locs != nullptr && a.neighbors != nullptr && a.edge_cost != nullptr);
  RL4CO_REQUIRE(a.init_w != nullptr && a.init_b != nullptr && a.edge_w != nullptr && a.edge_b != nullptr);
  RL4CO_REQUIRE(a.L == 0 || (a.lin_w != nullptr && a.lin_b != nullptr && a.bn != nullptr));
  RL4CO_REQUIRE(a.H == 1 || a.mlp_w != nullptr);
  RL4CO_REQUIRE(a.out_w != nullptr);
  RL4CO_REQUIRE(((reinterpret_cast<uintptr_t>(a.lin_w) | reinterpret_cast<uintptr_t>(a.mlp_w)) & 15) == 0);  // 16-byte fragments
  RL4CO_REQUIRE(a.scratch != nullptr);
  RL4CO_REQUIRE((reinterpret_cast<uintptr_t>(a.scratch) & 15) == 0);
  RL4CO_REQUIRE(a.scratch_bytes >= (int64_t)a.n_workgroups * rl4co_nargnn_scratch_bytes(a.N, a.K));
  RL4CO_REQUIRE(a.heatmap != nullptr && a.node_embed != nullptr && a.err != nullptr);
  hipStream_t s = rl4co::as_stream(stream);
  switch (tier_of(a.N, a.K)) {
    case 0: return launch<0>(a, s);
    case 1: return launch<1>(a, s);
    default: return launch<2>(a, s);
  }
}

// nargnn_depot.hip — DeepACO's heatmap encoder for the depot graphs of CVRP, OP and PCTSP (the reference's NARGNNEncoder in
// inference with VRP / OP / PCTSPInitEmbedding and CVRPEdgeEmbedding, env_embeddings/edge.py:119-176) as one launch for
// gfx950, fp32 throughout. The scheme, the MFMA tiles, the tiers and their LDS budget are nargnn_shared.h's, shared with
// nargnn.hip; what follows is the depot graph's own.
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
// The tiers are nargnn_shared.h's with R edge rows and eight extra scratch rows (`part`, behind x, x1, x3):
//   tier 0 (N <= rl4co_nargnn_depot_lds_nodes(K)) at K = 10: N <= 43; at K = 20: N <= 25.
// A neighbour index outside [1, N) raises RL4CO_EBIT_TOUR_INDEX and the instance is left untouched: the lists are checked
// before anything is read through them. 0 is refused as well: it would repeat the depot edge, and two rows would write one
// heatmap entry.
#include <hip/hip_runtime.h>

#include "common.h"
#include "nargnn_shared.h"

namespace {

using namespace rl4co::nargnn;

__host__ __device__ constexpr int64_t edge_rows(int N, int K) { return (int64_t)(N - 1) * (K + 2); }

// The edge rows: customer ci's K + 1 rows (k == K: its depot edge) below D0, the depot's row to customer ci + 1 from D0 on.
struct Rows {
  const int32_t* nbr;
  int D0, K1, K;
  // is row e a customer's? then (ci, k) are its customer and place, otherwise ci is the customer the depot's row goes to
  __device__ __forceinline__ bool customer_row(int e, int& ci, int& k) const {
    if (e < D0) {
      ci = e / K1, k = e - ci * K1;
      return true;
    }
    ci = e - D0;
    return false;
  }
  // row e is (u -> v)
  __device__ __forceinline__ Edge operator()(int e) const {
    int ci, k;
    if (customer_row(e, ci, k)) return {ci + 1, k < K ? nbr[ci * K + k] : 0};
    return {0, ci + 1};
  }
};

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

  const Planes p = planes<TIER>(a.scratch + (int64_t)blockIdx.x * scratch_floats(TIER, N, edge_rows(N, K), kWaves), lds, N, R, kWaves);
  float *X = p.X, *X1 = p.X1, *X3 = p.X3, *PART = p.extra, *X2 = p.X2, *X4 = p.X4, *E = p.E;

  // the wave's customers (and depot rows) in B1 and its edge rows everywhere else, for every layer
  const int cpw = (C + kWaves - 1) / kWaves;
  const int c0 = min(C, w * cpw), c1 = min(C, c0 + cpw);
  const int rpw = (R + kWaves - 1) / kWaves;
  const int e0 = min(R, w * rpw), e1 = min(R, e0 + rpw);

  for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
    const int32_t* nbr = a.neighbors + (int64_t)b * CK;
    const Rows uv{nbr, D0, K1, K};
    if (neighbors_refused(bad_flag, nbr, CK, 1, N, tid)) {  // 0 would repeat the depot edge
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
        int ci, k;
        const float d = uv.customer_row(e, ci, k) && k < K ? cost[ci * K + k] : dcost[ci];
        E[e * kRS + lane] = siluf(d * we + be);
      }
    }

    for (int l = 0; l < a.L; ++l) {
      const float* LW = a.lin_w + (int64_t)l * 5 * kD * kD;
      const float* LB = a.lin_b + (int64_t)l * 5 * kD;
      const float* BN = a.bn + (int64_t)l * 4 * kD;
      __syncthreads();  // 1: x of every node is this layer's; the layer before has finished with x1 .. x4 and part

      node_gemms(X1, X2, X3, X4, X, LW, LB, N, w, lane);
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
      edge_update(E, X3, X4, LW, LB, BN, e0, e1, lane, c, g, uv);
    }
    mlp_rows(E, a.mlp_w, a.mlp_b, a.H, e0, e1, lane, c, g);

    // ---- the fill, then the output layer and the scatter of the own rows -------------------------------------------------------
    {
      float* hm = a.heatmap + (int64_t)b * N * N;
      for (int j = tid; j < N * N; j += kThreads) hm[j] = a.fill_value;
      // a heatmap row is filled by many waves and scattered into by others: the barrier waits for every fill store
      __syncthreads();
      output_rows(hm, E, a.out_w, a.out_b, a.small_value, N, e0, e1, lane, uv);
    }
  }
}

}  // namespace

extern "C" int rl4co_nargnn_depot_lds_nodes(int K) { return lds_nodes(K, edge_rows); }

extern "C" int64_t rl4co_nargnn_depot_scratch_bytes(int N, int K) {
  if (N < 3 || N > 1024 || K < 1 || K > 256 || K > N - 2) return 0;
  return scratch_floats(tier_of(N, edge_rows(N, K)), N, edge_rows(N, K), kWaves) * 4;
}

extern "C" int rl4co_nargnn_depot_heatmap(const rl4co_nargnn_depot_args* args, void* stream) {
  static_assert(lds_bytes(1, kNodeLdsMax, edge_rows(kNodeLdsMax, 1)) + kStaticLds <= kCuLds, "the node planes of tier 1 fit the LDS");
  static_assert(edge_rows(1024, 256) * kRS < (int64_t)1 << 31, "row offsets fit an int");
  RL4CO_REQUIRE(args != nullptr);
  const rl4co_nargnn_depot_args& a = *args;
  if (const int rc = require_model(a)) return rc;
  RL4CO_REQUIRE(a.N >= 3 && a.N <= 1024);
  RL4CO_REQUIRE(a.K >= 1 && a.K <= 256 && a.K <= a.N - 2);
  RL4CO_REQUIRE(a.F == 1 || a.F == 2);
  if (const int rc = require_depth_and_grid(a)) return rc;
  RL4CO_REQUIRE(a.locs != nullptr && a.feats != nullptr && a.neighbors != nullptr && a.edge_cost != nullptr && a.depot_cost != nullptr);
  RL4CO_REQUIRE(a.init_w != nullptr && a.init_b != nullptr && a.depot_w != nullptr && a.depot_b != nullptr);
  RL4CO_REQUIRE(a.edge_w != nullptr && a.edge_b != nullptr);
  if (const int rc = require_buffers(a, rl4co_nargnn_depot_scratch_bytes(a.N, a.K))) return rc;
  return launch_tier<nargnn_depot_kernel<0>, nargnn_depot_kernel<1>, nargnn_depot_kernel<2>>(a, edge_rows(a.N, a.K), stream);
}

// nargnn.hip — DeepACO's heatmap encoder for TSP (the reference's NARGNNEncoder in inference: models/zoo/nargnn/encoder.py,
// models/nn/graph/gnn.py, env_embeddings/edge.py) as one launch for gfx950, fp32 throughout. The scheme, the MFMA tiles, the
// tiers and their LDS budget are nargnn_shared.h's, shared with nargnn_depot.hip. What is the regular graph's own:
//
// Node u has exactly K out-edges, to neighbors[u][0 .. K-1], so the edge state is a dense [N K][64] array whose rows
// u K .. u K + K - 1 belong to node u: row e is (e / K -> neighbors[e]), and gnn.py's pooling by edge_index[0] is a sum
// over a node's own K rows. No extra scratch rows. A wave owns the NODES [n0, n1) and their rows [n0 K, n1 K) in every phase:
//   per layer   A  (node_gemms)
//               -- workgroup barrier --
//               B  for the own nodes: x[u] += silu(bn_v(x1[u] + sum_k(sigmoid(w[u][k]) * x2[v_k]) / K)) (lane = channel),
//                  then the edge update of the same nodes' rows, in tiles that start at n0 K
//               -- workgroup barrier (top of the next layer) --
//   then heatmap[u][:] = fill_value for the own nodes and, behind a release fence, heatmap[u][v_k] of the own rows.
// Both updates of a layer read the layer's incoming x and w: the node update of a wave's nodes runs before the edge update
// of the same nodes' rows, and x1 .. x4 were taken from x in A.
// Tier 0 (N <= rl4co_nargnn_lds_nodes(K)) at K = 10: N <= 50 (163 264 bytes of LDS); at K = 20: N <= 27.
// A neighbour index outside [0, N) raises RL4CO_EBIT_TOUR_INDEX and the instance is left untouched: the lists are checked
// before anything is read through them.
#include <hip/hip_runtime.h>

#include "common.h"
#include "nargnn_shared.h"

namespace {

using namespace rl4co::nargnn;

__host__ __device__ constexpr int64_t edge_rows(int N, int K) { return (int64_t)N * K; }

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

  const Planes p = planes<TIER>(a.scratch + (int64_t)blockIdx.x * scratch_floats(TIER, N, edge_rows(N, K), 0), lds, N, NK, 0);
  float *X = p.X, *X1 = p.X1, *X3 = p.X3, *X2 = p.X2, *X4 = p.X4, *E = p.E;

  // the wave's own nodes and edge rows, for every layer
  const int npw = (N + kWaves - 1) / kWaves;
  const int n0 = min(N, w * npw), n1 = min(N, n0 + npw);
  const int e0 = n0 * K, e1 = n1 * K;

  for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
    const int32_t* nbr = a.neighbors + (int64_t)b * NK;
    const auto uv = [&](int e) { return Edge{e / K, nbr[e]}; };
    if (neighbors_refused(bad_flag, nbr, NK, 0, N, tid)) {
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
      node_gemms(X1, X2, X3, X4, X, LW, LB, N, w, lane);
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

      edge_update(E, X3, X4, LW, LB, BN, e0, e1, lane, c, g, uv);
    }
    mlp_rows(E, a.mlp_w, a.mlp_b, a.H, e0, e1, lane, c, g);

    // ---- the output layer and the heatmap rows of the own nodes -------------------------------------------------------------
    {
      float* hm = a.heatmap + (int64_t)b * N * N;
      for (int u = n0; u < n1; ++u)
        for (int j = lane; j < N; j += 64) hm[u * N + j] = a.fill_value;
      // the fill has reached memory before a neighbour entry of the same row is stored over it
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      output_rows(hm, E, a.out_w, a.out_b, a.small_value, N, e0, e1, lane, uv);
    }
  }
}

}  // namespace

extern "C" int rl4co_nargnn_lds_nodes(int K) { return lds_nodes(K, edge_rows); }

extern "C" int64_t rl4co_nargnn_scratch_bytes(int N, int K) {
  if (N < 2 || N > 1024 || K < 1 || K > 256) return 0;
  return scratch_floats(tier_of(N, edge_rows(N, K)), N, edge_rows(N, K), 0) * 4;
}

extern "C" int rl4co_nargnn_heatmap(const rl4co_nargnn_args* args, void* stream) {
  static_assert(lds_bytes(1, kNodeLdsMax, edge_rows(kNodeLdsMax, 1)) + kStaticLds <= kCuLds, "the node planes of tier 1 fit the LDS");
  RL4CO_REQUIRE(args != nullptr);
  const rl4co_nargnn_args& a = *args;
  if (const int rc = require_model(a)) return rc;
  RL4CO_REQUIRE(a.N >= 2 && a.N <= 1024);
  RL4CO_REQUIRE(a.K >= 1 && a.K <= 256 && a.K <= a.N - 1);
  if (const int rc = require_depth_and_grid(a)) return rc;
  RL4CO_REQUIRE(a.reserved0 == 0);
  RL4CO_REQUIRE(a.locs != nullptr && a.neighbors != nullptr && a.edge_cost != nullptr);
  RL4CO_REQUIRE(a.init_w != nullptr && a.init_b != nullptr && a.edge_w != nullptr && a.edge_b != nullptr);
  if (const int rc = require_buffers(a, rl4co_nargnn_scratch_bytes(a.N, a.K))) return rc;
  return launch_tier<nargnn_kernel<0>, nargnn_kernel<1>, nargnn_kernel<2>>(a, edge_rows(a.N, a.K), stream);
}

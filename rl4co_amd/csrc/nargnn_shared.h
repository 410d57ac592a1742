// nargnn_shared.h — the scheme of DeepACO's heatmap encoder (the reference's NARGNNEncoder in inference), stated once for its
// two kernels: nargnn.hip (the regular TSP graph) and nargnn_depot.hip (the depot graph of CVRP, OP and PCTSP). Here: the
// 68-float row and the MFMA tile product, the tiers, what they cost in LDS and scratch and the carve-up of a workgroup's
// planes, the neighbour-list check, the four node GEMMs of a layer, the three loops over a wave's own rows (edge update,
// heatmap MLP, output row), the launch and the host requirements both argument structs share. Each kernel adds what is
// particular to its graph: the edge rows and which of them a wave owns, the init embedding and the cost gather, the node
// sums (B1), the map from an edge row to its nodes (u, v) and the heatmap fill.
//
// One workgroup of eight waves per INSTANCE, persistent over the layers, grid-stride over the instances, fp32 throughout.
// The edge state is a dense [edge rows][64] array w, the node state x [N][64]:
//   the neighbour lists are range-checked before anything is read through them (neighbors_refused)
//   x = silu(init(...)); w = silu(edge_embed(cost))
//   per layer   A  x1 .. x4 = v_lin1 .. v_lin4 (x) for every node (node_gemms: MFMA; wave = one matrix, every other tile)
//               -- workgroup barrier --
//               B1 x[u] += silu(bn_v(x1[u] + mean over u's rows of sigmoid(w[e]) * x2[v]))        (lane = channel)
//               B2 w[e] += silu(bn_e((e_lin(w[e]) + x3[u]) + x4[v])) for the wave's OWN rows [e0, e1) (edge_update), in 16-row
//                  MFMA tiles that start at e0 (clamped on load, masked on store at e1): in place, a row is read by its own
//                  tile only
//   heatmap MLP on the own rows, layer by layer in place (mlp_rows; wave-local: no workgroup barrier), then the 64 -> 1
//   output as a wave reduction per row and heatmap[u][v] = log(sigmoid(out) + small_value) (output_rows) over the kernel's
//   fill with fill_value.
// Both updates of a layer read the layer's incoming x and w; how a kernel orders B1 before B2 is its own.
//
// MFMA v_mfma_f32_16x16x4_f32, operands as csrc/enc_f32.h states them: lane = 16 g + c holds A[row c][k-slot g] and
// B[k-slot g][col c]; a lane's 16-byte fragment (k = 16 j + 4 g .. + 3) feeds four steps, component s of both operands in
// step s. B is the weight row-major as torch keeps it ([out][in]): lane (c, g) of column tile ct reads
// W[16 ct + c][16 j + 4 g ..]. A wave holds one matrix (16 fragments, 64 VGPRs) for all of its row tiles. D[row 4 g + r]
// [col 16 ct + c] arrives in register r of accumulator ct. The sum over the 64 inputs is the hardware's (16 steps of 4).
//
// Where the state lives (rows of kRS = 68 floats: the 16 lanes of one g read 16 distinct bank quads), by the graph's edge
// rows R and the extra scratch rows X a kernel asks for (planes):
//   tier 0  N <= *_lds_nodes(K): x2, x4 and the edge state in LDS; x, x1, x3 and the extra rows in `scratch`
//   tier 1  N <= 300: x2, x4 in LDS; the edge state and x, x1, x3, the extra rows in `scratch`
//   tier 2  up to 1024 nodes: everything in `scratch`
// `scratch` is sized by the grid, not by B; a workgroup's slice is read and written by that workgroup only, so workgroup
// barriers (and, inside a wave, a workgroup-scope fence) order it. x, x1 and x3 are read by the node that owns them or as
// MFMA rows once per layer; only x2 and x4 are gathered through the neighbour lists.
// LDS budget (bytes, all dynamic; the launcher checks that the compiler added no static LDS beyond kStaticLds):
//   head 64 (the bad-index flag) + 272 (2 N + R) in tier 0 | 272 * 2 N in tier 1 | nothing more in tier 2.
// scratch rows per workgroup: 3 N + X, + R in tiers 1 and 2, + 2 N in tier 2.
#pragma once
#include <hip/hip_runtime.h>

#include "common.h"

namespace rl4co {
namespace nargnn {

constexpr int kD = 64;
constexpr int kRS = kD + 4;  // a row of 68 floats: the 16 lanes of one g read 16 distinct bank quads
constexpr int kThreads = 512;
constexpr int kWaves = kThreads / 64;
constexpr int kCuLds = 160 * 1024;
constexpr int kStaticLds = 64;
constexpr int kHeadBytes = 64;
constexpr int kNodeLdsMax = 300;  // tier 1: 64 + 2 * 300 * 272 + 64 <= 160 KiB

typedef float f32x4 __attribute__((ext_vector_type(4)));
struct Edge {
  int u, v;  // an edge row's nodes: (u -> v)
};

// ---- the tiers, over a graph's edge rows and a kernel's extra scratch rows ---------------------------------------------------
__host__ __device__ constexpr int64_t lds_bytes(int tier, int N, int64_t edge_rows) {
  const int64_t rows = tier == 0 ? 2 * (int64_t)N + edge_rows : (tier == 1 ? 2 * (int64_t)N : 0);
  return kHeadBytes + rows * kRS * 4;
}
__host__ __device__ constexpr int64_t scratch_floats(int tier, int N, int64_t edge_rows, int extra_rows) {
  const int64_t rows = 3 * (int64_t)N + extra_rows + (tier >= 1 ? edge_rows : 0) + (tier == 2 ? 2 * (int64_t)N : 0);
  return rows * kRS;
}
inline int tier_of(int N, int64_t edge_rows) {
  if (lds_bytes(0, N, edge_rows) + kStaticLds <= kCuLds) return 0;
  return N <= kNodeLdsMax ? 1 : 2;
}
// the largest N whose tier is 0 at K; `edge_rows` of (N, K)
template <typename RowsFn>
inline int lds_nodes(int K, RowsFn edge_rows) {
  if (K < 1) return 0;
  int n = 1024;
  while (n > 0 && lds_bytes(0, n, edge_rows(n, K)) + kStaticLds > kCuLds) --n;
  return n;
}

// a workgroup's planes: `gs` its slice of the scratch, `lds` the dynamic LDS behind the head; `extra`: the kernel's
// `extra_rows` rows
struct Planes {
  float *X, *X1, *X3, *extra, *X2, *X4, *E;
};
template <int TIER>
__device__ __forceinline__ Planes planes(float* gs, float* lds, int N, int edge_rows, int extra_rows) {
  Planes p;
  p.X = gs;
  p.X1 = gs + N * kRS;
  p.X3 = gs + 2 * N * kRS;
  p.extra = gs + 3 * N * kRS;
  float* after = p.extra + extra_rows * kRS;
  if constexpr (TIER == 0) {
    p.X2 = lds;
    p.X4 = lds + N * kRS;
    p.E = lds + 2 * N * kRS;
  } else if constexpr (TIER == 1) {
    p.X2 = lds;
    p.X4 = lds + N * kRS;
    p.E = after;
  } else {
    p.E = after;
    p.X2 = p.E + (int64_t)edge_rows * kRS;
    p.X4 = p.X2 + N * kRS;
  }
  return p;
}

// ---- device pieces -----------------------------------------------------------------------------------------------------------
__device__ inline float sigmoidf(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ inline float siluf(float x) { return x / (1.0f + expf(-x)); }

__device__ inline f32x4 mfma4(float a, float b, const f32x4& c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// the wave's copy of one 64 x 64 weight, row-major [out][in]: fragment [ct][j] of lane (c, g) is W[16 ct + c][16 j + 4 g ..]
__device__ inline void load_wfrags(f32x4 (&wf)[4][4], const float* W, int lane) {
  const float* row = W + (lane & 15) * kD + 4 * (lane >> 4);
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
#pragma unroll
    for (int j = 0; j < 4; ++j) wf[ct][j] = *reinterpret_cast<const f32x4*>(row + 16 * ct * kD + 16 * j);
}

// acc[ct] = (16 rows) . W^T for the four column tiles; `arow` is the lane's row c at float 4 g
__device__ inline void gemm_tile(f32x4 (&acc)[4], const f32x4 (&wf)[4][4], const float* arow) {
  f32x4 a[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) a[j] = *reinterpret_cast<const f32x4*>(arow + 16 * j);
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) acc[ct] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) acc[ct] = mfma4(a[j][s], wf[ct][j][s], acc[ct]);
}

// Y[n] = X[n] . W^T + bias for the node tiles tile0, tile0 + 2, ...
__device__ inline void node_gemm(float* Y, const float* X, const float* W, const float* bias, int N, int tile0, int lane) {
  const int c = lane & 15, g = lane >> 4;
  f32x4 wf[4][4];
  load_wfrags(wf, W, lane);
  float bcol[4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) bcol[ct] = bias[16 * ct + c];
  const int tiles = (N + 15) >> 4;
  for (int t = tile0; t < tiles; t += 2) {
    const int row = min(16 * t + c, N - 1);  // rows past N repeat the last node and are not stored
    f32x4 acc[4];
    gemm_tile(acc, wf, X + row * kRS + 4 * g);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = 16 * t + 4 * g + r;
      if (n < N) {
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) Y[n * kRS + 16 * ct + c] = acc[ct][r] + bcol[ct];
      }
    }
  }
}

// The neighbour lists, before anything is read through them: is any of nbr[0 .. count) outside [lo, N)? Uniform over the
// workgroup (one LDS word, three workgroup barriers); the caller raises RL4CO_EBIT_TOUR_INDEX and skips a refused instance.
__device__ __forceinline__ bool neighbors_refused(uint32_t* bad_flag, const int32_t* nbr, int count, int lo, int N, int tid) {
  if (tid == 0) *bad_flag = 0u;
  __syncthreads();
  bool bad = false;
  for (int e = tid; e < count; e += kThreads) {
    const int v = nbr[e];
    bad |= v < lo || v >= N;
  }
  if (bad) *bad_flag = 1u;
  __syncthreads();
  const bool refused = *bad_flag != 0u;  // (uniform: one LDS word)
  __syncthreads();                       // the word is reset at the top of the next instance
  return refused;
}

// A. x1 .. x4 of every node from the layer's v_lin1 .. v_lin4 (LW, LB): wave w takes matrix w & 3, node tiles w >> 2, + 2, ...
__device__ __forceinline__ void node_gemms(float* X1, float* X2, float* X3, float* X4, const float* X, const float* LW,
                                           const float* LB, int N, int w, int lane) {
  const int m = w & 3, tile0 = w >> 2;  // (wave-uniform)
  const float* Wm = LW + m * kD * kD;
  const float* bm = LB + m * kD;
  if (m == 0) node_gemm(X1, X, Wm, bm, N, tile0, lane);
  else if (m == 1) node_gemm(X2, X, Wm, bm, N, tile0, lane);
  else if (m == 2) node_gemm(X3, X, Wm, bm, N, tile0, lane);
  else node_gemm(X4, X, Wm, bm, N, tile0, lane);
}

// The three loops over a wave's own rows [e0, e1). `uv(e)` returns row e's Edge{u, v}. `c` and `g` MUST be lane & 15 and
// lane >> 4: the kernel takes them once and hands them in, because taken again in here they cost it VGPRs.
// B2. the edge update, in place
template <typename UV>
__device__ __forceinline__ void edge_update(float* E, const float* X3, const float* X4, const float* LW, const float* LB,
                                            const float* BN, int e0, int e1, int lane, int c, int g, const UV& uv) {
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
        const Edge uv_e = uv(e);
        const int u = uv_e.u, v = uv_e.v;
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

// the heatmap MLP: layer by layer in place, wave-local
__device__ __forceinline__ void mlp_rows(float* E, const float* mlp_w, const float* mlp_b, int H, int e0, int e1, int lane,
                                         int c, int g) {
  for (int h = 0; h + 1 < H; ++h) {
    rl4co::lds_barrier_wave();  // rows written in one lane layout are read in another, by this wave only
    f32x4 wf[4][4];
    load_wfrags(wf, mlp_w + (int64_t)h * kD * kD, lane);
    float bcol[4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) bcol[ct] = mlp_b ? mlp_b[h * kD + 16 * ct + c] : 0.0f;
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
}

// the output layer and the rows' entries hm[u][v] of the instance's (filled) heatmap
template <typename UV>
__device__ __forceinline__ void output_rows(float* hm, const float* E, const float* out_w, const float* out_b, float small_value,
                                            int N, int e0, int e1, int lane, const UV& uv) {
  const float wo = out_w[lane];
  const float bo = out_b ? out_b[0] : 0.0f;
  for (int e = e0; e < e1; ++e) {
    const float p = rl4co::bfly_sum<1, 64>(E[e * kRS + lane] * wo);
    if (lane == 0) {
      const Edge uv_e = uv(e);
      const int u = uv_e.u, v = uv_e.v;
      hm[u * N + v] = logf(sigmoidf(p + bo) + small_value);
    }
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
template <auto Kernel, typename Args>
int launch(const Args& a, int lds, hipStream_t stream) {
  hipFuncAttributes fa;
  RL4CO_HIP_TRY(hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(Kernel)));
  RL4CO_REQUIRE((int64_t)fa.sharedSizeBytes <= kStaticLds);  // the budget behind *_lds_nodes() holds
  if (lds > 64 * 1024) {
    RL4CO_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  }
  hipLaunchKernelGGL(Kernel, dim3(a.n_workgroups), dim3(kThreads), lds, stream, a);
  RL4CO_HIP_TRY(hipGetLastError());
  return RL4CO_OK;
}
// the kernel of the tier that (N, edge_rows) falls into
template <auto Tier0, auto Tier1, auto Tier2, typename Args>
int launch_tier(const Args& a, int64_t edge_rows, void* stream) {
  hipStream_t s = rl4co::as_stream(stream);
  switch (tier_of(a.N, edge_rows)) {
    case 0: return launch<Tier0>(a, (int)lds_bytes(0, a.N, edge_rows), s);
    case 1: return launch<Tier1>(a, (int)lds_bytes(1, a.N, edge_rows), s);
    default: return launch<Tier2>(a, (int)lds_bytes(2, a.N, edge_rows), s);
  }
}

// The requirements rl4co_nargnn_args and rl4co_nargnn_depot_args share, in the three runs between which an entry point
// states its own (N, K and the features; its inputs and their embeddings), so that the first one to fail is the same
// whichever are broken.
template <typename Args>
int require_model(const Args& a) {
  RL4CO_REQUIRE(a.D == kD);
  RL4CO_REQUIRE(a.B >= 1);
  return RL4CO_OK;
}
template <typename Args>
int require_depth_and_grid(const Args& a) {
  RL4CO_REQUIRE(a.L >= 0 && a.L <= (1 << 20));
  RL4CO_REQUIRE(a.H >= 1 && a.H <= (1 << 20));
  RL4CO_REQUIRE(a.n_workgroups >= 1 && a.n_workgroups <= a.B);
  return RL4CO_OK;
}
// `per_workgroup_bytes`: the entry point's *_scratch_bytes(a.N, a.K)
template <typename Args>
int require_buffers(const Args& a, int64_t per_workgroup_bytes) {
  RL4CO_REQUIRE(a.L == 0 || (a.lin_w != nullptr && a.lin_b != nullptr && a.bn != nullptr));
  RL4CO_REQUIRE(a.H == 1 || a.mlp_w != nullptr);
  RL4CO_REQUIRE(a.out_w != nullptr);
  RL4CO_REQUIRE(((reinterpret_cast<uintptr_t>(a.lin_w) | reinterpret_cast<uintptr_t>(a.mlp_w)) & 15) == 0);  // 16-byte fragments
  RL4CO_REQUIRE(a.scratch != nullptr);
  RL4CO_REQUIRE((reinterpret_cast<uintptr_t>(a.scratch) & 15) == 0);
  RL4CO_REQUIRE(a.scratch_bytes >= (int64_t)a.n_workgroups * per_workgroup_bytes);
  RL4CO_REQUIRE(a.heatmap != nullptr && a.node_embed != nullptr && a.err != nullptr);
  return RL4CO_OK;
}

}  // namespace nargnn
}  // namespace rl4co

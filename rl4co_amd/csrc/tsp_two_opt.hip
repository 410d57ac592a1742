// tsp_two_opt.hip — TSP local search: best-improvement 2-opt (envs/routing/tsp/local_search.py) as one launch for gfx950.
//
// One workgroup of four waves per TOUR runs the whole search of that tour: per iteration the arg-min of `change` over the
// (T-1)(T-2)/2 position pairs 1 <= i < j <= T-1 and, when the winner is below -1e-6, the reversal of tour[i..j]; it ends
// at the first iteration without such a move or at max_iterations. The answer is fully determined — the reference's
// sequential scan keeps the FIRST pair of the smallest change — and the kernel reproduces it bit for bit:
//   change   ((d[prev][tour[j]] + d[tour[i]][next]) - d[prev][tour[i]]) - d[tour[j]][next], prev = tour[i-1],
//            next = tour[(j+1) % T]: fp32, one rounding per operation, this association, this index order (an asymmetric
//            matrix is served), -ffp-contract=off. A pair with prev == tour[j] or next == tour[i] is skipped.
//   winner   the lexicographically smallest (change, i, j) among the pairs with change < 0 (NaN and -0.0 are not below 0).
//            Each thread keeps the minimum of a 64-bit key: the order-preserving image of `change` (NaN above everything)
//            in the high word, (i << 16) | j in the low word, so equal changes go to the lowest (i, j) however the pairs
//            are dealt. Pairs are dealt flat: thread k takes pairs k, k + 256, ... of the (i, j)-ordered list.
//   reduce   wave butterfly (common.h), lane 0 of each wave stores its key, workgroup barrier, EVERY thread reads the same
//            four LDS words and folds them in the same order: the move / stop decision is uniform by construction.
//   move     widened to double, change < -1e-6 (the reference compares in double): threads k < (j - i + 1) / 2 swap
//            tour[i + k] and tour[j - k]; workgroup barrier; next iteration. `iterations` counts the last, non-improving
//            scan too. No barrier sits inside divergent control flow; the only loop is bounded by max_iterations.
//
// Distances (one kernel template over the three sources, one text of the search loop: tsp_two_opt_search.h, which
// tsp_nls.hip calls too):
//   kMatrix   N <= rl4co_tsp_two_opt_lds_nodes(): the N x N fp32 matrix of the instance in LDS, 1e9 added on its diagonal —
//             built by the workgroup from `locs`, or staged once from `distances` with coalesced loads.
//   kCoords   above that, from `locs`: the coordinates in LDS (8 N bytes), every d[a][b] computed where it is used.
//   kGlobal   above that, from `distances`: entries read from global memory (the caches serve the re-reads).
//   From coordinates d[a][b] = sqrtf(fmaf(dy, dy, dx * dx)), dx = x_a - x_b, dy = y_a - y_b: the expression of
//   tour_length.hip, bit-identical to ATen's norm(p=2) over two elements, in kMatrix and kCoords alike; d[a][a] = 1e9.
//
// A tour holding an index outside [0, N) raises RL4CO_EBIT_TOUR_INDEX and is copied through unchanged with 0 iterations:
// the index is only compared, nothing is read through it.
//
// LDS budget (bytes, all dynamic; the kernel declares no static LDS and the launcher checks that the compiler added none
// beyond kStaticLds):
//   reduction scratch    64             (four 64-bit wave keys, the bad-index flag)
//   tour                 2 * 1024       (uint16_t, T <= 1024)
//   distances            4 N^2 (kMatrix) | 8 N (kCoords) | 0 (kGlobal)
//   static               <= 64
//   4 N^2 + 2 * 1024 + 64 + 64 <= 160 KiB  =>  N <= 201 (4 * 201^2 = 161 604): rl4co_tsp_two_opt_lds_nodes().
// Design estimates, NOT measured: at N = 100 a workgroup takes 42 112 B of LDS, so three workgroups (12 waves) share a
// CU; above N = 142 (80 KiB) one workgroup per CU. Nothing about this kernel's occupancy or time has been profiled
// (tools/two_opt_bench.py records the end-to-end time only).
#include <hip/hip_runtime.h>

#include "common.h"
#include "tsp_two_opt_search.h"

namespace {

using namespace rl4co::two_opt;  // tsp_two_opt_search.h: the constants, Distances<SRC>, staging and the search loop

template <int SRC>
__global__ void __launch_bounds__(kThreads) tsp_two_opt_kernel(const rl4co_tsp_two_opt_args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint64_t* red = reinterpret_cast<uint64_t*>(smem);                   // [kWaves]
  uint32_t* bad_flag = reinterpret_cast<uint32_t*>(smem + 8 * kWaves);
  uint16_t* tour = reinterpret_cast<uint16_t*>(smem + kRedBytes);      // [T]
  float* payload = reinterpret_cast<float*>(smem + kRedBytes + kTourBytes);

  const int tid = threadIdx.x;
  const int N = a.N, T = a.T;
  const int64_t row = (int64_t)blockIdx.x * T;
  const int64_t* in = a.actions + row;
  int64_t* out = a.out_actions + row;

  // ---- the tour: range check, then uint16_t in LDS -----------------------------------------------------------------
  if (tid == 0) *bad_flag = 0u;
  __syncthreads();
  bool bad = false;
  for (int t = tid; t < T; t += kThreads) {
    const int64_t v = in[t];
    if (v < 0 || v >= N) bad = true;
    tour[t] = (uint16_t)v;
  }
  if (bad) *bad_flag = 1u;
  __syncthreads();
  if (*bad_flag) {  // (uniform: one LDS word) the tour goes through as it came; every thread moves its own elements
    if (out != in)
      for (int t = tid; t < T; t += kThreads) out[t] = in[t];
    if (tid == 0) {
      if (a.iterations) a.iterations[blockIdx.x] = 0;
      atomicOr(a.err, RL4CO_EBIT_TOUR_INDEX);
    }
    return;
  }

  // ---- the distances ----------------------------------------------------------------------------------------------
  Distances<SRC> dist;
  dist.N = N;
  dist.mat = nullptr;
  dist.xy = nullptr;
  if constexpr (SRC == kMatrix) {
    if (a.locs) {
      stage_matrix_from_locs(payload, reinterpret_cast<const float2*>(a.locs) + (int64_t)blockIdx.x * N, N, tid);
    } else {
      stage_matrix_from_distances(payload, a.distances + (int64_t)blockIdx.x * N * N, N, tid);
    }
    dist.mat = payload;
  } else if constexpr (SRC == kCoords) {
    const float2* xy = reinterpret_cast<const float2*>(a.locs) + (int64_t)blockIdx.x * N;
    float2* lxy = reinterpret_cast<float2*>(payload);
    for (int e = tid; e < N; e += kThreads) lxy[e] = xy[e];
    dist.xy = lxy;
  } else {
    dist.mat = a.distances + (int64_t)blockIdx.x * N * N;
  }
  __syncthreads();

  // ---- the search -------------------------------------------------------------------------------------------------
  const int it = search(dist, tour, red, T, a.max_iterations, tid);  // tsp_two_opt_search.h

  for (int t = tid; t < T; t += kThreads) out[t] = (int64_t)tour[t];
  if (tid == 0 && a.iterations) a.iterations[blockIdx.x] = it;
}

template <int SRC>
int launch(const rl4co_tsp_two_opt_args& a, hipStream_t stream) {
  const int lds = (int)two_opt_lds_bytes(SRC, a.N);
  hipFuncAttributes fa;
  RL4CO_HIP_TRY(hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(tsp_two_opt_kernel<SRC>)));
  RL4CO_REQUIRE((int64_t)fa.sharedSizeBytes <= kStaticLds);  // the budget of rl4co_tsp_two_opt_lds_nodes holds
  if (lds > 64 * 1024) {
    RL4CO_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(tsp_two_opt_kernel<SRC>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  }
  hipLaunchKernelGGL((tsp_two_opt_kernel<SRC>), dim3(a.B), dim3(kThreads), lds, stream, a);
  RL4CO_HIP_TRY(hipGetLastError());
  return RL4CO_OK;
}

}  // namespace

extern "C" int rl4co_tsp_two_opt_lds_nodes(void) {
  int n = kMaxTour;
  while (n > 0 && two_opt_lds_bytes(kMatrix, n) + kStaticLds > kCuLds) --n;
  return n;
}

extern "C" int rl4co_tsp_two_opt(const rl4co_tsp_two_opt_args* args, void* stream) {
  RL4CO_REQUIRE(args != nullptr);
  const rl4co_tsp_two_opt_args& a = *args;
  RL4CO_REQUIRE(a.B >= 1);
  RL4CO_REQUIRE(a.N >= 2 && a.N <= 1024);
  RL4CO_REQUIRE(a.T >= 1 && a.T <= 1024);
  RL4CO_REQUIRE(a.max_iterations >= 0);
  RL4CO_REQUIRE((a.locs != nullptr) != (a.distances != nullptr));  // exactly one distance source
  RL4CO_REQUIRE(a.actions != nullptr);
  RL4CO_REQUIRE(a.out_actions != nullptr);
  RL4CO_REQUIRE(a.err != nullptr);
  hipStream_t s = rl4co::as_stream(stream);
  if (a.N <= rl4co_tsp_two_opt_lds_nodes()) return launch<kMatrix>(a, s);
  return a.locs ? launch<kCoords>(a, s) : launch<kGlobal>(a, s);
}

// tsp_nls.hip — neural-guided local search for TSP (DeepACO's NLS: models/zoo/deepaco/antsystem.py:173-230) as one launch
// for gfx950.
//
// One workgroup of four waves per TOUR ROW runs the whole of the reference's AntSystem.local_search(use_nls=True) of that
// row, the tour in LDS throughout:
//   cur  = two_opt(real, cur, ls_max_iterations)
//   best = cur (written to out_actions[row]); best_r = reward(cur)
//   repeat n_perturbations times:
//     cur = two_opt(perturb, cur, perturb_max_iterations)     the learned heatmap's matrix throws the tour off its optimum
//     cur = two_opt(real,    cur, ls_max_iterations)          and the real distances repair it
//     r   = reward(cur)
//     if r > best_r: out_actions[row] = cur; best_r = r       fp32 '>', NaN never wins
//     (cur carries on whether or not it won: the reference's new_actions)
//   out_reward[row] = best_r
// Row r uses instance r % n_instances (the ant-major layout rl4co_aco_tsp produces): neither `locs` nor the perturbation
// matrix is tiled per ant.
//   two_opt  tsp_two_opt_search.h: the search of tsp_two_opt.hip itself, every rule of that file's header unchanged. `real`
//            is the matrix of `locs` (d[a][b] = sqrtf(fmaf(dy, dy, dx * dx)), 1e9 on the diagonal), `perturb` is
//            perturb_distances with 1e9 added on its diagonal (local_search.py:38); it may be asymmetric.
//   reward   lds_tour_reward.h: minus the closed tour length from `locs`, bit-equal to TSPEnv.get_reward /
//            rl4co_tour_length_f32. Wave 0 computes it and leaves it in one LDS word; behind a workgroup barrier every
//            thread reads that word: the accept decision is uniform by construction.
//   best     lives in out_actions (global memory): written after the first search and again on each accepted round, every
//            thread storing its own elements of the LDS tour. LDS holds one tour only.
// No barrier sits inside divergent control flow; every loop is bounded by one of the three counts (or by N, T).
//
// Distances (one kernel template, two tiers):
//   LDS       N <= rl4co_tsp_nls_lds_nodes(): ONE N x N matrix slot in LDS, restaged at each phase switch (1 + 2 *
//             n_perturbations stagings): built by the workgroup from `locs` for a real phase, loaded coalesced from
//             perturb_distances for a perturbation phase. Both phases search through Distances<kMatrix>.
//   above     up to 1024 nodes: the coordinates stay in LDS (8 N bytes) and the real phases use Distances<kCoords>; the
//             perturbation phases read global memory through Distances<kGlobal>.
//   Holding both matrices at once would spare the restaging but double the LDS of a workgroup; whether that pays at
//   N <= 140 is NOT measured.
//
// A tour holding an index outside [0, N) raises RL4CO_EBIT_TOUR_INDEX and is copied through unchanged with reward NaN, zero
// scans and zero accepted: the index is only compared, nothing is read through it.
//
// LDS budget (bytes, all dynamic; the launcher checks that the compiler added no static LDS beyond kStaticLds):
//   scratch              64             (four 64-bit wave keys, the bad-index flag, the reward word: 40 bytes used)
//   tour                 2 * 1024       (uint16_t, T <= 1024)
//   distances            4 N^2 (LDS tier) | 8 N (above)
//   static               <= 64
//   4 N^2 + 2 * 1024 + 64 + 64 <= 160 KiB  =>  N <= 201: rl4co_tsp_nls_lds_nodes() == rl4co_tsp_two_opt_lds_nodes().
// Design estimates, NOT measured: the LDS of a workgroup is the 2-opt kernel's (42 112 B at N = 100, three workgroups per
// CU); a restaging at N = 100 moves 40 000 B per workgroup, against scans of 4 851 pairs each. Nothing about this kernel's
// occupancy or time has been profiled (tools/aco_bench.py --nls records the end-to-end time only).
#include <hip/hip_runtime.h>

#include "common.h"
#include "lds_tour_reward.h"
#include "tsp_two_opt_search.h"

namespace {

using namespace rl4co::two_opt;

__host__ __device__ inline int64_t nls_lds_bytes(bool lds, int N) { return two_opt_lds_bytes(lds ? kMatrix : kCoords, N); }

template <bool LDS>
__global__ void __launch_bounds__(kThreads) tsp_nls_kernel(const rl4co_tsp_nls_args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint64_t* red = reinterpret_cast<uint64_t*>(smem);                       // [kWaves]
  uint32_t* bad_flag = reinterpret_cast<uint32_t*>(smem + 8 * kWaves);
  float* reward_word = reinterpret_cast<float*>(smem + 8 * kWaves + 4);
  uint16_t* tour = reinterpret_cast<uint16_t*>(smem + kRedBytes);          // [T]
  float* payload = reinterpret_cast<float*>(smem + kRedBytes + kTourBytes);

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int N = a.N, T = a.T;
  const int phases = 1 + 2 * a.n_perturbations;
  const int64_t r = blockIdx.x;
  const int64_t inst = r % a.n_instances;
  const int64_t* in = a.actions + r * T;
  int64_t* out = a.out_actions + r * T;
  int32_t* scans = a.scans ? a.scans + r * phases : nullptr;

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
    if (scans)
      for (int p = tid; p < phases; p += kThreads) scans[p] = 0;
    if (tid == 0) {
      a.out_reward[r] = __builtin_nanf("");
      if (a.accepted) a.accepted[r] = 0;
      atomicOr(a.err, RL4CO_EBIT_TOUR_INDEX);
    }
    return;
  }

  const float2* xy = reinterpret_cast<const float2*>(a.locs) + inst * N;
  const float* pert = a.perturb_distances + inst * N * N;
  Distances<LDS ? kMatrix : kCoords> real;
  Distances<LDS ? kMatrix : kGlobal> perturb;
  real.N = perturb.N = N;
  real.mat = perturb.mat = nullptr;
  real.xy = perturb.xy = nullptr;
  if constexpr (LDS) {
    real.mat = perturb.mat = payload;  // the one slot: staged before each phase
  } else {
    float2* lxy = reinterpret_cast<float2*>(payload);
    for (int e = tid; e < N; e += kThreads) lxy[e] = xy[e];
    real.xy = lxy;
    perturb.mat = pert;
  }
  rl4co::AntTour tv;
  tv.tour = tour;
  tv.xy = xy;
  tv.n = T;

  // One phase: the slot restaged where there is one, a workgroup barrier (it also separates this search's writes of red[]
  // from the reads of the search before), the search.
  auto real_phase = [&]() -> int {
    if constexpr (LDS) stage_matrix_from_locs(payload, xy, N, tid);
    __syncthreads();
    return search(real, tour, red, T, a.ls_max_iterations, tid);
  };
  auto perturb_phase = [&]() -> int {
    if constexpr (LDS) stage_matrix_from_distances(payload, pert, N, tid);
    __syncthreads();
    return search(perturb, tour, red, T, a.perturb_max_iterations, tid);
  };
  // The reward of the LDS tour in every thread: wave 0 computes, one LDS word carries it over a workgroup barrier. The
  // word is rewritten only behind the barriers of the next round's phases.
  auto reward = [&]() -> float {
    if (w == 0) {  // (wave-uniform)
      const float rew = rl4co::ant_reward(tv, lane);
      if (lane == 0) *reward_word = rew;
    }
    __syncthreads();
    return *reward_word;
  };

  int it = real_phase();
  if (tid == 0 && scans) scans[0] = it;
  for (int t = tid; t < T; t += kThreads) out[t] = (int64_t)tour[t];
  float best_r = reward();
  int accepted = 0;
  for (int p = 0; p < a.n_perturbations; ++p) {
    it = perturb_phase();
    if (tid == 0 && scans) scans[1 + 2 * p] = it;
    it = real_phase();
    if (tid == 0 && scans) scans[2 + 2 * p] = it;
    const float rew = reward();
    if (rew > best_r) {  // (uniform: one LDS word) NaN never wins
      for (int t = tid; t < T; t += kThreads) out[t] = (int64_t)tour[t];
      best_r = rew;
      ++accepted;
    }
  }
  if (tid == 0) {
    a.out_reward[r] = best_r;
    if (a.accepted) a.accepted[r] = accepted;
  }
}

template <bool LDS>
int launch(const rl4co_tsp_nls_args& a, hipStream_t stream) {
  const int lds = (int)nls_lds_bytes(LDS, a.N);
  hipFuncAttributes fa;
  RL4CO_HIP_TRY(hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(tsp_nls_kernel<LDS>)));
  RL4CO_REQUIRE((int64_t)fa.sharedSizeBytes <= kStaticLds);  // the budget of rl4co_tsp_nls_lds_nodes holds
  if (lds > 64 * 1024) {
    RL4CO_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(tsp_nls_kernel<LDS>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  }
  hipLaunchKernelGGL((tsp_nls_kernel<LDS>), dim3(a.R), dim3(kThreads), lds, stream, a);
  RL4CO_HIP_TRY(hipGetLastError());
  return RL4CO_OK;
}

}  // namespace

extern "C" int rl4co_tsp_nls_lds_nodes(void) {
  static_assert(8 * kWaves + 4 + 4 <= kRedBytes, "wave keys, bad-index flag and reward word fit the scratch");
  int n = kMaxTour;
  while (n > 0 && nls_lds_bytes(true, n) + kStaticLds > kCuLds) --n;
  return n;
}

extern "C" int rl4co_tsp_nls(const rl4co_tsp_nls_args* args, void* stream) {
  RL4CO_REQUIRE(args != nullptr);
  const rl4co_tsp_nls_args& a = *args;
  RL4CO_REQUIRE(a.R >= 1);
  RL4CO_REQUIRE(a.n_instances >= 1);
  RL4CO_REQUIRE(a.R % a.n_instances == 0);
  RL4CO_REQUIRE(a.N >= 2 && a.N <= 1024);
  RL4CO_REQUIRE(a.T >= 1 && a.T <= 1024);
  RL4CO_REQUIRE(a.ls_max_iterations >= 0);
  RL4CO_REQUIRE(a.perturb_max_iterations >= 0);
  RL4CO_REQUIRE(a.n_perturbations >= 0);
  RL4CO_REQUIRE(a.n_perturbations <= (1 << 30) - 1);  // 1 + 2 * n_perturbations phases in an int32
  RL4CO_REQUIRE(a.locs != nullptr);
  RL4CO_REQUIRE(a.perturb_distances != nullptr);
  RL4CO_REQUIRE(a.actions != nullptr);
  RL4CO_REQUIRE(a.out_actions != nullptr);
  RL4CO_REQUIRE(a.out_reward != nullptr);
  RL4CO_REQUIRE(a.err != nullptr);
  hipStream_t s = rl4co::as_stream(stream);
  return a.N <= rl4co_tsp_nls_lds_nodes() ? launch<true>(a, s) : launch<false>(a, s);
}

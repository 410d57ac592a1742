// aco_tsp.hip — Ant System search on a heatmap (models/zoo/deepaco/antsystem.py) for TSP as one launch for gfx950.
//
// One workgroup of four waves per INSTANCE runs `iterations` Ant System iterations of that instance. Rows are ant-major
// (the reference's batchify): row j * B + b is ant j of instance b. The step, the update and the launch are ant_system.h's,
// shared with aco_cvrp.hip; this file keeps the LDS layout, the ant's state (the visited mask), its stores and stage R.
//   A  sample  L[i][n] = alpha * rl4co_logf(phe[i][n]) + beta * log_heu[i][n] (two multiplies, one add, each rounded once;
//              -ffp-contract=off), rebuilt from the current pheromone at the top of every iteration. One wave carries one
//              ant (wave w takes ants w, w + 4, ...): from start_nodes[row], N - 1 steps; a step reads row `cur` of L
//              (lane l owns nodes l, l + 64, ...: consecutive LDS words, no bank conflict), masks visited nodes to -inf (a
//              per-lane 16-bit register mask), divides by `temperature` when it is not 1, takes the log-softmax in the
//              project's order (max butterfly, lane-strided sum of rl4co_expf, butterfly, rl4co_logf) and selects the
//              argmax over feasible n of lp[n] - ln_noise[n], lowest node on equal keys (a NaN key counts as -inf).
//              ln_noise: the caller's fp32 [iterations, N - 1, rows, N] (parity mode), else
//              rl4co_logf(rl4co_exp1_noise(seed, philox_offset + it * N + t, row, n)). forced_actions: the given tours are
//              followed and only their log-probs computed.
//   R  reward  minus the closed tour length: tour_length.hip's arithmetic RESTATED in lds_tour_reward.h in the same order
//              (ATen's vector_norm over two elements, then SumKernel's 8-lane / 4-ILP / 4-level cascade; lanes 0..7 of the
//              ant's wave play the SIMD lanes) from the wave's tour in LDS; the expression text is kept equal to that file's
//              TourView::seg and lane_row_sum — change both together. Bit-equal to TSPEnv.get_reward (tested).
//   U  update  per instance over its ants, bit for bit the reference's _update_results / _reward_map / _update_pheromone:
//              M, m = max, min reward; best ant = lowest j with r_j == M; the first iteration or final_reward <= M replaces
//              final_reward / final_actions; v_j = (((r_j - m) / (M - m)) * same) * Q, NOT guarded against M == m (NaN, as
//              the reference); delta = 0, then for ants in ascending order each DIRECTED edge (a_t, a_t+1), t = 0 .. N - 2,
//              gets delta[from][to] += v_j (threads take one ant's edges in parallel: they are distinct for a permutation;
//              a workgroup barrier between ants keeps the ant order of every sum); delta[0][0] = 0;
//              phe = phe * decay + delta (multiply, round, add). The closing edge is not deposited and nothing is
//              symmetrised. delta is built in L's storage (L is rebuilt before it is read again).
// No barrier sits inside divergent control flow: the early exit below is decided from one LDS word.
//
// Range: a start node, a forced action or (UPDATE alone) an input action outside [0, N) raises RL4CO_EBIT_TOUR_INDEX and
// the instance is left untouched — the indices are only compared before anything is read or written through them.
// In-range input tours that are no permutations (forced / UPDATE alone) are served, their repeated edges in no stated order.
//
// LDS budget (bytes, all dynamic; the launcher checks that the compiler added no static LDS beyond kStaticLds):
//   scratch              256            (workgroup reductions, the bad-index flag)
//   wave tours           4 * 2 * 1024   (uint16_t, one tour per wave)
//   L and pheromone      8 N^2          (N <= rl4co_aco_tsp_lds_nodes(); above, both stay in global memory: `pheromone`
//                                        itself and the caller's `logits_scratch`, the same arithmetic)
//   static               <= 64
//   8 N^2 + 8192 + 256 + 64 <= 160 KiB  =>  N <= 139 (8 * 139^2 = 154 568): rl4co_aco_tsp_lds_nodes().
// Design estimates, NOT measured: at N = 100 a workgroup takes 88 448 B of LDS, so one workgroup (4 waves, one per SIMD)
// runs per CU; nothing about this kernel's occupancy has been profiled (tools/aco_bench.py records end-to-end time only).
#include <hip/hip_runtime.h>

#include "ant_system.h"
#include "lds_tour_reward.h"

namespace {

using namespace rl4co::aco;  // ant_system.h: the constants, check_indices, build_logits, ant_step, update_phase, launch
using rl4co::AntTour;        // lds_tour_reward.h: the reward of a tour held in LDS
using rl4co::ant_reward;

constexpr int kTourBytes = kWaves * 2 * kMaxNodes;

__host__ __device__ inline int64_t aco_lds_bytes(bool lds, int N) {
  return kScratchBytes + kTourBytes + (lds ? (int64_t)8 * N * N : 0);
}

// OPTS: the step with the decode options `o` (ant_system.h: ant_step<true>); false reads no `o` and is the kernel without them
template <bool LDS, bool OPTS>
__global__ void __launch_bounds__(kThreads) aco_tsp_kernel(const rl4co_aco_tsp_args a, const rl4co_heatmap_decode_opts o) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int b = blockIdx.x, B = a.B, N = a.N, A = a.n_ants;
  const int NN = N * N;
  const int64_t rows = (int64_t)A * B;
  const bool sample = (a.phases & RL4CO_ACO_SAMPLE) != 0, update = (a.phases & RL4CO_ACO_UPDATE) != 0;
  uint16_t* wtour = reinterpret_cast<uint16_t*>(smem + kScratchBytes) + w * kMaxNodes;
  float* gphe = a.pheromone + (int64_t)b * NN;
  float *Lm, *Pm;  // the logits / delta matrix and the pheromone of this instance
  if constexpr (LDS) {
    Lm = reinterpret_cast<float*>(smem + kScratchBytes + kTourBytes);
    Pm = Lm + NN;
  } else {
    Lm = a.logits_scratch + (int64_t)b * NN;
    Pm = gphe;
  }

  if (!check_indices(sample ? a.start_nodes : nullptr, 0, a.iterations, sample ? a.forced_actions : a.actions, N, A, B, b, N,
                     smem, a.err))
    return;  // (uniform: one LDS word)

  if constexpr (LDS) {
    for (int e = tid; e < NN; e += kThreads) Pm[e] = gphe[e];
    __syncthreads();
  }

  const unsigned long long seed = a.philox_seed ^ (a.philox_seed_dev ? *a.philox_seed_dev : 0ull);
  const float* heu = sample ? a.log_heuristic + (int64_t)b * NN : nullptr;
  const float2* xy = a.locs ? reinterpret_cast<const float2*>(a.locs) + (int64_t)b * N : nullptr;
  const int K = (N + 63) >> 6;  // nodes per lane
  uint32_t errbits = 0;
  bool have_best = a.has_best != 0;
  float best_r = have_best ? a.final_reward[b] : 0.0f;  // (uniform: every thread follows the same record)

  for (int it = 0; it < a.iterations; ++it) {
    if (sample) {
      // ---- A. the logits of this iteration ------------------------------------------------------------------------------
      build_logits(Lm, Pm, heu, NN, a.alpha, a.beta, tid);
      __syncthreads();

      for (int j = w; j < A; j += kWaves) {  // one wave, one ant
        const int64_t row = (int64_t)j * B + b;
        int cur = (int)a.start_nodes[(int64_t)it * rows + row];
        uint32_t vis = ((cur & 63) == lane) ? 1u << (cur >> 6) : 0u;  // bit k: node lane + 64 k is visited
        if (lane == 0) {
          wtour[0] = (uint16_t)cur;
          a.actions[row * N] = cur;
          if (a.logps) a.logps[row * N] = 0.0f;  // Sampling.pre_decoder_hook: the start node's log-prob is 0
        }
        if (a.all_logps)
          for (int n = lane; n < N; n += 64) a.all_logps[row * NN + n] = 0.0f;

        for (int t = 1; t < N; ++t) {
          const int forced = a.forced_actions ? (int)a.forced_actions[row * N + t] : -1;
          float* alp = a.all_logps ? a.all_logps + row * NN + (int64_t)t * N : nullptr;
          const float* lnz = a.ln_noise ? a.ln_noise + (((int64_t)it * (N - 1) + (t - 1)) * rows + row) * N : nullptr;
          float logp;
          const int chosen = ant_step<OPTS>(Lm + cur * N, N, K, lane, ~vis, a.temperature, forced, alp, lnz, seed,
                                            a.philox_offset + (uint64_t)it * N + t, (uint32_t)row, logp, errbits, &o);
          const uint32_t was = __shfl(vis, chosen & 63, 64);
          if ((was >> (chosen >> 6)) & 1u) errbits |= RL4CO_EBIT_INFEASIBLE;  // a forced node that was visited already
          if ((chosen & 63) == lane) vis |= 1u << (chosen >> 6);
          if (lane == 0) {
            wtour[t] = (uint16_t)chosen;
            a.actions[row * N + t] = chosen;
            if (a.logps) a.logps[row * N + t] = logp;
          }
          cur = chosen;
        }
        rl4co::lds_barrier_wave();  // the wave's tour is in LDS

        // ---- R. reward ---------------------------------------------------------------------------------------------------
        if (a.iter_actions)
          for (int t = lane; t < N; t += 64) a.iter_actions[((int64_t)it * rows + row) * N + t] = wtour[t];
        if (xy) {
          AntTour tv;
          tv.tour = wtour;
          tv.xy = xy;
          tv.n = N;
          const float rew = ant_reward(tv, lane);
          if (lane == 0) {
            a.reward[row] = rew;
            if (a.iter_reward) a.iter_reward[(int64_t)it * rows + row] = rew;
          }
        }
        rl4co::lds_barrier_wave();  // before the wave's next ant rewrites the tour
      }
      __syncthreads();  // every ant's tour and reward of this instance is in global memory
    }

    if (update)  // ---- U. best tour, reward map, pheromone; every edge deposited, then delta[0][0] = 0 -------------------
      update_phase<false>(a.actions, N, a.reward, a.final_reward, a.final_actions, a.final_reward_cache, nullptr, 0, Lm, Pm, N, A,
                          B, b, it, a.decay, a.Q, have_best, best_r, smem);
  }

  if constexpr (LDS) {
    if (update)
      for (int e = tid; e < NN; e += kThreads) gphe[e] = Pm[e];
  }
  if (errbits) atomicOr(a.err, (int)errbits);
}

}  // namespace

extern "C" int rl4co_aco_tsp_lds_nodes(void) { return lds_nodes(aco_lds_bytes); }

extern "C" int rl4co_aco_tsp(const rl4co_aco_tsp_args* args, void* stream) {
  const rl4co_heatmap_decode_opts off = {};
  return rl4co_aco_tsp_opts(args, &off, stream);
}

extern "C" int rl4co_aco_tsp_opts(const rl4co_aco_tsp_args* args, const rl4co_heatmap_decode_opts* opts, void* stream) {
  RL4CO_REQUIRE(args != nullptr);
  const rl4co_aco_tsp_args& a = *args;
  if (const int rc = require_common(a)) return rc;
  if (const int rc = require_decode_opts(opts, a.ln_noise)) return rc;
  const rl4co_heatmap_decode_opts& o = *opts;
  const bool sample = (a.phases & RL4CO_ACO_SAMPLE) != 0;
  RL4CO_REQUIRE(!sample || (a.log_heuristic != nullptr && a.start_nodes != nullptr));
  const bool lds = a.N <= rl4co_aco_tsp_lds_nodes();
  RL4CO_REQUIRE(lds || a.logits_scratch != nullptr);  // above the LDS tier L / delta live in the caller's [B,N,N] scratch
  hipStream_t s = rl4co::as_stream(stream);
  const int bytes = (int)aco_lds_bytes(lds, a.N);
  if (decode_opts_on(o))
    return lds ? launch<aco_tsp_kernel<true, true>>(a, bytes, s, 0, o) : launch<aco_tsp_kernel<false, true>>(a, bytes, s, 0, o);
  return lds ? launch<aco_tsp_kernel<true, false>>(a, bytes, s, 0, o) : launch<aco_tsp_kernel<false, false>>(a, bytes, s, 0, o);
}

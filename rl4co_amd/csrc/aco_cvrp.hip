// aco_cvrp.hip — Ant System search on a heatmap (models/zoo/deepaco/antsystem.py) for CVRP as one launch for gfx950.
//
// aco_tsp.hip's layout with CVRP's transition rule inside the step: one workgroup of four waves per INSTANCE runs
// `iterations` Ant System iterations of that instance; rows are ant-major (row j * B + b is ant j of instance b). The step,
// the update and the launch are ant_system.h's, shared with aco_tsp.hip; this file keeps the LDS layout, the ant's state
// (visited mask, load, feasible set), its stores and stage R.
// N is the heatmap side (the depot is node 0), C = N - 1 the customers, W = max(C + 1, 2 C - 1) the longest action row the
// reference can produce (a row takes C + max(k, 1) actions, k <= C - 1 its mid-tour depot returns).
//   A  sample  L[i][n] = alpha * rl4co_logf(phe[i][n]) + beta * log_heu[i][n] (each operation rounded once), rebuilt at the
//              top of every iteration. One wave carries one ant (wave w takes ants w, w + 4, ...). The ant's state is
//              cvrp/env.py:66-136 in fp32 in env_step.hip's order (cvrp_step_body): used = (used + demand[clamp(a - 1)]) *
//              (a != 0 ? 1 : 0); customer c is infeasible when visited or demand[c - 1] + used > cap + 1e-5f (the right side
//              ONE fp32 add); the depot is infeasible when cur == 0 and some customer is feasible; done = every customer
//              visited and action 0 taken at least once; the reset state does not mark the depot. The visited set is a
//              per-lane 16-bit register mask (lane l owns nodes l, l + 64, ...), the demands sit in LDS, used / cur / the
//              depot flag are wave-uniform. Entry: start_nodes == nullptr (multisample) starts every ant at the depot and
//              samples the first action from row 0; with start_nodes (multistart) the start is action 0 with log-prob 0
//              and is stepped through the state (Sampling.pre_decoder_hook). A step is aco_tsp.hip's: row `cur` of L,
//              infeasible nodes to -inf, divided by `temperature` when it is not 1, log-softmax (max butterfly, lane-strided
//              rl4co_expf sum, butterfly, rl4co_logf), key = lp - ln_noise, lowest-index argmax (a NaN key counts as -inf).
//              ln_noise: the caller's fp32 [iterations, W, rows, N] (parity mode; step t reads [it, t, row]), else
//              rl4co_logf(rl4co_exp1_noise(seed, philox_offset + it * W + t, row, n)). forced_actions [rows, W]: the given
//              rows are followed and only their log-probs computed. An ant stops at done; its row is zero-filled after its
//              length (log-probs 0 there, what the reference's one-feasible-node softmax gives), lengths[row] counts the
//              actions up to and including the one that made it done. The step loop is bounded by W: a row not done after W
//              actions (possible only if a demand exceeds the capacity) raises RL4CO_EBIT_INFEASIBLE and ends.
//   R  reward  minus the closed length of [depot, actions[0 .. W-1]] AT THE FIXED WIDTH W: tour_length.hip's arithmetic with
//              prepend_depot, through its restatement in lds_tour_reward.h with n = W + 1 (ATen's vector_norm over two
//              elements, then SumKernel's 8-lane / 4-ILP / 4-level cascade over W + 1 segments; two texts remain,
//              tour_length.hip and lds_tour_reward.h — change both together). Bit-equal to CVRPEnv.get_reward on the W-wide
//              zero-padded row.
//              CONVENTION: the reference trims every iteration's rows to the longest row of the whole batch before it sums,
//              so the last bits of its reward depend on the other instances; a per-instance workgroup cannot know that
//              width and does not try. Trailing depot segments have length exactly 0: only the summation order differs.
//   U  update  aco_tsp.hip's, bit for bit the reference's _update_results / _reward_map / _update_pheromone over the
//              whole padded row: M, m = max, min reward; best ant = lowest j with r_j == M; the first iteration or
//              final_reward <= M replaces final_reward / final_actions and writes final_iteration[b] = iteration_base + it;
//              v_j NOT guarded against M == m; for ants in ascending order each directed edge (a_t, a_t+1), t = 0 .. T - 2,
//              gets delta[from][to] += v_j, EXCEPT (0, 0) edges, which are skipped: the reference zeroes delta[0][0]
//              afterwards, so skipping gives the same matrix without a race on that word. Every other edge of a sampled
//              ant is distinct (each customer is entered once and left once), so one ant's edges go in parallel with a
//              workgroup barrier between ants. phe = phe * decay + delta. (depot, first action) is never deposited; the
//              closing edge (last customer, 0) only where a trailing 0 is in the row. At the fixed width W that is every
//              sampled row shorter than W; the reference, trimming to the batch's longest row, leaves it out for the rows
//              that are the longest of their batch and end at a customer — the same batch dependence as in R, and UPDATE
//              alone on rows trimmed the reference's way reproduces the reference bit for bit (tested against its
//              records). UPDATE alone takes rows of any width T >= 2.
// No barrier sits inside divergent control flow: the early exit below is decided from one LDS word.
//
// Range: a start node outside [1, N), a forced action or (UPDATE alone) an input action outside [0, N) raises
// RL4CO_EBIT_TOUR_INDEX and the instance is left untouched — the indices are only compared before anything is read or
// written through them. In-range input rows with repeated edges (forced / UPDATE alone) are served in no stated order.
//
// LDS budget (bytes, all dynamic; the launcher checks that the compiler added no static LDS beyond kStaticLds):
//   scratch              256                        (workgroup reductions, the bad-index flag)
//   demands              4 * roundup(N, 4)          (float; word c is demand[c - 1], word 0 the clamp's demand[0])
//   wave tours           4 * 2 * roundup(W + 1, 8)  (uint16_t, [depot, actions] per wave)
//   L and pheromone      8 N^2                      (N <= rl4co_aco_cvrp_lds_nodes(); above, both stay in global memory:
//                                                    `pheromone` itself and the caller's `logits_scratch`)
//   static               <= 64
//   8 N^2 + 8 roundup(W + 1, 8) + 4 roundup(N, 4) + 256 + 64 <= 160 KiB  =>  N <= 141
//   (N = 141: 159 048 + 2 240 + 576 + 320 = 162 184; N = 142: 161 312 + 2 304 + 576 + 320 = 164 512 > 163 840).
// Design estimates, NOT measured: at N = 101 (CVRP-100) a workgroup takes 83 880 B of LDS, so one workgroup (4 waves, one
// per SIMD) runs per CU; nothing about this kernel's occupancy has been profiled (tools/aco_bench.py --env cvrp records
// end-to-end time only).
#include <hip/hip_runtime.h>

#include "ant_rules.h"
#include "ant_system.h"
#include "lds_tour_reward.h"

namespace {

using namespace rl4co::aco;  // ant_system.h: the constants, check_indices, build_logits, ant_step, update_phase, launch;
                             // ant_rules.h: the capacity test and the load (shared with aco_depot_grad.hip)
using rl4co::AntTour;        // lds_tour_reward.h: the reward of a tour held in LDS
using rl4co::ant_reward;

__host__ __device__ inline int cvrp_width(int N) {  // W
  const int C = N - 1;
  return C + 1 > 2 * C - 1 ? C + 1 : 2 * C - 1;
}
__host__ __device__ inline int demand_bytes(int N) { return 4 * ((N + 3) & ~3); }
__host__ __device__ inline int tour_stride(int N) { return (cvrp_width(N) + 1 + 7) & ~7; }  // uint16_t per wave
__host__ __device__ inline int64_t aco_lds_bytes(bool lds, int N) {
  return kScratchBytes + demand_bytes(N) + kWaves * 2 * tour_stride(N) + (lds ? (int64_t)8 * N * N : 0);
}

// OPTS: the step with the decode options `o` (ant_system.h: ant_step<true>); false reads no `o` and is the kernel without them
template <bool LDS, bool OPTS>
__global__ void __launch_bounds__(kThreads) aco_cvrp_kernel(const rl4co_aco_cvrp_args a, const rl4co_heatmap_decode_opts o) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int b = blockIdx.x, B = a.B, N = a.N, A = a.n_ants;
  const int C = N - 1, W = cvrp_width(N), NN = N * N;
  const int64_t rows = (int64_t)A * B;
  const bool sample = (a.phases & RL4CO_ACO_SAMPLE) != 0, update = (a.phases & RL4CO_ACO_UPDATE) != 0;
  const int T = sample ? W : a.T;  // the width of `actions` and `final_actions`
  float* dnode = reinterpret_cast<float*>(smem + kScratchBytes);  // [N]: word c is demand[c - 1], word 0 demand[0]
  uint16_t* wtour = reinterpret_cast<uint16_t*>(smem + kScratchBytes + demand_bytes(N)) + w * tour_stride(N);
  float* gphe = a.pheromone + (int64_t)b * NN;
  float *Lm, *Pm;  // the logits / delta matrix and the pheromone of this instance
  if constexpr (LDS) {
    Lm = reinterpret_cast<float*>(smem + kScratchBytes + demand_bytes(N) + kWaves * 2 * tour_stride(N));
    Pm = Lm + NN;
  } else {
    Lm = a.logits_scratch + (int64_t)b * NN;
    Pm = gphe;
  }

  // a start is a customer: the lower bound is 1
  if (!check_indices(sample ? a.start_nodes : nullptr, 1, a.iterations, sample ? a.forced_actions : a.actions, T, A, B, b, N,
                     smem, a.err))
    return;  // (uniform: one LDS word)

  if constexpr (LDS) {
    for (int e = tid; e < NN; e += kThreads) Pm[e] = gphe[e];
  }
  if (sample) {
    const float* dem = a.demand + (int64_t)b * C;
    for (int c = tid; c < N; c += kThreads) dnode[c] = dem[c > 0 ? c - 1 : 0];  // clamp(a - 1, 0, C - 1)
  }
  __syncthreads();

  const unsigned long long seed = a.philox_seed ^ (a.philox_seed_dev ? *a.philox_seed_dev : 0ull);
  const float* heu = sample ? a.log_heuristic + (int64_t)b * NN : nullptr;
  const float2* xy = a.locs ? reinterpret_cast<const float2*>(a.locs) + (int64_t)b * N : nullptr;
  const int K = (N + 63) >> 6;  // nodes per lane
  const float thr = sample ? cvrp_threshold(a.vehicle_capacity[b]) : 0.0f;  // cvrp/env.py:129, one fp32 add
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
        // the reset state (cvrp/env.py:98-124): at the depot, nothing visited — not the depot either
        int cur = 0, left = C, t = 0;
        uint32_t vis = 0u;  // bit k: node lane + 64 k is visited
        float used = 0.0f;
        bool depot_seen = false;
        if (lane == 0) wtour[0] = 0;  // the prepended depot of the reward
        if (a.start_nodes) {  // multistart: action 0 is given, log-prob 0, stepped through the state
          cur = __builtin_amdgcn_readfirstlane((int)a.start_nodes[(int64_t)it * rows + row]);
          used = cvrp_advance(used, dnode[cur], 1);  // (a start is a customer: check_indices' lower bound)
          if ((cur & 63) == lane) vis |= 1u << (cur >> 6);
          left = C - 1;
          if (lane == 0) {
            wtour[1] = (uint16_t)cur;
            a.actions[row * W] = cur;
            if (a.logps) a.logps[row * W] = 0.0f;
          }
          if (a.all_logps)
            for (int n = lane; n < N; n += 64) a.all_logps[row * W * N + n] = 0.0f;
          t = 1;
        }
        bool done = false;  // (C >= 1 and the depot is unseen)

        for (; t < W && !done; ++t) {  // bounded by W whatever the data
          // cvrp/env.py:126-136: the feasible set of this step
          uint32_t feas = 0u;
          for (int k = 0; k < K; ++k) {
            const int n = lane + 64 * k;
            if (n >= 1 && n < N && !((vis >> k) & 1u) && cvrp_fits(dnode[n], used, thr)) feas |= 1u << k;
          }
          const bool any_customer = __any(feas != 0u);
          if (lane == 0 && cvrp_depot_ok(cur, any_customer)) feas |= 1u;

          const int forced = a.forced_actions ? (int)a.forced_actions[row * W + t] : -1;
          float* alp = a.all_logps ? a.all_logps + (row * W + t) * N : nullptr;
          const float* lnz = a.ln_noise ? a.ln_noise + (((int64_t)it * W + t) * rows + row) * N : nullptr;
          float logp;
          const int chosen = ant_step<OPTS>(Lm + cur * N, N, K, lane, feas, a.temperature, forced, alp, lnz, seed,
                                            a.philox_offset + (uint64_t)it * W + t, (uint32_t)row, logp, errbits, &o);
          const uint32_t could = __shfl(feas, chosen & 63, 64);
          const uint32_t was = __shfl(vis, chosen & 63, 64);
          if (!((could >> (chosen >> 6)) & 1u)) errbits |= RL4CO_EBIT_INFEASIBLE;  // a forced node that is infeasible
          // cvrp/env.py:66-96 (cvrp_step_body's order)
          used = cvrp_advance(used, dnode[chosen], chosen);
          if (chosen == 0) {
            depot_seen = true;
          } else {
            if (!((was >> (chosen >> 6)) & 1u)) --left;
            if ((chosen & 63) == lane) vis |= 1u << (chosen >> 6);
          }
          if (lane == 0) {
            wtour[1 + t] = (uint16_t)chosen;
            a.actions[row * W + t] = chosen;
            if (a.logps) a.logps[row * W + t] = logp;
          }
          cur = chosen;
          done = left == 0 && depot_seen;
        }
        if (!done) errbits |= RL4CO_EBIT_INFEASIBLE;  // W actions and not done: some demand exceeds the capacity
        const int len = t;
        for (int tt = len + lane; tt < W; tt += 64) {  // the reference's trailing depot visits, log-prob 0
          wtour[1 + tt] = 0;
          a.actions[row * W + tt] = 0;
          if (a.logps) a.logps[row * W + tt] = 0.0f;
        }
        if (a.all_logps)
          for (int64_t e = (int64_t)len * N + lane; e < (int64_t)W * N; e += 64) a.all_logps[row * W * N + e] = 0.0f;
        if (lane == 0) {
          a.lengths[row] = len;
          if (a.iter_lengths) a.iter_lengths[(int64_t)it * rows + row] = len;
        }
        rl4co::lds_barrier_wave();  // the wave's tour is in LDS

        // ---- R. reward ---------------------------------------------------------------------------------------------------
        if (a.iter_actions)
          for (int tt = lane; tt < W; tt += 64) a.iter_actions[((int64_t)it * rows + row) * W + tt] = wtour[1 + tt];
        if (xy) {
          AntTour tv;
          tv.tour = wtour;
          tv.xy = xy;
          tv.n = W + 1;
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

    if (update)  // ---- U. best tour, reward map, pheromone; (0, 0) edges skipped, nothing zeroed afterwards ---------------
      update_phase<true>(a.actions, T, a.reward, a.final_reward, a.final_actions, a.final_reward_cache, a.final_iteration,
                         a.iteration_base, Lm, Pm, N, A, B, b, it, a.decay, a.Q, have_best, best_r, smem);
  }

  if constexpr (LDS) {
    if (update)
      for (int e = tid; e < NN; e += kThreads) gphe[e] = Pm[e];
  }
  if (errbits) atomicOr(a.err, (int)errbits);
}

}  // namespace

extern "C" int rl4co_aco_cvrp_lds_nodes(void) { return lds_nodes(aco_lds_bytes); }

extern "C" int rl4co_aco_cvrp(const rl4co_aco_cvrp_args* args, void* stream) {
  const rl4co_heatmap_decode_opts off = {};
  return rl4co_aco_cvrp_opts(args, &off, stream);
}

extern "C" int rl4co_aco_cvrp_opts(const rl4co_aco_cvrp_args* args, const rl4co_heatmap_decode_opts* opts, void* stream) {
  RL4CO_REQUIRE(args != nullptr);
  const rl4co_aco_cvrp_args& a = *args;
  if (const int rc = require_common(a)) return rc;
  if (const int rc = require_decode_opts(opts, a.ln_noise)) return rc;
  const rl4co_heatmap_decode_opts& o = *opts;
  const bool sample = (a.phases & RL4CO_ACO_SAMPLE) != 0;
  RL4CO_REQUIRE(sample ? a.T == cvrp_width(a.N) : a.T >= 2);  // sampled rows are W wide; UPDATE alone takes any width
  RL4CO_REQUIRE(!sample || (a.log_heuristic != nullptr && a.demand != nullptr && a.vehicle_capacity != nullptr));
  RL4CO_REQUIRE(!sample || a.lengths != nullptr);
  const bool lds = a.N <= rl4co_aco_cvrp_lds_nodes();
  RL4CO_REQUIRE(lds || a.logits_scratch != nullptr);  // above the LDS tier L / delta live in the caller's [B,N,N] scratch
  hipStream_t s = rl4co::as_stream(stream);
  const int bytes = (int)aco_lds_bytes(lds, a.N);
  if (decode_opts_on(o))
    return lds ? launch<aco_cvrp_kernel<true, true>>(a, bytes, s, 0, o) : launch<aco_cvrp_kernel<false, true>>(a, bytes, s, 0, o);
  return lds ? launch<aco_cvrp_kernel<true, false>>(a, bytes, s, 0, o) : launch<aco_cvrp_kernel<false, false>>(a, bytes, s, 0, o);
}

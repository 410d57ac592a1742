// aco_prize.hip — Ant System search on a heatmap (models/zoo/deepaco/antsystem.py) for the prize problems, OP and PCTSP, as
// one launch for gfx950: one templated kernel, one instantiation per environment.
//
// aco_cvrp.hip's layout with the prize problems' transition rules inside the step: one workgroup of kWaves waves per
// INSTANCE runs `iterations` Ant System iterations of that instance (a workgroup takes instances b, b + n_workgroups, ...
// one after the other; the results do not depend on n_workgroups); rows are ant-major (row j * B + b is ant j of instance
// b). The step, the update and the launch are ant_system.h's, shared with aco_tsp.hip and aco_cvrp.hip; the sums of stage R
// are lds_tour_reward.h's; this file keeps the LDS layout, the ant's state and mask per environment, its stores and stage R.
// N is the heatmap side (the depot is node 0), C = N - 1 the customers, W = N the longest action row the reference can
// produce: at most C customers, then the depot.
//   A  sample  L[i][n] = alpha * rl4co_logf(phe[i][n]) + beta * log_heu[i][n] (each operation rounded once), rebuilt at the
//              top of every iteration. One wave carries one ant (wave w takes ants w, w + kWaves, ...). Every ant starts at
//              the depot with nothing visited (the depot neither) and samples its first action from row 0. The visited set
//              is a per-lane 16-bit register mask (lane l owns nodes l, l + 64, ...), the per-node vectors sit in LDS, the
//              rest of the state is wave-uniform. A distance is d(i, j) = sqrtf(fmaf(dy, dy, dx * dx)) with dx = x_j - x_i,
//              dy = y_j - y_i: env_step.hip's op_dist, torch's norm over a dim of two.
//              OP (op/env.py:67-154, env_step.hip's op_step_body): state cur, visited, tour_length, t. Customer j is
//              infeasible when visited, when the depot has been visited, or when tour_length + d(cur, j) > max_length[j]
//              (one fp32 add; max_length is the environment's per-node table); the depot is always feasible. A step is
//              tour_length = tour_length + d(cur, a), visited[a] = 1, done = (a == 0 && t > 0): a row may take the depot
//              at step 0 and again at step 1.
//              PCTSP (pctsp/env.py:62-144, pctsp_step_body): state cur, visited, cur_total_prize, t. Customer j is
//              infeasible when visited or when the depot has been visited; the depot is infeasible while
//              cur_total_prize < 1.0f and an unvisited customer remains. A step is cur_total_prize = cur_total_prize +
//              prize[a], visited[a] = 1, done = (t > 0 && a == 0).
//              A step is aco_tsp.hip's: row `cur` of L, infeasible nodes to -inf, divided by `temperature` when it is not 1,
//              log-softmax, key = lp - ln_noise, lowest-index argmax. ln_noise: the caller's fp32 [iterations, W, rows, N]
//              (parity mode; step t reads [it, t, row]), else rl4co_logf(rl4co_exp1_noise(seed, philox_offset + it * W + t,
//              row, n)). forced_actions [rows, W]: the given rows are followed and only their log-probs computed. An ant
//              stops at done; its row is zero-filled after its length (log-probs 0 there, what the reference's
//              one-feasible-node softmax gives), lengths[row] counts the actions up to and including the one that made it
//              done. The step loop is bounded by W: a sampled row is done within W actions whatever the data (each customer
//              at most once, then only the depot is left); a forced row that is not raises RL4CO_EBIT_INFEASIBLE.
//   R  reward  AT THE FIXED WIDTH W, every sum in ONE order: lds_tour_reward.h's ant_reward over n terms, which is ATen's
//              row sum (n < 8: four accumulators over the groups of four, the rest into the first, then 0 + 1 + 2 + 3;
//              else 8 lanes over the vectors of eight, each lane 4 accumulators with the 4-level cascade, the tail into the
//              running total first, then the lanes in ascending order).
//              OP: the W terms prize[a_t] (the depot's prize is 0): OPEnv.get_reward on the W-wide row.
//              PCTSP: S - (len + P), S over the W terms penalty[a_t], len over the W + 1 segments of [depot, a_0 .. a_{W-1}]
//              closed (aco_cvrp.hip's R), P over the C terms penalty[1 .. C]; P is computed once per instance.
//              PCTSPEnv.get_reward on the W-wide row.
//              CONVENTION (as aco_cvrp.hip): the reference trims every iteration's rows to the longest row of the whole
//              batch before it sums; the trailing terms are exactly 0, only the association differs (measured in
//              tests/aco_prize_ref.py).
//   U  update  aco_cvrp.hip's (update_phase<true>): (0, 0) edges are skipped, every other edge of a sampled ant is
//              distinct. UPDATE alone takes rows of any width T >= 2.
// No barrier sits inside divergent control flow: the skip of an instance below is decided from one LDS word, and every
// instance begins with a workgroup barrier (the word and the LDS matrices of the last instance are done with).
//
// Range: a forced action or (UPDATE alone) an input action outside [0, N) raises RL4CO_EBIT_TOUR_INDEX and the instance is
// left untouched — the indices are only compared before anything is read or written through them.
//
// LDS budget (bytes, all dynamic; the launcher checks that the compiler added no static LDS beyond kStaticLds):
//   scratch              256                        (workgroup reductions, the bad-index flag, PCTSP's P)
//   per-node vectors     4 * V * roundup(N, 4)      (float; OP V = 3: x, y, max_length; PCTSP V = 2: prize, penalty)
//   wave tours           4 * 2 * roundup(W + 1, 8)  (uint16_t, [depot, actions] per wave)
//   L and pheromone      8 N^2                      (N <= rl4co_aco_prize_lds_nodes(env); above, both stay in global memory:
//                                                    `pheromone` itself and the caller's `logits_scratch`)
//   static               <= 64
//   8 N^2 + 8 roundup(W + 1, 8) + 4 V roundup(N, 4) + 256 + 64 <= 160 KiB  =>  N <= 141 for OP and for PCTSP
//   (OP N = 141: 159 048 + 1 152 + 1 728 + 320 = 162 248; N = 142: 161 312 + 1 152 + 1 728 + 320 = 164 512 > 163 840;
//    PCTSP N = 141: 159 048 + 1 152 + 1 152 + 320 = 161 672; N = 142: 161 312 + 1 152 + 1 152 + 320 = 163 936 > 163 840).
// Design estimate, NOT measured: at N = 51 a workgroup takes about 22 KiB of LDS; nothing about this kernel's occupancy has
// been profiled (tools/aco_bench.py --env prize records end-to-end time only).
#include <hip/hip_runtime.h>

#include "ant_rules.h"
#include "ant_system.h"
#include "lds_tour_reward.h"

namespace {

using namespace rl4co::aco;  // ant_system.h: the constants, check_indices, build_logits, ant_step, update_phase, launch;
                             // ant_rules.h: the budget and prize tests (shared with aco_depot_grad.hip)
using rl4co::AntTour;        // lds_tour_reward.h: the sums of stage R
using rl4co::ant_reward;

__host__ __device__ inline int node_vectors(int env) { return env == RL4CO_ENV_OP ? 3 : 2; }  // V
__host__ __device__ inline int node_stride(int N) { return (N + 3) & ~3; }                    // floats per vector
__host__ __device__ inline int node_bytes(int env, int N) { return 4 * node_vectors(env) * node_stride(N); }
__host__ __device__ inline int tour_stride(int N) { return (N + 1 + 7) & ~7; }  // uint16_t per wave (W = N)
__host__ __device__ inline int64_t aco_lds_bytes(int env, bool lds, int N) {
  return kScratchBytes + node_bytes(env, N) + kWaves * 2 * tour_stride(N) + (lds ? (int64_t)8 * N * N : 0);
}
__device__ inline float* penalty_total(unsigned char* smem) { return reinterpret_cast<float*>(smem + 56); }  // PCTSP's P

// the terms vec[row[t]], t = 0 .. n - 1, of a row held in LDS
struct RowTerms {
  const uint16_t* row;
  const float* vec;
  int n;
  __device__ inline float seg(int t) const { return vec[row[t]]; }
};
// the terms vec[t], t = 0 .. n - 1
struct VecTerms {
  const float* vec;
  int n;
  __device__ inline float seg(int t) const { return vec[t]; }
};

// OPTS: the step with the decode options `o` (ant_system.h: ant_step<true>); false reads no `o` and is the kernel without them
template <int ENV, bool LDS, bool OPTS>
__global__ void __launch_bounds__(kThreads) aco_prize_kernel(const rl4co_aco_prize_args a, const rl4co_heatmap_decode_opts o) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr bool kOp = ENV == RL4CO_ENV_OP;

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int B = a.B, N = a.N, A = a.n_ants;
  const int C = N - 1, W = N, NN = N * N, NS = node_stride(N);
  const int64_t rows = (int64_t)A * B;
  const bool sample = (a.phases & RL4CO_ACO_SAMPLE) != 0, update = (a.phases & RL4CO_ACO_UPDATE) != 0;
  const int T = sample ? W : a.T;  // the width of `actions` and `final_actions`
  float* v0 = reinterpret_cast<float*>(smem + kScratchBytes);  // OP: x          PCTSP: prize
  float* v1 = v0 + NS;                                         // OP: y          PCTSP: penalty
  float* v2 = v1 + NS;                                         // OP: max_length
  uint16_t* wtour = reinterpret_cast<uint16_t*>(smem + kScratchBytes + node_bytes(ENV, N)) + w * tour_stride(N);
  const unsigned long long seed = a.philox_seed ^ (a.philox_seed_dev ? *a.philox_seed_dev : 0ull);
  const int K = (N + 63) >> 6;  // nodes per lane
  uint32_t errbits = 0;

  for (int b = blockIdx.x; b < B; b += gridDim.x) {
    __syncthreads();  // the last instance's scratch words and LDS matrices are done with
    float* gphe = a.pheromone + (int64_t)b * NN;
    float *Lm, *Pm;  // the logits / delta matrix and the pheromone of this instance
    if constexpr (LDS) {
      Lm = reinterpret_cast<float*>(smem + kScratchBytes + node_bytes(ENV, N) + kWaves * 2 * tour_stride(N));
      Pm = Lm + NN;
    } else {
      Lm = a.logits_scratch + (int64_t)b * NN;
      Pm = gphe;
    }

    if (!check_indices(nullptr, 0, a.iterations, sample ? a.forced_actions : a.actions, T, A, B, b, N, smem, a.err))
      continue;  // (uniform: one LDS word)

    if constexpr (LDS) {
      for (int e = tid; e < NN; e += kThreads) Pm[e] = gphe[e];
    }
    const float2* xy = sample ? reinterpret_cast<const float2*>(a.locs) + (int64_t)b * N : nullptr;
    const float* gprize = sample ? a.prize + (int64_t)b * N : nullptr;
    if (sample) {
      for (int n = tid; n < N; n += kThreads) {
        if constexpr (kOp) {
          const float2 p = xy[n];
          v0[n] = p.x;
          v1[n] = p.y;
          v2[n] = a.max_length[(int64_t)b * N + n];
        } else {
          v0[n] = gprize[n];
          v1[n] = a.penalty[(int64_t)b * N + n];
        }
      }
    }
    __syncthreads();
    if constexpr (!kOp) {
      if (sample) {  // P: the penalties of all customers, once per instance
        if (w == 0) {
          VecTerms all;
          all.vec = v1 + 1;
          all.n = C;
          const float total = -ant_reward(all, lane);
          if (lane == 0) *penalty_total(smem) = total;
        }
        __syncthreads();
      }
    }

    const float* heu = sample ? a.log_heuristic + (int64_t)b * NN : nullptr;
    bool have_best = a.has_best != 0;
    float best_r = have_best ? a.final_reward[b] : 0.0f;  // (uniform: every thread follows the same record)

    for (int it = 0; it < a.iterations; ++it) {
      if (sample) {
        // ---- A. the logits of this iteration ----------------------------------------------------------------------------
        build_logits(Lm, Pm, heu, NN, a.alpha, a.beta, tid);
        __syncthreads();

        for (int j = w; j < A; j += kWaves) {  // one wave, one ant
          const int64_t row = (int64_t)j * B + b;
          // the reset state: at the depot, nothing visited — not the depot either
          int cur = 0, left = C, t = 0;
          uint32_t vis = 0u;     // bit k: node lane + 64 k is visited
          float acc = 0.0f;      // OP: tour_length; PCTSP: cur_total_prize
          bool depot_seen = false;
          if (lane == 0) wtour[0] = 0;  // the prepended depot of the length
          bool done = false;

          for (; t < W && !done; ++t) {  // bounded by W whatever the data
            uint32_t feas = 0u;
            if constexpr (kOp) {  // op/env.py:137-154
              const float cx = v0[cur], cy = v1[cur];
              for (int k = 0; k < K; ++k) {
                const int n = lane + 64 * k;
                if (n >= 1 && n < N && !((vis >> k) & 1u) && !depot_seen) {
                  const float reach = op_advance(acc, op_dist(cx, cy, v0[n], v1[n]));
                  if (op_within(reach, v2[n])) feas |= 1u << k;
                }
              }
              if (lane == 0) feas |= 1u;
            } else {  // pctsp/env.py:137-144
              for (int k = 0; k < K; ++k) {
                const int n = lane + 64 * k;
                if (n >= 1 && n < N && !((vis >> k) & 1u) && !depot_seen) feas |= 1u << k;
              }
              if (lane == 0 && pctsp_depot_ok(acc, left)) feas |= 1u;
            }

            const int forced = a.forced_actions ? (int)a.forced_actions[row * W + t] : -1;
            float* alp = a.all_logps ? a.all_logps + (row * W + t) * N : nullptr;
            const float* lnz = a.ln_noise ? a.ln_noise + (((int64_t)it * W + t) * rows + row) * N : nullptr;
            float logp;
            const int chosen = ant_step<OPTS>(Lm + cur * N, N, K, lane, feas, a.temperature, forced, alp, lnz, seed,
                                              a.philox_offset + (uint64_t)it * W + t, (uint32_t)row, logp, errbits, &o);
            const uint32_t could = __shfl(feas, chosen & 63, 64);
            const uint32_t was = __shfl(vis, chosen & 63, 64);
            if (!((could >> (chosen >> 6)) & 1u)) errbits |= RL4CO_EBIT_INFEASIBLE;  // a forced node that is infeasible
            if constexpr (kOp) {  // op/env.py:67-98
              acc = op_advance(acc, op_dist(v0[cur], v1[cur], v0[chosen], v1[chosen]));
            } else {  // pctsp/env.py:62-91
              acc = pctsp_advance(acc, v0[chosen]);
            }
            if (chosen == 0) {
              depot_seen = true;
            } else if (!((was >> (chosen >> 6)) & 1u)) {
              --left;
            }
            if ((chosen & 63) == lane) vis |= 1u << (chosen >> 6);
            if (lane == 0) {
              wtour[1 + t] = (uint16_t)chosen;
              a.actions[row * W + t] = chosen;
              if (a.logps) a.logps[row * W + t] = logp;
            }
            cur = chosen;
            done = chosen == 0 && t > 0;
          }
          if (!done) errbits |= RL4CO_EBIT_INFEASIBLE;  // W actions and not done: forced rows only
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

          // ---- R. reward -------------------------------------------------------------------------------------------------
          if (a.iter_actions)
            for (int tt = lane; tt < W; tt += 64) a.iter_actions[((int64_t)it * rows + row) * W + tt] = wtour[1 + tt];
          RowTerms gathered;
          gathered.row = wtour + 1;
          gathered.vec = kOp ? gprize : v1;  // OP: the prizes (global); PCTSP: the penalties (LDS)
          gathered.n = W;
          float rew = -ant_reward(gathered, lane);
          if constexpr (!kOp) {
            AntTour tv;
            tv.tour = wtour;
            tv.xy = xy;
            tv.n = W + 1;
            const float length = -ant_reward(tv, lane);
            const float cost = length + *penalty_total(smem);
            rew = rew - cost;
          }
          if (lane == 0) {
            a.reward[row] = rew;
            if (a.iter_reward) a.iter_reward[(int64_t)it * rows + row] = rew;
          }
          rl4co::lds_barrier_wave();  // before the wave's next ant rewrites the tour
        }
        __syncthreads();  // every ant's row and reward of this instance is in global memory
      }

      if (update)  // ---- U. best row, reward map, pheromone; (0, 0) edges skipped, nothing zeroed afterwards ---------------
        update_phase<true>(a.actions, T, a.reward, a.final_reward, a.final_actions, a.final_reward_cache, a.final_iteration,
                           a.iteration_base, Lm, Pm, N, A, B, b, it, a.decay, a.Q, have_best, best_r, smem);
    }

    if constexpr (LDS) {
      if (update)
        for (int e = tid; e < NN; e += kThreads) gphe[e] = Pm[e];
    }
  }
  if (errbits) atomicOr(a.err, (int)errbits);
}

template <int ENV>
int launch_env(const rl4co_aco_prize_args& a, const rl4co_heatmap_decode_opts& o, hipStream_t s) {
  const bool lds = a.N <= rl4co_aco_prize_lds_nodes(ENV);
  RL4CO_REQUIRE(lds || a.logits_scratch != nullptr);  // above the LDS tier L / delta live in the caller's [B,N,N] scratch
  const int bytes = (int)aco_lds_bytes(ENV, lds, a.N);
  const int grid = a.n_workgroups > 0 ? a.n_workgroups : a.B;
  if (decode_opts_on(o))
    return lds ? launch<aco_prize_kernel<ENV, true, true>>(a, bytes, s, grid, o)
               : launch<aco_prize_kernel<ENV, false, true>>(a, bytes, s, grid, o);
  return lds ? launch<aco_prize_kernel<ENV, true, false>>(a, bytes, s, grid, o)
             : launch<aco_prize_kernel<ENV, false, false>>(a, bytes, s, grid, o);
}

}  // namespace

extern "C" int rl4co_aco_prize_lds_nodes(int env) {
  if (env != RL4CO_ENV_OP && env != RL4CO_ENV_PCTSP) return -1;
  return lds_nodes([env](bool lds, int n) { return aco_lds_bytes(env, lds, n); });
}

extern "C" int rl4co_aco_prize(const rl4co_aco_prize_args* args, void* stream) {
  const rl4co_heatmap_decode_opts off = {};
  return rl4co_aco_prize_opts(args, &off, stream);
}

extern "C" int rl4co_aco_prize_opts(const rl4co_aco_prize_args* args, const rl4co_heatmap_decode_opts* opts, void* stream) {
  RL4CO_REQUIRE(args != nullptr);
  const rl4co_aco_prize_args& a = *args;
  RL4CO_REQUIRE(a.env == RL4CO_ENV_OP || a.env == RL4CO_ENV_PCTSP);
  if (const int rc = require_common(a)) return rc;
  if (const int rc = require_decode_opts(opts, a.ln_noise)) return rc;
  RL4CO_REQUIRE(a.n_workgroups >= 0 && a.n_workgroups <= a.B);
  const bool sample = (a.phases & RL4CO_ACO_SAMPLE) != 0;
  RL4CO_REQUIRE(sample ? a.T == a.N : a.T >= 2);  // sampled rows are W = N wide; UPDATE alone takes any width
  RL4CO_REQUIRE(!sample || (a.log_heuristic != nullptr && a.locs != nullptr && a.prize != nullptr));
  RL4CO_REQUIRE(!sample || a.env != RL4CO_ENV_OP || a.max_length != nullptr);
  RL4CO_REQUIRE(!sample || a.env != RL4CO_ENV_PCTSP || a.penalty != nullptr);
  RL4CO_REQUIRE(!sample || a.lengths != nullptr);
  hipStream_t s = rl4co::as_stream(stream);
  return a.env == RL4CO_ENV_OP ? launch_env<RL4CO_ENV_OP>(a, *opts, s) : launch_env<RL4CO_ENV_PCTSP>(a, *opts, s);
}

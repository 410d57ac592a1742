// aco_tsp.hip — Ant System search on a heatmap (models/zoo/deepaco/antsystem.py) for TSP as one launch for gfx950.
//
// One workgroup of four waves per INSTANCE runs `iterations` Ant System iterations of that instance. Rows are ant-major
// (the reference's batchify): row j * B + b is ant j of instance b.
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

#include "common.h"
#include "lds_tour_reward.h"
#include "rl4co_math.h"

namespace {

using rl4co::AntTour;  // lds_tour_reward.h: the reward of a tour held in LDS (shared with tsp_nls.hip)
using rl4co::ant_reward;

constexpr int kWaves = 4;
constexpr int kThreads = 64 * kWaves;
constexpr int kMaxNodes = 1024;
constexpr int kCuLds = 160 * 1024;
constexpr int kScratchBytes = 256;
constexpr int kTourBytes = kWaves * 2 * kMaxNodes;
constexpr int kStaticLds = 64;  // static LDS allowed beside the dynamic bytes (checked at launch)
constexpr int kEmpty = 0x7fffffff;
constexpr float kNegInf = -__builtin_huge_valf();

__host__ __device__ inline int64_t aco_lds_bytes(bool lds, int N) {
  return kScratchBytes + kTourBytes + (lds ? (int64_t)8 * N * N : 0);
}

template <bool LDS>
__global__ void __launch_bounds__(kThreads) aco_tsp_kernel(const rl4co_aco_tsp_args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* redf = reinterpret_cast<float*>(smem);                 // [2 * kWaves]
  int* redi = reinterpret_cast<int*>(smem + 32);                // [kWaves]
  uint32_t* bad_flag = reinterpret_cast<uint32_t*>(smem + 48);

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

  // ---- every index this instance will be addressed through, compared first --------------------------------------------
  if (tid == 0) *bad_flag = 0u;
  __syncthreads();
  {
    bool bad = false;
    if (sample) {
      for (int64_t e = tid; e < (int64_t)a.iterations * A; e += kThreads) {
        const int64_t it = e / A, j = e - it * A;
        const int64_t v = a.start_nodes[it * rows + j * B + b];
        bad |= v < 0 || v >= N;
      }
    }
    const int64_t* given = sample ? a.forced_actions : a.actions;
    if (given) {
      for (int64_t e = tid; e < (int64_t)A * N; e += kThreads) {
        const int64_t j = e / N, t = e - j * N;
        const int64_t v = given[(j * B + b) * N + t];
        bad |= v < 0 || v >= N;
      }
    }
    if (bad) *bad_flag = 1u;
  }
  __syncthreads();
  if (*bad_flag) {  // (uniform: one LDS word)
    if (tid == 0) atomicOr(a.err, RL4CO_EBIT_TOUR_INDEX);
    return;
  }

  if constexpr (LDS) {
    for (int e = tid; e < NN; e += kThreads) Pm[e] = gphe[e];
    __syncthreads();
  }

  const unsigned long long seed = a.philox_seed ^ (a.philox_seed_dev ? *a.philox_seed_dev : 0ull);
  const float* heu = sample ? a.log_heuristic + (int64_t)b * NN : nullptr;
  const float2* xy = a.locs ? reinterpret_cast<const float2*>(a.locs) + (int64_t)b * N : nullptr;
  const int K = (N + 63) >> 6;  // nodes per lane
  const float temp = a.temperature;
  uint32_t errbits = 0;
  bool have_best = a.has_best != 0;
  float best_r = have_best ? a.final_reward[b] : 0.0f;  // (uniform: every thread follows the same record)

  for (int it = 0; it < a.iterations; ++it) {
    if (sample) {
      // ---- A. the logits of this iteration ------------------------------------------------------------------------------
      for (int e = tid; e < NN; e += kThreads) {
        const float lp = a.alpha * rl4co_logf(Pm[e]);
        const float lh = a.beta * heu[e];
        Lm[e] = lp + lh;
      }
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
          const float* lrow = Lm + cur * N;
          bool nan_seen = false;
          float zmax = kNegInf;
          for (int k = 0; k < K; ++k) {
            const int n = lane + 64 * k;
            if (n < N && !((vis >> k) & 1u)) {
              float z = lrow[n];
              if (temp != 1.0f) z = z / temp;
              nan_seen |= z != z;
              zmax = fmaxf(zmax, z);
            }
          }
          zmax = rl4co::bfly_max<1, 64>(zmax);
          if (__any(nan_seen)) errbits |= RL4CO_EBIT_NAN_LOGIT;
          const bool dead = !(zmax > kNegInf);  // every feasible logit is -inf (or NaN): the lowest feasible node is taken
          if (dead) errbits |= RL4CO_EBIT_INFEASIBLE;
          float zsum = 0.0f;
          for (int k = 0; k < K; ++k) {
            const int n = lane + 64 * k;
            if (n < N && !((vis >> k) & 1u)) {
              float z = lrow[n];
              if (temp != 1.0f) z = z / temp;
              zsum = zsum + rl4co_expf(z - zmax);
            }
          }
          zsum = rl4co::bfly_sum<1, 64>(zsum);
          const float lse = rl4co_logf(zsum);

          const int forced = a.forced_actions ? (int)a.forced_actions[row * N + t] : -1;
          float* alp = a.all_logps ? a.all_logps + row * NN + (int64_t)t * N : nullptr;
          const float* lnz = a.ln_noise ? a.ln_noise + (((int64_t)it * (N - 1) + (t - 1)) * rows + row) * N : nullptr;
          float best = kNegInf, blp = kNegInf;  // best key of this lane, its log-prob (forced: the forced node's)
          int bi = kEmpty;
          for (int k = 0; k < K; ++k) {
            const int n = lane + 64 * k;
            if (n >= N) break;
            const bool feasible = !((vis >> k) & 1u);
            float lp = kNegInf;
            if (feasible && !dead) {
              float z = lrow[n];
              if (temp != 1.0f) z = z / temp;
              lp = (z - zmax) - lse;
            }
            if (alp) alp[n] = lp;
            if (!feasible) continue;
            if (forced >= 0) {
              if (n == forced) blp = lp;
            } else {
              const float ln = lnz ? lnz[n]
                                   : rl4co_logf(rl4co_exp1_noise(seed, a.philox_offset + (uint64_t)it * N + t, (uint32_t)row,
                                                                 (uint32_t)n));
              float key = lp - ln;  // multinomial(p, 1) == argmax(log p - log Exp(1))
              if (key != key) key = kNegInf;
              if (bi == kEmpty || key > best) {  // ascending nodes, strict '>': equal keys keep the lower node
                best = key;
                bi = n;
                blp = lp;
              }
            }
          }
          int chosen;
          if (forced >= 0) {
            chosen = forced;
          } else {
            rl4co::bfly_argmax(best, bi);
            chosen = __builtin_amdgcn_readfirstlane(bi);
            if (chosen == kEmpty) chosen = 0;  // (no feasible node: unreachable while fewer than N nodes are visited)
          }
          const float logp = __shfl(blp, chosen & 63, 64);
          const uint32_t was = __shfl(vis, chosen & 63, 64);
          if ((was >> (chosen >> 6)) & 1u) errbits |= RL4CO_EBIT_INFEASIBLE;  // a forced node that was visited already
          if (!(logp > -1000.0f)) errbits |= RL4CO_EBIT_NEG_INF_LOGP;         // decoding.py:56
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

    if (update) {
      // ---- U. best tour, reward map, pheromone -------------------------------------------------------------------------
      float mx = kNegInf, mn = -kNegInf;
      for (int j = tid; j < A; j += kThreads) {
        const float r = a.reward[(int64_t)j * B + b];
        mx = fmaxf(mx, r);
        mn = fminf(mn, r);
      }
      mx = rl4co::bfly_max<1, 64>(mx);
      mn = -rl4co::bfly_max<1, 64>(-mn);
      if (lane == 0) {
        redf[w] = mx;
        redf[kWaves + w] = mn;
      }
      __syncthreads();
      float M = redf[0], m = redf[kWaves];
      for (int x = 1; x < kWaves; ++x) {
        M = fmaxf(M, redf[x]);
        m = fminf(m, redf[kWaves + x]);
      }
      int bj = kEmpty;  // reward.argmax(-1): the lowest ant holding the maximum
      for (int j = tid; j < A; j += kThreads)
        if (a.reward[(int64_t)j * B + b] == M) bj = j < bj ? j : bj;
      bj = -rl4co::bfly_i_max(-bj);
      if (lane == 0) redi[w] = bj;
      __syncthreads();
      bj = redi[0];
      for (int x = 1; x < kWaves; ++x) bj = redi[x] < bj ? redi[x] : bj;
      if (bj == kEmpty) bj = 0;  // (every reward NaN)
      if (!have_best || best_r <= M) {  // antsystem.py:238-245: equal rewards replace too
        best_r = M;
        const int64_t* src = a.actions + ((int64_t)bj * B + b) * N;
        for (int t = tid; t < N; t += kThreads) a.final_actions[(int64_t)b * N + t] = src[t];
        if (tid == 0) a.final_reward[b] = M;
      }
      have_best = true;
      if (tid == 0 && a.final_reward_cache) a.final_reward_cache[(int64_t)it * B + b] = best_r;

      for (int e = tid; e < NN; e += kThreads) Lm[e] = 0.0f;  // delta, in the logits' storage
      __syncthreads();
      const float span = M - m;
      for (int j = 0; j < A; ++j) {
        const float r = a.reward[(int64_t)j * B + b];
        const float x = (r - m) / span;  // NOT guarded: M == m gives NaN as in the reference
        const float v = (x * x) * a.Q;
        const int64_t* act = a.actions + ((int64_t)j * B + b) * N;
        for (int t = tid; t < N - 1; t += kThreads) {
          const int e = (int)act[t] * N + (int)act[t + 1];
          Lm[e] = Lm[e] + v;
        }
        __syncthreads();  // ant j is deposited before ant j + 1: every edge's sum is in ant order
      }
      if (tid == 0) Lm[0] = 0.0f;
      __syncthreads();
      for (int e = tid; e < NN; e += kThreads) {
        const float kept = Pm[e] * a.decay;
        Pm[e] = kept + Lm[e];
      }
      __syncthreads();
    }
  }

  if constexpr (LDS) {
    if (update)
      for (int e = tid; e < NN; e += kThreads) gphe[e] = Pm[e];
  }
  if (errbits) atomicOr(a.err, (int)errbits);
}

template <bool LDS>
int launch(const rl4co_aco_tsp_args& a, hipStream_t stream) {
  const int lds = (int)aco_lds_bytes(LDS, a.N);
  hipFuncAttributes fa;
  RL4CO_HIP_TRY(hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(aco_tsp_kernel<LDS>)));
  RL4CO_REQUIRE((int64_t)fa.sharedSizeBytes <= kStaticLds);  // the budget of rl4co_aco_tsp_lds_nodes holds
  if (lds > 64 * 1024) {
    RL4CO_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(aco_tsp_kernel<LDS>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  }
  hipLaunchKernelGGL((aco_tsp_kernel<LDS>), dim3(a.B), dim3(kThreads), lds, stream, a);
  RL4CO_HIP_TRY(hipGetLastError());
  return RL4CO_OK;
}

}  // namespace

extern "C" int rl4co_aco_tsp_lds_nodes(void) {
  int n = kMaxNodes;
  while (n > 0 && aco_lds_bytes(true, n) + kStaticLds > kCuLds) --n;
  return n;
}

extern "C" int rl4co_aco_tsp(const rl4co_aco_tsp_args* args, void* stream) {
  RL4CO_REQUIRE(args != nullptr);
  const rl4co_aco_tsp_args& a = *args;
  RL4CO_REQUIRE(a.B >= 1);
  RL4CO_REQUIRE(a.N >= 2 && a.N <= 1024);
  RL4CO_REQUIRE(a.n_ants >= 1);
  RL4CO_REQUIRE((int64_t)a.n_ants * a.B <= 2147483647LL);
  RL4CO_REQUIRE(a.iterations >= 1);
  RL4CO_REQUIRE(a.phases >= 1 && a.phases <= (RL4CO_ACO_SAMPLE | RL4CO_ACO_UPDATE));
  const bool sample = (a.phases & RL4CO_ACO_SAMPLE) != 0, update = (a.phases & RL4CO_ACO_UPDATE) != 0;
  RL4CO_REQUIRE((sample && update) || a.iterations == 1);  // one phase alone runs once
  RL4CO_REQUIRE(!(sample && update) || a.locs != nullptr);  // the update needs the sampled tours' rewards
  RL4CO_REQUIRE(a.temperature > 0.0f);
  RL4CO_REQUIRE(!sample || (a.log_heuristic != nullptr && a.start_nodes != nullptr));
  RL4CO_REQUIRE(a.forced_actions == nullptr || (sample && a.iterations == 1));
  RL4CO_REQUIRE(a.pheromone != nullptr);
  RL4CO_REQUIRE(a.actions != nullptr);
  RL4CO_REQUIRE(a.reward != nullptr);
  RL4CO_REQUIRE(!update || (a.final_reward != nullptr && a.final_actions != nullptr));
  RL4CO_REQUIRE(a.err != nullptr);
  const bool lds = a.N <= rl4co_aco_tsp_lds_nodes();
  RL4CO_REQUIRE(lds || a.logits_scratch != nullptr);  // above the LDS tier L / delta live in the caller's [B,N,N] scratch
  hipStream_t s = rl4co::as_stream(stream);
  return lds ? launch<true>(a, s) : launch<false>(a, s);
}

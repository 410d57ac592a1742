// aco_cvrp.hip — Ant System search on a heatmap (models/zoo/deepaco/antsystem.py) for CVRP as one launch for gfx950.
//
// aco_tsp.hip's layout with CVRP's transition rule inside the step: one workgroup of four waves per INSTANCE runs
// `iterations` Ant System iterations of that instance; rows are ant-major (row j * B + b is ant j of instance b).
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
//              prepend_depot RESTATED as aco_tsp.hip restates it (ATen's vector_norm over two elements, then SumKernel's
//              8-lane / 4-ILP / 4-level cascade over W + 1 segments; the expression text equals that file's TourView::seg
//              and lane_row_sum — change all three together). Bit-equal to CVRPEnv.get_reward on the W-wide zero-padded row.
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

#include "common.h"
#include "rl4co_math.h"

namespace {

constexpr int kWaves = 4;
constexpr int kThreads = 64 * kWaves;
constexpr int kMaxNodes = 1024;
constexpr int kCuLds = 160 * 1024;
constexpr int kScratchBytes = 256;
constexpr int kStaticLds = 64;  // static LDS allowed beside the dynamic bytes (checked at launch)
constexpr int kEmpty = 0x7fffffff;
constexpr float kNegInf = -__builtin_huge_valf();

__host__ __device__ inline int cvrp_width(int N) {  // W
  const int C = N - 1;
  return C + 1 > 2 * C - 1 ? C + 1 : 2 * C - 1;
}
__host__ __device__ inline int demand_bytes(int N) { return 4 * ((N + 3) & ~3); }
__host__ __device__ inline int tour_stride(int N) { return (cvrp_width(N) + 1 + 7) & ~7; }  // uint16_t per wave
__host__ __device__ inline int64_t aco_lds_bytes(bool lds, int N) {
  return kScratchBytes + demand_bytes(N) + kWaves * 2 * tour_stride(N) + (lds ? (int64_t)8 * N * N : 0);
}

// ---- reward: tour_length.hip's TourView::seg / lane_row_sum over the wave's LDS tour (same text, same order) -----------
struct AntTour {
  const uint16_t* tour;  // [n] in LDS: the depot, then the W actions
  const float2* xy;      // [N] of the instance
  int n;
  __device__ inline float seg(int t) const {
    const float2 p0 = xy[tour[t]];
    const float2 p1 = xy[tour[t + 1 == n ? 0 : t + 1]];  // torch.roll(-1)
    const float dx = p1.x - p0.x;
    const float dy = p1.y - p0.y;
    return sqrtf(fmaf(dy, dy, dx * dx));
  }
};

__device__ float lane_row_sum(const AntTour& tv, int lane8, int nvec) {
  constexpr int kIlp = 4;
  constexpr int kLevels = 4;
  const int size = nvec / kIlp;  // size_ilp
  int ceil_log2 = 0;
  while ((1LL << ceil_log2) < size) ++ceil_log2;
  int level_power = ceil_log2 / kLevels;
  if (level_power < 4) level_power = 4;
  const int level_step = 1 << level_power;
  const int level_mask = level_step - 1;
  float acc[kLevels][kIlp];
  for (int l = 0; l < kLevels; ++l)
    for (int k = 0; k < kIlp; ++k) acc[l][k] = 0.0f;
  int i = 0;
  for (; i + level_step <= size;) {
    for (int j = 0; j < level_step; ++j, ++i) {
      for (int k = 0; k < kIlp; ++k) acc[0][k] = acc[0][k] + tv.seg(8 * (i * kIlp + k) + lane8);
    }
    for (int j = 1; j < kLevels; ++j) {
      for (int k = 0; k < kIlp; ++k) {
        acc[j][k] = acc[j][k] + acc[j - 1][k];
        acc[j - 1][k] = 0.0f;
      }
      const int mask = level_mask << (j * level_power);
      if ((i & mask) != 0) break;
    }
  }
  for (; i < size; ++i) {
    for (int k = 0; k < kIlp; ++k) acc[0][k] = acc[0][k] + tv.seg(8 * (i * kIlp + k) + lane8);
  }
  for (int j = 1; j < kLevels; ++j)
    for (int k = 0; k < kIlp; ++k) acc[0][0] = acc[0][0] + acc[j][k];
  for (int v = size * kIlp; v < nvec; ++v) acc[0][0] = acc[0][0] + tv.seg(8 * v + lane8);
  for (int k = 1; k < kIlp; ++k) acc[0][0] = acc[0][0] + acc[0][k];
  return acc[0][0];
}

// minus the closed tour length, valid in lane 0; the whole wave calls it (tour_length_kernel's body for one trajectory)
__device__ float ant_reward(const AntTour& tv, int lane) {
  const int n = tv.n;
  const int nvec = n / 8;
  if (n < 8) {  // ATen's scalar_inner_sum
    float p[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (lane == 0) {
      const int g = n / 4;
      for (int i = 0; i < g; ++i)
        for (int k = 0; k < 4; ++k) p[k] = p[k] + tv.seg(4 * i + k);
      for (int k = 4 * g; k < n; ++k) p[0] = p[0] + tv.seg(k);
      for (int k = 1; k < 4; ++k) p[0] = p[0] + p[k];
    }
    return -p[0];
  }
  float part = 0.0f;
  if (lane < 8) part = lane_row_sum(tv, lane, nvec);
  float fin = 0.0f;
  if (lane == 0) {
    for (int k = nvec * 8; k < n; ++k) fin = fin + tv.seg(k);
  }
  for (int l = 0; l < 8; ++l) {
    const float pl = __shfl(part, l, 64);
    fin = fin + pl;
  }
  return -fin;
}

template <bool LDS>
__global__ void __launch_bounds__(kThreads) aco_cvrp_kernel(const rl4co_aco_cvrp_args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* redf = reinterpret_cast<float*>(smem);                 // [2 * kWaves]
  int* redi = reinterpret_cast<int*>(smem + 32);                // [kWaves]
  uint32_t* bad_flag = reinterpret_cast<uint32_t*>(smem + 48);

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

  // ---- every index this instance will be addressed through, compared first --------------------------------------------
  if (tid == 0) *bad_flag = 0u;
  __syncthreads();
  {
    bool bad = false;
    if (sample && a.start_nodes) {
      for (int64_t e = tid; e < (int64_t)a.iterations * A; e += kThreads) {
        const int64_t it = e / A, j = e - it * A;
        const int64_t v = a.start_nodes[it * rows + j * B + b];
        bad |= v < 1 || v >= N;  // a start is a customer
      }
    }
    const int64_t* given = sample ? a.forced_actions : a.actions;
    if (given) {
      for (int64_t e = tid; e < (int64_t)A * T; e += kThreads) {
        const int64_t j = e / T, t = e - j * T;
        const int64_t v = given[(j * B + b) * T + t];
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
  const float temp = a.temperature;
  const float thr = sample ? a.vehicle_capacity[b] + 1e-5f : 0.0f;  // cvrp/env.py:129, one fp32 add
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
        // the reset state (cvrp/env.py:98-124): at the depot, nothing visited — not the depot either
        int cur = 0, left = C, t = 0;
        uint32_t vis = 0u;  // bit k: node lane + 64 k is visited
        float used = 0.0f;
        bool depot_seen = false;
        if (lane == 0) wtour[0] = 0;  // the prepended depot of the reward
        if (a.start_nodes) {  // multistart: action 0 is given, log-prob 0, stepped through the state
          cur = __builtin_amdgcn_readfirstlane((int)a.start_nodes[(int64_t)it * rows + row]);
          used = (used + dnode[cur]) * 1.0f;
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
            if (n >= 1 && n < N && !((vis >> k) & 1u) && !(dnode[n] + used > thr)) feas |= 1u << k;
          }
          const bool any_customer = __any(feas != 0u);
          if (lane == 0 && !(cur == 0 && any_customer)) feas |= 1u;

          const float* lrow = Lm + cur * N;
          bool nan_seen = false;
          float zmax = kNegInf;
          for (int k = 0; k < K; ++k) {
            const int n = lane + 64 * k;
            if (n < N && ((feas >> k) & 1u)) {
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
            if (n < N && ((feas >> k) & 1u)) {
              float z = lrow[n];
              if (temp != 1.0f) z = z / temp;
              zsum = zsum + rl4co_expf(z - zmax);
            }
          }
          zsum = rl4co::bfly_sum<1, 64>(zsum);
          const float lse = rl4co_logf(zsum);

          const int forced = a.forced_actions ? (int)a.forced_actions[row * W + t] : -1;
          float* alp = a.all_logps ? a.all_logps + (row * W + t) * N : nullptr;
          const float* lnz = a.ln_noise ? a.ln_noise + (((int64_t)it * W + t) * rows + row) * N : nullptr;
          float best = kNegInf, blp = kNegInf;  // best key of this lane, its log-prob (forced: the forced node's)
          int bi = kEmpty;
          for (int k = 0; k < K; ++k) {
            const int n = lane + 64 * k;
            if (n >= N) break;
            const bool feasible = (feas >> k) & 1u;
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
                                   : rl4co_logf(rl4co_exp1_noise(seed, a.philox_offset + (uint64_t)it * W + t, (uint32_t)row,
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
            chosen = __builtin_amdgcn_readfirstlane(forced);
          } else {
            rl4co::bfly_argmax(best, bi);
            chosen = __builtin_amdgcn_readfirstlane(bi);
            if (chosen == kEmpty) chosen = 0;  // (no feasible node: unreachable, the depot is feasible when no customer is)
          }
          const float logp = __shfl(blp, chosen & 63, 64);
          const uint32_t could = __shfl(feas, chosen & 63, 64);
          const uint32_t was = __shfl(vis, chosen & 63, 64);
          if (!((could >> (chosen >> 6)) & 1u)) errbits |= RL4CO_EBIT_INFEASIBLE;  // a forced node that is infeasible
          if (!(logp > -1000.0f)) errbits |= RL4CO_EBIT_NEG_INF_LOGP;              // decoding.py:56
          // cvrp/env.py:66-96 (cvrp_step_body's order)
          used = (used + dnode[chosen]) * (chosen != 0 ? 1.0f : 0.0f);
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
        const int64_t* src = a.actions + ((int64_t)bj * B + b) * T;
        for (int t = tid; t < T; t += kThreads) a.final_actions[(int64_t)b * T + t] = src[t];
        if (tid == 0) {
          a.final_reward[b] = M;
          if (a.final_iteration) a.final_iteration[b] = a.iteration_base + it;
        }
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
        const int64_t* act = a.actions + ((int64_t)j * B + b) * T;
        for (int t = tid; t < T - 1; t += kThreads) {
          const int from = (int)act[t], to = (int)act[t + 1];
          if ((from | to) == 0) continue;  // delta[0][0] = 0 (antsystem.py:265): the trailing zeros deposit nothing
          const int e = from * N + to;
          Lm[e] = Lm[e] + v;
        }
        __syncthreads();  // ant j is deposited before ant j + 1: every edge's sum is in ant order
      }
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
int launch(const rl4co_aco_cvrp_args& a, hipStream_t stream) {
  const int lds = (int)aco_lds_bytes(LDS, a.N);
  hipFuncAttributes fa;
  RL4CO_HIP_TRY(hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(aco_cvrp_kernel<LDS>)));
  RL4CO_REQUIRE((int64_t)fa.sharedSizeBytes <= kStaticLds);  // the budget of rl4co_aco_cvrp_lds_nodes holds
  if (lds > 64 * 1024) {
    RL4CO_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(aco_cvrp_kernel<LDS>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  }
  hipLaunchKernelGGL((aco_cvrp_kernel<LDS>), dim3(a.B), dim3(kThreads), lds, stream, a);
  RL4CO_HIP_TRY(hipGetLastError());
  return RL4CO_OK;
}

}  // namespace

extern "C" int rl4co_aco_cvrp_lds_nodes(void) {
  int n = kMaxNodes;
  while (n > 0 && aco_lds_bytes(true, n) + kStaticLds > kCuLds) --n;
  return n;
}

extern "C" int rl4co_aco_cvrp(const rl4co_aco_cvrp_args* args, void* stream) {
  RL4CO_REQUIRE(args != nullptr);
  const rl4co_aco_cvrp_args& a = *args;
  RL4CO_REQUIRE(a.B >= 1);
  RL4CO_REQUIRE(a.N >= 2 && a.N <= 1024);
  RL4CO_REQUIRE(a.n_ants >= 1);
  RL4CO_REQUIRE((int64_t)a.n_ants * a.B <= 2147483647LL);
  RL4CO_REQUIRE(a.iterations >= 1);
  RL4CO_REQUIRE(a.phases >= 1 && a.phases <= (RL4CO_ACO_SAMPLE | RL4CO_ACO_UPDATE));
  const bool sample = (a.phases & RL4CO_ACO_SAMPLE) != 0, update = (a.phases & RL4CO_ACO_UPDATE) != 0;
  RL4CO_REQUIRE((sample && update) || a.iterations == 1);  // one phase alone runs once
  RL4CO_REQUIRE(!(sample && update) || a.locs != nullptr);  // the update needs the sampled tours' rewards
  RL4CO_REQUIRE(sample ? a.T == cvrp_width(a.N) : a.T >= 2);  // sampled rows are W wide; UPDATE alone takes any width
  RL4CO_REQUIRE(a.temperature > 0.0f);
  RL4CO_REQUIRE(!sample || (a.log_heuristic != nullptr && a.demand != nullptr && a.vehicle_capacity != nullptr));
  RL4CO_REQUIRE(!sample || a.lengths != nullptr);
  RL4CO_REQUIRE(a.forced_actions == nullptr || (sample && a.iterations == 1));
  RL4CO_REQUIRE(a.pheromone != nullptr);
  RL4CO_REQUIRE(a.actions != nullptr);
  RL4CO_REQUIRE(a.reward != nullptr);
  RL4CO_REQUIRE(!update || (a.final_reward != nullptr && a.final_actions != nullptr));
  RL4CO_REQUIRE(a.err != nullptr);
  const bool lds = a.N <= rl4co_aco_cvrp_lds_nodes();
  RL4CO_REQUIRE(lds || a.logits_scratch != nullptr);  // above the LDS tier L / delta live in the caller's [B,N,N] scratch
  hipStream_t s = rl4co::as_stream(stream);
  return lds ? launch<true>(a, s) : launch<false>(a, s);
}

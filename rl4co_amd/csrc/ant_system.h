// ant_system.h — what the Ant System kernels (aco_tsp.hip, aco_cvrp.hip, aco_prize.hip) share, stated once: the constants and the scratch
// words, the index pre-check, stage A (the logits), one sampling step of one wave, stage U (record, reward map, pheromone)
// and the host side (launch, the LDS-tier search, the argument checks common to both entry points). A kernel keeps its
// LDS layout, its per-ant state, its tour / actions / logps stores and its R stage (lds_tour_reward.h). aco_tsp_grad.hip (the
// backward of the ants' log-likelihoods) takes the constants, the index pre-check, the log-softmax statistics and the launch.
// Thread layout of both: one workgroup of kWaves waves per instance, one wave per ant, lane l owns nodes l, l + 64, ...
// Every floating-point expression below is part of the parity contract (-ffp-contract=off; tests compare bit for bit).
#pragma once

#include <hip/hip_runtime.h>

#include "common.h"
#include "rl4co_math.h"
#include "topkp.h"

namespace rl4co::aco {

constexpr int kWaves = 4;
constexpr int kThreads = 64 * kWaves;
constexpr int kMaxNodes = 1024;
constexpr int kCuLds = 160 * 1024;
constexpr int kScratchBytes = 256;  // the first bytes of the dynamic LDS: the words below
constexpr int kStaticLds = 64;      // static LDS allowed beside the dynamic bytes (checked at launch)
constexpr int kEmpty = 0x7fffffff;
constexpr float kNegInf = -__builtin_huge_valf();

__device__ inline float* redf(unsigned char* smem) { return reinterpret_cast<float*>(smem); }                  // [2 * kWaves]
__device__ inline int* redi(unsigned char* smem) { return reinterpret_cast<int*>(smem + 32); }                 // [kWaves]
__device__ inline uint32_t* bad_flag(unsigned char* smem) { return reinterpret_cast<uint32_t*>(smem + 48); }

// Every index instance b will be addressed through, compared before anything is read or written through it: the start
// nodes [iterations, rows] against [start_lo, N) (nullptr: none are given) and the given rows [rows, T] (forced actions, or
// the input actions of UPDATE alone; nullptr: none) against [0, N). One out of range raises RL4CO_EBIT_TOUR_INDEX and
// returns false to EVERY thread (decided from one LDS word: the caller's early exit is uniform). Two workgroup barriers.
__device__ inline bool check_indices(const int64_t* start_nodes, int start_lo, int iterations, const int64_t* given, int T,
                                     int A, int B, int b, int N, unsigned char* smem, int32_t* err) {
  const int tid = threadIdx.x;
  const int64_t rows = (int64_t)A * B;
  if (tid == 0) *bad_flag(smem) = 0u;
  __syncthreads();
  bool bad = false;
  if (start_nodes) {
    for (int64_t e = tid; e < (int64_t)iterations * A; e += kThreads) {
      const int64_t it = e / A, j = e - it * A;
      const int64_t v = start_nodes[it * rows + j * B + b];
      bad |= v < start_lo || v >= N;
    }
  }
  if (given) {
    for (int64_t e = tid; e < (int64_t)A * T; e += kThreads) {
      const int64_t j = e / T, t = e - j * T;
      const int64_t v = given[(j * B + b) * T + t];
      bad |= v < 0 || v >= N;
    }
  }
  if (bad) *bad_flag(smem) = 1u;
  __syncthreads();
  if (*bad_flag(smem) == 0u) return true;
  if (tid == 0) atomicOr(err, RL4CO_EBIT_TOUR_INDEX);
  return false;
}

// A. L[e] = alpha * rl4co_logf(phe[e]) + beta * log_heu[e]: two multiplies, one add, each rounded once. No barrier.
__device__ inline void build_logits(float* Lm, const float* Pm, const float* heu, int NN, float alpha, float beta, int tid) {
  for (int e = tid; e < NN; e += kThreads) {
    const float lp = alpha * rl4co_logf(Pm[e]);
    const float lh = beta * heu[e];
    Lm[e] = lp + lh;
  }
}

// The two statistics of a masked log-softmax in the project's order: log_softmax_max, the max butterfly over the feasible
// logits, and log_softmax_lse = rl4co_logf of the butterfly of the lane-strided (ascending k) sum of rl4co_expf(z - zmax);
// lp[n] = (z - zmax) - lse.
// z(k, n) is the logit of node n = lane + 64 k, already divided by the temperature; it is asked only where n < N and
// feasible(k). `nan_seen`: a feasible logit of THIS lane is NaN. Stated once for ant_step and for the backward
// (aco_tsp_grad.hip), which therefore sees the probabilities the forward's log-probs report.
template <typename ZFn, typename FeasFn>
__device__ inline float log_softmax_max(int N, int K, int lane, ZFn z, FeasFn feasible, bool& nan_seen) {
  nan_seen = false;
  float zmax = kNegInf;
  for (int k = 0; k < K; ++k) {
    const int n = lane + 64 * k;
    if (n < N && feasible(k)) {
      const float zn = z(k, n);
      nan_seen |= zn != zn;
      zmax = fmaxf(zmax, zn);
    }
  }
  return rl4co::bfly_max<1, 64>(zmax);
}

template <typename ZFn, typename FeasFn>
__device__ inline float log_softmax_lse(int N, int K, int lane, ZFn z, FeasFn feasible, float zmax) {
  float zsum = 0.0f;
  for (int k = 0; k < K; ++k) {
    const int n = lane + 64 * k;
    if (n < N && feasible(k)) zsum = zsum + rl4co_expf(z(k, n) - zmax);
  }
  zsum = rl4co::bfly_sum<1, 64>(zsum);
  return rl4co_logf(zsum);
}

// The kept set of one step under top-k / top-p (utils/decoding.py:109-188), for one wave, as bits: z[k] is the logit of node
// lane + 64 k, already divided by the temperature, read only where bit k of `feas` is set and the node is below N. Returns
// `feas` (cut to the nodes below N) without the bits the filter removes. This is topkp.h's topkp_filter in register form:
// a lane holds its nodes' keys and masses in registers instead of walking a list in LDS, the list position c is the node,
// and what is removed leaves the bit mask instead of becoming -inf. Restated from topkp.h: lines 37-54 (top-k: the k-th
// largest topkp_key by 32 counting passes with bfly_i_sum, keys < tau removed, ties at tau stay; fewer than k feasible nodes
// remove nothing; a feasible -inf counts, so tau can be -inf's key and nothing is below it), lines 55-63 (`mass`) and lines
// 64-89 (top-p over the survivors in (z, node) ascending order: removed while the cumulative mass is <= (1 - p) Z, the
// threshold kept under Z so that the largest logit always stays). The masses are rl4co_expf(z - zmax) and every sum of them
// runs lane-strided over ascending k and then through the butterfly, the order of log_softmax_lse. Stated once for ant_step
// and for the two backward kernels, which therefore see exactly the set the forward sampled from.
template <int KMAX>
__device__ inline uint32_t filter_kept(const float (&z)[KMAX], uint32_t feas, int N, int lane, int top_k, float top_p) {
  uint32_t kept = 0u;
  uint32_t key[KMAX];
  int mine = 0;
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    const bool live = lane + 64 * k < N && ((feas >> k) & 1u) != 0;
    key[k] = live ? rl4co::topkp_key(z[k]) : 0u;
    if (live) {
      kept |= 1u << k;
      ++mine;
    }
  }
  if (top_k > 0 && top_k < rl4co::bfly_i_sum(mine)) {
    // tau = largest T with #{n : key_n >= T} >= k = the key of the k-th largest z, counted with multiplicity
    uint32_t tau = 0;
#pragma unroll 1
    for (int b = 31; b >= 0; --b) {
      const uint32_t cand = tau | (1u << b);
      int n = 0;
#pragma unroll
      for (int k = 0; k < KMAX; ++k) n += (((kept >> k) & 1u) && key[k] >= cand) ? 1 : 0;
      if (rl4co::bfly_i_sum(n) >= top_k) tau = cand;
    }
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (key[k] < tau) kept &= ~(1u << k);  // the reference removes logits < tau: ties at tau stay
  }
  if (top_p > 0.0f && top_p < 1.0f) {
    float zmax = kNegInf;
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if ((kept >> k) & 1u) zmax = fmaxf(zmax, z[k]);
    zmax = rl4co::bfly_max<1, 64>(zmax);
    if (zmax > kNegInf) {  // (wave-uniform) else every kept logit is -inf (or NaN): nothing to order
      float e[KMAX];
#pragma unroll
      for (int k = 0; k < KMAX; ++k) e[k] = ((kept >> k) & 1u) ? rl4co_expf(z[k] - zmax) : 0.0f;
      const auto mass = [&](uint32_t below, uint32_t at, int upto) {  // sum of e over key < below, or key == at and n <= upto
        float s = 0.0f;
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
          if ((kept >> k) & 1u) s = s + ((key[k] < below || (key[k] == at && lane + 64 * k <= upto)) ? e[k] : 0.0f);
        return rl4co::bfly_sum<1, 64>(s);
      };
      // nodes ordered by (z, n) ascending; n is removed iff A_n = mass of the nodes up to n <= (1 - p) Z
      const float zall = mass(0xFFFFFFFFu, 0xFFFFFFFFu, 0x7fffffff);
      const float thr = fminf((1.0f - top_p) * zall, __uint_as_float(__float_as_uint(zall) - 1u));
      uint32_t cut = 0;  // largest T with mass(key < T) <= thr: below it all removed, above it all kept
#pragma unroll 1
      for (int b = 31; b >= 0; --b) {
        const uint32_t cand = cut | (1u << b);
        if (mass(cand, 0u, -1) <= thr) cut = cand;
      }
      int lo = -1, hi = N;  // the tie group at the cut, by node: the largest lo with A(lo) <= thr
#pragma unroll 1
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (mass(cut, cut, mid) <= thr) lo = mid; else hi = mid;
      }
#pragma unroll
      for (int k = 0; k < KMAX; ++k)
        if (key[k] < cut || (key[k] == cut && lane + 64 * k <= lo)) kept &= ~(1u << k);
    }
  }
  return kept;
}

// whether the options ask for anything (all off: the entry points launch the instantiation without them)
__host__ __device__ inline bool decode_opts_on(const rl4co_heatmap_decode_opts& o) {
  return o.greedy != 0 || o.top_k > 0 || (o.top_p > 0.0f && o.top_p < 1.0f);
}
__host__ __device__ inline bool decode_filter_on(const rl4co_heatmap_decode_opts& o) {
  return o.top_k > 0 || (o.top_p > 0.0f && o.top_p < 1.0f);
}

// filter_kept on row `lrow` of L: the lane's logits into KMAX registers (the quotient ant_step forms), KMAX >= K
template <int KMAX>
__device__ inline uint32_t filter_kept_row(const float* lrow, int N, int lane, uint32_t feas, float temp, int top_k,
                                           float top_p) {
  float z[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    const int n = lane + 64 * k;
    float v = 0.0f;
    if (n < N && ((feas >> k) & 1u)) {
      v = lrow[n];
      if (temp != 1.0f) v = v / temp;
    }
    z[k] = v;
  }
  return filter_kept<KMAX>(z, feas, N, lane, top_k, top_p);
}

// One sampling step of one wave: row `lrow` of L over the nodes of `feas` (bit k of a lane: node lane + 64 k is feasible;
// bits of nodes >= N are not read), divided by `temp` when it is not 1, log-softmax in the project's order (max butterfly,
// lane-strided sum of rl4co_expf, butterfly, rl4co_logf), then the argmax over feasible n of lp[n] - ln_noise[n], lowest
// node on equal keys (a NaN key counts as -inf). ln_noise[n] is lnz[n], or with lnz == nullptr
// rl4co_logf(rl4co_exp1_noise(seed, counter, row, n)). forced >= 0: that node is taken and only its log-prob computed.
// alp != nullptr: receives the N log-probs (-inf on infeasible nodes). Returns the chosen node (wave-uniform) and its
// log-prob in `logp`; ORs into `errbits` RL4CO_EBIT_NAN_LOGIT (a feasible logit is NaN), RL4CO_EBIT_INFEASIBLE (every
// feasible logit is -inf or NaN: the lowest feasible node is taken) and RL4CO_EBIT_NEG_INF_LOGP. The caller checks a forced
// node against its own mask, updates its state and stores.
// OPTS (a compile-time choice; false is the step above and reads no `o`): with top_k / top_p the feasible set is first cut
// to filter_kept's and everything after runs on the kept set, so a removed node has lp = -inf in `alp` and a forced node
// outside the kept set gets logp = -inf and raises RL4CO_EBIT_NEG_INF_LOGP (decoding.py:56). With `greedy` the key is lp
// itself: the argmax over the kept set, lowest node on equal values; no noise is read and no Philox word is drawn.
template <bool OPTS = false>
__device__ inline int ant_step(const float* lrow, int N, int K, int lane, uint32_t feas, float temp, int forced, float* alp,
                               const float* lnz, unsigned long long seed, uint64_t counter, uint32_t row, float& logp,
                               uint32_t& errbits, const rl4co_heatmap_decode_opts* o = nullptr) {
  if constexpr (OPTS) {
    if (decode_filter_on(*o)) {  // (uniform over the launch)
      if (K <= 1) feas = filter_kept_row<1>(lrow, N, lane, feas, temp, o->top_k, o->top_p);
      else if (K <= 2) feas = filter_kept_row<2>(lrow, N, lane, feas, temp, o->top_k, o->top_p);
      else if (K <= 4) feas = filter_kept_row<4>(lrow, N, lane, feas, temp, o->top_k, o->top_p);
      else if (K <= 8) feas = filter_kept_row<8>(lrow, N, lane, feas, temp, o->top_k, o->top_p);
      else feas = filter_kept_row<16>(lrow, N, lane, feas, temp, o->top_k, o->top_p);
    }
  }
  const auto z_of = [&](int, int n) {
    float z = lrow[n];
    if (temp != 1.0f) z = z / temp;
    return z;
  };
  const auto feas_of = [&](int k) { return ((feas >> k) & 1u) != 0; };
  bool nan_seen;
  const float zmax = log_softmax_max(N, K, lane, z_of, feas_of, nan_seen);
  if (__any(nan_seen)) errbits |= RL4CO_EBIT_NAN_LOGIT;
  const bool dead = !(zmax > kNegInf);  // every feasible logit is -inf (or NaN): the lowest feasible node is taken
  if (dead) errbits |= RL4CO_EBIT_INFEASIBLE;
  const float lse = log_softmax_lse(N, K, lane, z_of, feas_of, zmax);

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
      float key;
      bool greedy = false;
      if constexpr (OPTS) greedy = o->greedy != 0;
      if (greedy) {
        key = lp;
      } else {
        const float ln = lnz ? lnz[n] : rl4co_logf(rl4co_exp1_noise(seed, counter, row, (uint32_t)n));
        key = lp - ln;  // multinomial(p, 1) == argmax(log p - log Exp(1))
      }
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
    if (chosen == kEmpty) chosen = 0;  // (no feasible node: neither kernel reaches a step in that state)
  }
  logp = __shfl(blp, chosen & 63, 64);
  if (!(logp > -1000.0f)) errbits |= RL4CO_EBIT_NEG_INF_LOGP;  // decoding.py:56
  return chosen;
}

// U. best tour, reward map, pheromone of instance b over its A ants (rows j * B + b of `actions` [rows, T] and `reward`),
// bit for bit the reference's _update_results / _reward_map / _update_pheromone: M, m = max, min reward; best ant = lowest
// j with r_j == M; the first iteration or best_r <= M replaces final_reward / final_actions (and final_iteration[b] =
// iteration_base + it where the pointer is given); v_j = (((r_j - m) / (M - m)) * same) * Q, NOT guarded against M == m;
// delta = 0 in L's storage, then for ants in ascending order each directed edge (a_t, a_t+1), t = 0 .. T - 2, gets
// delta[from][to] += v_j, a workgroup barrier between ants keeping the ant order of every sum; phe = phe * decay + delta.
// The reference zeroes delta[0][0] afterwards (antsystem.py:265). SkipDepotLoop says how that is done:
//   false  every edge is deposited, then delta[0][0] = 0. For rows with at most one (0, 0) edge per ant (a TSP
//          permutation has at most one edge leaving node 0), whose edges are therefore distinct words.
//   true   (0, 0) edges are skipped and nothing is zeroed: the same matrix, without a race on that word where a row holds
//          many of them (CVRP's trailing zeros).
// The whole workgroup calls it; no barrier sits inside divergent control flow.
template <bool SkipDepotLoop>
__device__ inline void update_phase(const int64_t* actions, int T, const float* reward, float* final_reward,
                                    int64_t* final_actions, float* final_reward_cache, int32_t* final_iteration,
                                    int iteration_base, float* Lm, float* Pm, int N, int A, int B, int b, int it, float decay,
                                    float Q, bool& have_best, float& best_r, unsigned char* smem) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int NN = N * N;
  float* rf = redf(smem);
  int* ri = redi(smem);
  float mx = kNegInf, mn = -kNegInf;
  for (int j = tid; j < A; j += kThreads) {
    const float r = reward[(int64_t)j * B + b];
    mx = fmaxf(mx, r);
    mn = fminf(mn, r);
  }
  mx = rl4co::bfly_max<1, 64>(mx);
  mn = -rl4co::bfly_max<1, 64>(-mn);
  if (lane == 0) {
    rf[w] = mx;
    rf[kWaves + w] = mn;
  }
  __syncthreads();
  float M = rf[0], m = rf[kWaves];
  for (int x = 1; x < kWaves; ++x) {
    M = fmaxf(M, rf[x]);
    m = fminf(m, rf[kWaves + x]);
  }
  int bj = kEmpty;  // reward.argmax(-1): the lowest ant holding the maximum
  for (int j = tid; j < A; j += kThreads)
    if (reward[(int64_t)j * B + b] == M) bj = j < bj ? j : bj;
  bj = -rl4co::bfly_i_max(-bj);
  if (lane == 0) ri[w] = bj;
  __syncthreads();
  bj = ri[0];
  for (int x = 1; x < kWaves; ++x) bj = ri[x] < bj ? ri[x] : bj;
  if (bj == kEmpty) bj = 0;  // (every reward NaN)
  if (!have_best || best_r <= M) {  // antsystem.py:238-245: equal rewards replace too
    best_r = M;
    const int64_t* src = actions + ((int64_t)bj * B + b) * T;
    for (int t = tid; t < T; t += kThreads) final_actions[(int64_t)b * T + t] = src[t];
    if (tid == 0) {
      final_reward[b] = M;
      if (final_iteration) final_iteration[b] = iteration_base + it;
    }
  }
  have_best = true;
  if (tid == 0 && final_reward_cache) final_reward_cache[(int64_t)it * B + b] = best_r;

  for (int e = tid; e < NN; e += kThreads) Lm[e] = 0.0f;  // delta, in the logits' storage
  __syncthreads();
  const float span = M - m;
  for (int j = 0; j < A; ++j) {
    const float r = reward[(int64_t)j * B + b];
    const float x = (r - m) / span;  // NOT guarded: M == m gives NaN as in the reference
    const float v = (x * x) * Q;
    const int64_t* act = actions + ((int64_t)j * B + b) * T;
    for (int t = tid; t < T - 1; t += kThreads) {
      const int from = (int)act[t], to = (int)act[t + 1];
      if (SkipDepotLoop && (from | to) == 0) continue;  // delta[0][0] = 0: the trailing zeros deposit nothing
      const int e = from * N + to;
      Lm[e] = Lm[e] + v;
    }
    __syncthreads();  // ant j is deposited before ant j + 1: every edge's sum is in ant order
  }
  if constexpr (!SkipDepotLoop) {
    if (tid == 0) Lm[0] = 0.0f;
    __syncthreads();
  }
  for (int e = tid; e < NN; e += kThreads) {
    const float kept = Pm[e] * decay;
    Pm[e] = kept + Lm[e];
  }
  __syncthreads();
}

// ---- host side -------------------------------------------------------------------------------------------------------------
// the largest N at which lds_bytes(true, N), the kernel's dynamic LDS with L and the pheromone on chip, fits one CU
template <typename BytesFn>
inline int lds_nodes(BytesFn lds_bytes) {
  int n = kMaxNodes;
  while (n > 0 && lds_bytes(true, n) + kStaticLds > kCuLds) --n;
  return n;
}

// one workgroup per instance with `lds_bytes` of dynamic LDS; `grid` > 0: that many workgroups (a kernel that strides
// over the instances itself); `more`: the kernel's arguments behind `a` (the decode options)
template <auto Kernel, typename Args, typename... More>
int launch(const Args& a, int lds_bytes, hipStream_t stream, int grid = 0, const More&... more) {
  hipFuncAttributes fa;
  RL4CO_HIP_TRY(hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(Kernel)));
  RL4CO_REQUIRE((int64_t)fa.sharedSizeBytes <= kStaticLds);  // the budget behind *_lds_nodes() holds
  if (lds_bytes > 64 * 1024) {
    RL4CO_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      lds_bytes));
  }
  hipLaunchKernelGGL(Kernel, dim3(grid > 0 ? grid : a.B), dim3(kThreads), lds_bytes, stream, a, more...);
  RL4CO_HIP_TRY(hipGetLastError());
  return RL4CO_OK;
}

// the requirements rl4co_aco_tsp_args, rl4co_aco_cvrp_args and rl4co_aco_prize_args share
template <typename Args>
int require_common(const Args& a) {
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
  RL4CO_REQUIRE(a.forced_actions == nullptr || (sample && a.iterations == 1));
  RL4CO_REQUIRE(a.pheromone != nullptr);
  RL4CO_REQUIRE(a.actions != nullptr);
  RL4CO_REQUIRE(a.reward != nullptr);
  RL4CO_REQUIRE(!update || (a.final_reward != nullptr && a.final_actions != nullptr));
  RL4CO_REQUIRE(a.err != nullptr);
  return RL4CO_OK;
}

// rl4co_heatmap_decode_opts as every *_opts entry point takes it; `ln_noise`: the caller's noise (nullptr: none, the
// gradients)
inline int require_decode_opts(const rl4co_heatmap_decode_opts* o, const void* ln_noise) {
  RL4CO_REQUIRE(o != nullptr);
  RL4CO_REQUIRE(o->greedy == 0 || o->greedy == 1);
  RL4CO_REQUIRE(o->top_k >= 0);
  RL4CO_REQUIRE(o->top_p >= 0.0f && o->top_p <= 1.0f);
  RL4CO_REQUIRE(o->reserved0 == 0);
  RL4CO_REQUIRE(!(o->greedy != 0 && ln_noise != nullptr));  // greedy reads no noise: a caller's noise is a mistake
  return RL4CO_OK;
}

}  // namespace rl4co::aco

// am_decode.hip — fused AttentionModel decode step / persistent rollout for gfx950.
//
// One launch runs the whole autoregressive loop of every trajectory: per step it streams the
// trajectory's three folded cache planes (glimpse key, glimpse value, logit key; [N,128] each),
// keeps the feasibility mask / per-head scores / logits in LDS, reduces with DPP / permlane
// butterflies, selects the action (greedy, sampled or forced), updates the TSP / CVRP state and
// goes on to the next step — no host round trip, no inter-workgroup traffic (instances are
// independent), no weights (they were folded into the cache once per rollout, rl4co_amd/cache.py).
//
// Reference semantics restated (file:line in the reference checkout):
//   context / query      env_embeddings/context.py:105-149, zoo/am/decoder.py:128-140
//   pointer attention    nn/attention.py:274-320 (8 heads x 16, mask_inner, /sqrt(128))
//   logits -> logprobs   utils/decoding.py:138-188 (tanh clip, mask, temperature, log_softmax)
//   selection            utils/decoding.py:387-413,448-461
//   env transition       envs/routing/tsp/env.py:60-86, envs/routing/cvrp/env.py:66-96,126-136
//   loop                 models/common/constructive/base.py:226-238
//
// Masked nodes are never read. The reference computes scores, values and logits for all N nodes
// and then overwrites the infeasible ones with -inf (attention.py:306-312, decoding.py:174-178):
// their softmax weight is exactly 0 and their log-prob exactly -inf. With mask_inner and
// mask_logits both on (the defaults) a step therefore only needs the cache rows of the F
// currently feasible nodes: each step compacts them (ascending node index) into a list and the
// three passes walk that list — on a TSP rollout F = N - t, i.e. half the bytes and half the
// arithmetic of the reference's formulation, with bit-identical semantics (a skipped term is an
// exact +0). If either flag is off the list simply holds all N nodes.
//
// Arithmetic order — the parity contract, mirrored value-for-value by
// oracle/rollout_ref.c (every op is an IEEE fp32 add/mul/fma/div, -ffp-contract=off):
//   list        = feasible nodes ascending (or all nodes), c = position in the list, F = length
//   EPL = elements per lane per 16-byte load (4 fp32 / 8 bf16); a cache row is covered by
//   LPR = 128/EPL lanes, a head by LPH = 16/EPL lanes; list entry c belongs to row group c % G
//   (G = rows handled concurrently: 64/LPR per wave x waves per trajectory).
//   tree(x_0..x_{n-1}) = pairwise butterfly sum: tree(lo half) + tree(hi half).
//   q[d]        = ((ctx_first[first][d] + ctx_cur[cur][d]) + q_bias[d]) * 0.25   (TSP, i > 0)
//   score(c,h)  = tree over the head's LPH chunks of [fma chain over the chunk's EPL dims,
//                 ascending, from 0]
//   softmax     = m = max_c score ; p_c = exp(score_c - m) ; per row group g:
//                 l_g = sum p_c, o_g[d] = fma(p_c, v_c[d], o_g[d]) over its entries in ascending c ;
//                 heads[d] = tree_g(o_g[d]) * (1 / tree_g(l_g))
//   logit(c)    = tree over the row's LPR chunks of [fma chain over EPL dims] ; / fl(sqrt(128))
//   log_softmax = zmax = max ; s_k = sum over c = k, k+64, ... of exp(z_c - zmax) (k < 64) ;
//                 lse = log(tree_k(s_k)) ; lp_c = (z_c - zmax) - lse
//   argmax      = maximum key, lowest index on ties (greedy: key = lp ; sampling:
//                 key = exp(lp) / noise[node])
//   top-k/top-p = (utils/decoding.py:109-188, only when the arguments ask for it; topkp.h) on the z above, after the
//                 temperature: key(z) = order-preserving uint32 image of z ; e_c = exp(z_c - zmax) (the log-sum-exp's
//                 terms) ; mass(S) = tree_k(sum over c in S, c = k, k+64, ... of e_c) — one order, so monotone in S.
//                 top-k (0 < k < F): tau = largest key with #{key_c >= tau} >= k (32 counting passes) ; remove
//                 key_c < tau (ties at tau kept) ; removed: z = -inf, e = 0.
//                 top-p (0 < p < 1): order the entries by (z, c) ascending, A_c = mass(entries up to c), Z = mass(all),
//                 remove c iff A_c <= thr, thr = min((1 - p) * Z, Z - 1 ulp) (the maximum always stays): cut = largest key with mass(key < cut) <= thr (32 mass
//                 passes), then inside the tie group key == cut the largest list position lo with
//                 mass(key < cut or (key == cut, c <= lo)) <= thr (bisection, <= 13 passes) ; removed as above.
//                 lse = log(mass(kept)) (== the unfiltered lse when nothing is removed) ; removed entries: lp = -inf,
//                 sampling key = -inf
//   SDVRP       = (env_embeddings/dynamic.py:60-78, zoo/am/decoder.py:142-152) the reference adds Linear(1 -> 3 * 128)(d) to
//                 the glimpse key, the glimpse value and the logit key, d_j = remaining demand of node j (the depot's taken
//                 as 0). Rank one per node, so with (u_k, u_v, u_l' = W_out^T u_l) the batch-shared fp32 vectors:
//                 kq_h   = tree over the head's LPH chunks of [fma chain of q against u_k], once per step
//                 score  = fmaf(d_j, kq_h, score(c,h) above)
//                 pd_g   = fmaf(p_c, d_c, pd_g) per row group over its entries in ascending c
//                 heads[d] = fmaf(tree_g(pd_g), u_v[d], tree_g(o_g[d])) * (1 / tree_g(l_g))
//                 ul     = tree over the row's LPR chunks of [fma chain of heads against u_l'], once per step
//                 logit  = fmaf(d_j, ul, logit(c) above)
//                 With 16-bit planes the one-wave kernel keeps G = 16 row groups for this environment (one accumulator per
//                 load in flight: entry c -> load (c % 16) / 4, row c % 4; tree = butterfly over the 4 rows, then
//                 ((g0 + g1) + (g2 + g3)) over the loads) — the four-wave kernels' tree, so STREAM, LDS and WIDE agree bit
//                 for bit. State (sdvrp/env.py:56-123, one rounding each): delivered = min(d[a], cap - used) ;
//                 used = (used + delivered) * (a != 0) ; d[a] = d[a] - delivered ; done = no d_j > 0 ; customer j masked
//                 iff d_j == 0 or used >= cap ; depot masked iff cur == 0 and some customer is feasible. The list holds
//                 every feasible node every step (a customer comes back until it is served): no row cache.
//   MTSP        = (env_embeddings/context.py:246-280, envs/routing/mtsp/env.py:63-131) min-max multi-agent TSP. The context is
//                 W_ctx [h_cur ; W_dyn f] with f = (num_agents - agent_idx, current_length, max_subtour_length,
//                 |loc_cur - loc_0|); with g = W_ctx[:, 128:] W_dyn the batch-shared fp32 [4,128] table, per dim:
//                 q = (fmaf(g3, f3, fmaf(g2, f2, fmaf(g1, f1, fmaf(g0, f0, ctx_cur[cur])))) + q_bias) * 0.25 — elementwise,
//                 the same chain in every variant. Pass 2 keeps the SDVRP build's 16 row groups (16-bit planes), so STREAM,
//                 LDS and WIDE agree bit for bit. State, one rounding each, dist = sqrt(fma(dy, dy, dx * dx)) as OP:
//                 avail[a] = 0 ; avail[0] = a != 0 and agent_idx < num_agents - 1 ; done = no customer available ;
//                 avail[0] |= done ; len = len + dist(a, prev) ; if done: len = len + dist(a, depot) ;
//                 max = len > max ? len : max ; agent_idx += (a == 0) ; len = len * (a != 0). The trajectory ends AT done.
#include <hip/hip_runtime.h>

#include "common.h"
#include "decode_wave.h"
#include "env_table.h"
#include "rl4co_math.h"
#include "topkp.h"

namespace {

constexpr int kLdsWaves = 4;    // four-wave kernels (LDS / WIDE, below): waves per trajectory
constexpr int kLdsGroups = 16;  // ... and their row groups

// The folded context tables of one instance, EPL dims from e0 on, as fp32: dense fp32 [N,128] rows (the default), or — r06,
// ctx_dtype — rows in the planes' 16-bit element type with the caller's strides (e.g. column blocks of the one 16-bit
// matrix the fused cache fold writes), widened exactly on load: the arithmetic downstream is that of the fp32 tables, so
// the specified-order oracle, given the widened values, still equals the kernel bit for bit.
template <class C>
struct CtxTables {
  const char *cur, *first;
  int64_t rs;  // bytes between node rows
  int late;    // bytes added at every load (`late_e0`: the lane's first dim when e0 is passed as 0 to keep cur / first wave-uniform)
  bool half;
  __device__ inline CtxTables(const rl4co_am_decode_args& a, int cb, int N, int e0, int late_e0 = 0) {
    half = a.ctx_dtype != RL4CO_DT_F32;
    const int64_t esz = half ? 2 : 4;
    late = late_e0 * (int)esz;
    rs = (a.ctx_row_stride ? a.ctx_row_stride : (int64_t)kD) * esz;
    const int64_t off = ((int64_t)cb * (a.ctx_batch_stride ? a.ctx_batch_stride : (int64_t)N * kD) + e0) * esz;
    cur = a.ctx_cur ? static_cast<const char*>(a.ctx_cur) + off : nullptr;
    first = a.ctx_first ? static_cast<const char*>(a.ctx_first) + off : nullptr;
  }
  __device__ inline void load(const char* table, int64_t row, float (&v)[C::EPL]) const {
    const char* p = table + row * rs + late;
    if constexpr (sizeof(typename C::elem) == 2) {
      if (half) {
        C::cvt(C::ld(reinterpret_cast<const typename C::elem*>(p)), v);
        return;
      }
    }
#pragma unroll
    for (int e = 0; e < C::EPL; ++e) v[e] = reinterpret_cast<const float*>(p)[e];
  }
};

// blockIdx -> trajectory. Trajectories are stored s-major (row r = s * B_inst + instance, the
// reference's batchify layout) and the S trajectories of an instance stream the SAME cache planes.
// Workgroup b is dispatched to XCD b % 8 (observed placement, used for speed only), and each XCD
// has its own L2 — so consecutive workgroups of one XCD are given the S starts of one instance:
// they run concurrently on that XCD and all but the first touch of a plane row hit its L2.
__device__ inline int trajectory_of_block(int b, int B, int B_inst) {
  const int S = B / B_inst;
  if (S == 1 || (B_inst & 7) != 0) return b;
  const int xcd = b & 7, k = b >> 3;
  return (k % S) * B_inst + (k / S) * 8 + xcd;
}

template <int ENV>
__device__ inline int commit_and_step(const rl4co_am_decode_args& a, TrajState& st, float* lg, const uint16_t* fl, int F,
                                      uint8_t* mk, uint8_t* vis, const float* dem, float cap, int r, int t, int N, int lane,
                                      const float* oplocs, const float* opmax, const float* twdur, int bc, float* dd = nullptr);

// One wave: raw logits lg[0..F) (list order) -> log-probs, selection, outputs, environment
// transition on the LDS-resident mask. Returns the action; st is updated (incl. done).
// FILT: the top-k / top-p filter instantiation (launched only when the arguments ask for it, so that the kernels without it
// keep their registers); `xs`: 2 N floats of scratch (the score block, dead after pass 2), read only by the filter.
template <int ENV, bool FILT = false>
__device__ inline int finalize_and_step(const rl4co_am_decode_args& a, TrajState& st, float* lg, float* xs,
                                        const uint16_t* fl, int F, uint8_t* mk, uint8_t* vis, const float* dem, float cap,
                                        int r, int t, int N, int lane, const float* oplocs = nullptr,
                                        const float* opmax = nullptr, const float* twdur = nullptr, float* dd = nullptr) {
  bool nan_seen = false;
  float zmax = kNegInf;
  for (int c = lane; c < F; c += 64) {
    float z = lg[c] / kSqrtD;
    if (z != z) nan_seen = true;  // attention.py:295-296
    if (a.tanh_clipping > 0.0f) z = rl4co_tanhf(z) * a.tanh_clipping;
    if (a.mask_logits && mk[fl[c]] == 0) z = kNegInf;
    if (a.temperature != 1.0f) z = z / a.temperature;  // x / 1.0f == x exactly
    lg[c] = z;
    zmax = fmaxf(zmax, z);
  }
  if (__any(nan_seen)) st.errbits |= RL4CO_EBIT_NAN_LOGIT;
  zmax = rl4co::bfly_max<1, 64>(zmax);
  float zsum = 0.0f;
  const int64_t tcol = (int64_t)a.t0 + t;
  constexpr bool filt = FILT;
  if (filt) {  // top-k / top-p: the same terms staged, removed entries -> z = -inf, e = 0; zsum over the kept ones
    for (int c = lane; c < F; c += 64) xs[c] = rl4co_expf(lg[c] - zmax);
    zsum = rl4co::topkp_filter(lg, xs, F, a.top_k, a.top_p, lane);
    if (a.kept_bits)
      rl4co::topkp_write_bits(a.kept_bits + ((int64_t)r * a.out_stride + tcol) * a.kept_words, a.kept_words, lg, fl, F,
                              N, reinterpret_cast<uint32_t*>(xs + N), lane);
  } else {
    for (int c = lane; c < F; c += 64) zsum = zsum + rl4co_expf(lg[c] - zmax);
    zsum = rl4co::bfly_sum<1, 64>(zsum);
  }
  const float lse = rl4co_logf(zsum);

  float best = kNegInf;
  int bc = 0x7fffffff;  // best list position
  float ent = 0.0f;
  float* alp = a.all_logps ? a.all_logps + ((int64_t)r * a.out_stride + tcol) * N : nullptr;
  if (alp && F < N) {  // nodes outside the list have log-prob -inf
    for (int j = lane; j < N; j += 64)
      if (mk[j] == 0) alp[j] = kNegInf;
  }
  for (int c = lane; c < F; c += 64) {
    const int j = fl[c];
    const float lp = (lg[c] - zmax) - lse;
    lg[c] = lp;
    float key = lp;
    if (a.mode == RL4CO_DECODE_SAMPLE) {
      const float nz = a.exp_noise
                           ? a.exp_noise[((int64_t)t * a.B + r) * N + j]
                           : rl4co_exp1_noise(a.philox_seed ^ (a.philox_seed_dev ? *a.philox_seed_dev : 0ull),
                                              a.philox_offset + (uint64_t)tcol, (uint32_t)r,
                                              (uint32_t)j);
      key = rl4co_expf(lp) / nz;  // multinomial(p,1) == argmax(p / Exp(1))
      if (filt && !(lp > kNegInf)) key = kNegInf;  // a removed entry is never drawn, even if every kept key underflows
    }
    if (bc == 0x7fffffff || key > best) {  // strict '>' keeps the lowest index on ties
      best = key;
      bc = c;
    }
    if (a.entropy && lp > kNegInf) ent = fmaf(rl4co_expf(lp), lp, ent);
    if (alp) alp[j] = lp;
  }
  rl4co::bfly_argmax(best, bc);
  if (a.entropy) st.ent_acc = st.ent_acc - rl4co::bfly_sum<1, 64>(ent);
  rl4co::lds_barrier_wave();
  return commit_and_step<ENV>(a, st, lg, fl, F, mk, vis, dem, cap, r, t, N, lane, oplocs, opmax, twdur, bc, dd);
}

// One wave: lg[0..F) hold the step's log-probs (list order) and `bc` the selected list position. Evaluate-mode lookup,
// outputs, environment transition on the LDS-resident mask. Returns the action; st is updated (incl. done).
template <int ENV>
__device__ inline int commit_and_step(const rl4co_am_decode_args& a, TrajState& st, float* lg, const uint16_t* fl, int F,
                                      uint8_t* mk, uint8_t* vis, const float* dem, float cap, int r, int t, int N, int lane,
                                      const float* oplocs, const float* opmax, const float* twdur, int bc, float* dd) {
  const int64_t tcol = (int64_t)a.t0 + t;
  int bi;
  float logp;
  if (a.mode == RL4CO_DECODE_EVALUATE) {
    bi = (int)a.forced_actions[(int64_t)r * a.out_stride + tcol];
    if (bi < 0 || bi >= N) {  // forced action out of range
      st.errbits |= RL4CO_EBIT_INFEASIBLE;
      bi = 0;
    }
    // position of the forced node in the list (absent = masked out = log-prob -inf)
    int pos = 0x7fffffff;
    for (int c = lane; c < F; c += 64)
      if (fl[c] == bi) pos = c;
    pos = -rl4co::bfly_i_max(-pos);
    logp = pos < F ? lg[pos] : kNegInf;
  } else {
    bi = (bc < F) ? (int)fl[bc] : 0;
    logp = (bc < F) ? lg[bc] : kNegInf;
  }
  if (mk[bi] == 0) st.errbits |= RL4CO_EBIT_INFEASIBLE;            // decoding.py:393,409
  if (!(logp > -1000.0f)) st.errbits |= RL4CO_EBIT_NEG_INF_LOGP;   // decoding.py:56
  if (lane == 0) {
    a.actions[(int64_t)r * a.out_stride + tcol] = bi;
    a.logps[(int64_t)r * a.out_stride + tcol] = logp;
  }
  rl4co::lds_barrier_wave();

  // ---- environment transition -------------------------------------------------------
  if constexpr (ENV == RL4CO_ENV_MTSP) {  // (discarded in every other instantiation: their code is what it was)
    // min-max multi-agent TSP (mtsp/env.py:63-131); st.used = current_length, st.time = max_subtour_length, st.step_i =
    // agent_idx, oplocs = coordinates (depot row 0), mk = the reference's `available`
    const long long nag = a.num_agents[r % a.B_inst];
    const float px = oplocs[2 * st.cur], py = oplocs[2 * st.cur + 1];
    const float bx = oplocs[2 * bi], by = oplocs[2 * bi + 1];
    const bool depot_open = (bi != 0) && (st.step_i < nag - 1);  // mtsp/env.py:86-88 (agent_idx before the step)
    if (lane == 0) mk[bi] = 0;
    rl4co::lds_barrier_wave();
    bool left = false;
    for (int j = lane; j < N; j += 64) left |= (j >= 1) && mk[j] != 0;
    st.done = !__any(left);                                      // mtsp/env.py:91
    if (lane == 0) mk[0] = (depot_open || st.done) ? 1 : 0;      // mtsp/env.py:94
    float len;
    {
      const float dx = bx - px, dy = by - py;
      len = st.used + sqrtf(fmaf(dy, dy, dx * dx));              // mtsp/env.py:97
    }
    if (st.done) {
      const float dx = bx - oplocs[0], dy = by - oplocs[1];
      len = len + sqrtf(fmaf(dy, dy, dx * dx));                  // mtsp/env.py:100-102
    }
    st.time = len > st.time ? len : st.time;                     // mtsp/env.py:105-109
    st.step_i += (bi == 0) ? 1 : 0;                              // mtsp/env.py:77
    st.used = len * (bi != 0 ? 1.0f : 0.0f);                     // mtsp/env.py:112
    st.cur = bi;
  } else if (ENV == RL4CO_ENV_TSP) {
    if (st.step_i == 0) st.first = bi;  // tsp/env.py:63
    st.cur = bi;
    if (lane == 0) mk[bi] = 0;
    st.step_i += 1;
    rl4co::lds_barrier_wave();
    bool any_left = false;
    for (int j = lane; j < N; j += 64) any_left |= mk[j] != 0;
    st.done = !__any(any_left);  // tsp/env.py:71
  } else if (ENV == RL4CO_ENV_PDP) {
    // pickup and delivery (pdp/env.py:64-99); vis[j]: bit 0 = available, bit 1 = to_deliver
    const int n = N - 1;
    if (lane == 0) {
      vis[bi] &= (uint8_t)~1u;
      vis[(bi + n / 2) % (n + 1)] |= 2;
    }
    st.step_i += 1;
    st.cur = bi;
    rl4co::lds_barrier_wave();
    bool left = false;
    for (int j = lane; j < N; j += 64) {
      const uint8_t v = vis[j];
      mk[j] = (v == 3) ? 1 : 0;
      left |= (v & 1) != 0;
    }
    st.done = !__any(left);  // pdp/env.py:83
  } else if (ENV == RL4CO_ENV_SDVRP) {
    // split delivery (sdvrp/env.py:56-123); dd: the trajectory's remaining demands (depot column 0), in LDS
    const float da = dd[bi];
    const float delivered = fminf(da, cap - st.used);
    st.used = (st.used + delivered) * (bi != 0 ? 1.0f : 0.0f);
    st.cur = bi;
    rl4co::lds_barrier_wave();  // every lane has read dd[bi]
    if (lane == 0) dd[bi] = da - delivered;
    rl4co::lds_barrier_wave();
    bool any_feasible = false, any_left = false;
    for (int j = lane; j < N; j += 64) {
      const float dj = dd[j];
      any_left |= dj > 0.0f;
      if (j >= 1) {
        const bool masked = (dj == 0.0f) || (st.used >= cap);
        mk[j] = masked ? 0 : 1;
        any_feasible |= !masked;
      }
    }
    any_feasible = __any(any_feasible);
    st.done = !__any(any_left);
    if (lane == 0) mk[0] = ((st.cur == 0) && any_feasible) ? 0 : 1;
  } else if (ENV == RL4CO_ENV_PCTSP) {
    // prize-collecting TSP (pctsp/env.py:62-91,141-148); st.used is the prize collected so far,
    // dem the real prize per node (depot column 0)
    st.used = st.used + dem[bi];
    if (lane == 0) vis[bi] = 1;
    st.done = (bi == 0) && (st.step_i > 0);
    st.step_i += 1;
    st.cur = bi;
    rl4co::lds_barrier_wave();
    const bool depot_visited = vis[0] != 0;
    bool unvisited = false;
    for (int j = lane; j < N; j += 64) {
      if (j >= 1) {
        mk[j] = (vis[j] != 0 || depot_visited) ? 0 : 1;
        unvisited |= vis[j] == 0;
      }
    }
    unvisited = __any(unvisited);
    if (lane == 0) mk[0] = ((st.used < 1.0f) && unvisited) ? 0 : 1;
  } else if (ENV == RL4CO_ENV_OP) {
    // orienteering (op/env.py:67-98,137-154); st.used is the tour length, distances as in the
    // tour-length kernel: sqrt(fma(dy, dy, dx * dx))
    const float cx = oplocs[2 * st.cur], cy = oplocs[2 * st.cur + 1];
    const float bx = oplocs[2 * bi], by = oplocs[2 * bi + 1];
    {
      const float dx = bx - cx, dy = by - cy;
      st.used = st.used + sqrtf(fmaf(dy, dy, dx * dx));
    }
    if (lane == 0) vis[bi] = 1;
    st.done = (bi == 0) && (st.step_i > 0);
    st.step_i += 1;
    st.cur = bi;
    rl4co::lds_barrier_wave();
    const bool depot_visited = vis[0] != 0;
    for (int j = lane; j < N; j += 64) {
      const float dx = oplocs[2 * j] - bx, dy = oplocs[2 * j + 1] - by;
      const bool exceeds = st.used + sqrtf(fmaf(dy, dy, dx * dx)) > opmax[j];
      mk[j] = (j == 0 || !(vis[j] != 0 || depot_visited || exceeds)) ? 1 : 0;
    }
  } else {
    if (ENV == RL4CO_ENV_CVRPTW) {
      // cvrptw/env.py:97-113 (oplocs = coordinates, opmax = (start, end) windows, twdur = service times): the
      // clock advances by the distance from the node the vehicle stands on, waits for the window, serves
      const float dx = oplocs[2 * bi] - oplocs[2 * st.cur], dy = oplocs[2 * bi + 1] - oplocs[2 * st.cur + 1];
      const float served = fmaxf(st.time + sqrtf(fmaf(dy, dy, dx * dx)), opmax[2 * bi]) + twdur[bi];
      st.time = (bi != 0 ? 1.0f : 0.0f) * served;
    }
    const int di = min(max(bi - 1, 0), N - 2);                       // cvrp/env.py:71-73
    st.used = (st.used + dem[di]) * (bi != 0 ? 1.0f : 0.0f);         // cvrp/env.py:76
    st.cur = bi;
    if (lane == 0) vis[bi] = 1;
    rl4co::lds_barrier_wave();
    const float thr = cap + 1e-5f;  // cvrp/env.py:128
    bool any_feasible = false, all_visited = true;
    for (int j = lane; j < N; j += 64) {
      all_visited &= vis[j] != 0;
      if (j >= 1) {
        const bool masked = (vis[j] != 0) || (dem[j - 1] + st.used > thr);
        mk[j] = masked ? 0 : 1;
        any_feasible |= !masked;
      }
    }
    any_feasible = __any(any_feasible);
    st.done = __all(all_visited);  // cvrp/env.py:83
    if (lane == 0) mk[0] = ((st.cur == 0) && any_feasible) ? 0 : 1;  // cvrp/env.py:134-135
    if (ENV == RL4CO_ENV_CVRPTW) {  // cvrptw/env.py:91-95: only nodes whose window is still open on arrival
      rl4co::lds_barrier_wave();
      const float bx = oplocs[2 * bi], by = oplocs[2 * bi + 1];
      for (int j = lane; j < N; j += 64) {
        const float dx = oplocs[2 * j] - bx, dy = oplocs[2 * j + 1] - by;
        if (!(st.time + sqrtf(fmaf(dy, dy, dx * dx)) <= opmax[2 * j + 1])) mk[j] = 0;
      }
    }
  }
  rl4co::lds_barrier_wave();
  return bi;
}

// ================================================================================================
// Streaming kernel: ONE wavefront (= one 64-thread workgroup) per trajectory; with thousands of
// trajectories 16 independent waves per CU hide each other's latency chains and the kernel runs
// at the HBM / Infinity-Cache rate. kUnroll wave-wide 1 KiB loads in flight per pass.
// ================================================================================================
// UNFOLD (parity mode, TSP / CVRP): the context projection and project_out are per-step GEMVs in the reference's
// association — out[d] = fma chain over k ascending of Wt[k][d] * in[k], from 0 — with the input vector broadcast
// from LDS and the transposed weight rows read as 16-byte lanes (each lane produces the EPL dims it owns).
template <int EPL>
__device__ inline void gemv_t(float (&out)[EPL], const float* __restrict__ wt, const float* in_lds, int width, int e0) {
#pragma unroll
  for (int e = 0; e < EPL; ++e) out[e] = 0.0f;
  for (int k = 0; k < width; ++k) {
    const float c = in_lds[k];
#pragma unroll
    for (int e = 0; e < EPL; ++e) out[e] = fmaf(wt[(int64_t)k * kD + e0 + e], c, out[e]);
  }
}

// Row cache (TSP / CVRP, not UNFOLD): the LDS a workgroup may hold without lowering the CU's workgroup count keeps the
// three plane rows of S nodes. Resident are the S highest-index nodes that can still be listed (TSP: unvisited; CVRP:
// the depot and the unvisited customers; mask off: all nodes) — as the list is ascending and holds only such nodes,
// its resident entries are always its tail. When a resident node leaves (visited), its slot goes to the highest
// non-resident candidate, marked pending: the next step that lists that node reads its rows from HBM as it would
// anyway and writes them into the slot in the same passes; from then on they come from LDS. Only the load source
// differs — every lane walks the same list positions in the same order, so the arithmetic is untouched.
constexpr int kRowCacheNone = 0xFF;  // slot byte of a node that is not resident
__host__ __device__ inline int row_cache_bytes(int N, int S, int esz) {
  return S > 0 ? S * 3 * kD * esz + lds_pad(N) + S : 0;
}

// REG (RL4CO_VARIANT_STREAM_REG; 16-bit planes, TSP / CVRP, N <= kRegMaxN): a step's per-head scores never go to LDS. Pass 2
// walks the list positions of pass 1 with the same lanes — row group rg takes c = c0 + u RPL + rg in both — and a lane
// needs only its own head's value of an entry, so pass 1 keeps them in registers (both loops fully unrolled, the outer
// iterations behind wave-uniform c0 < F guards; the two lanes of a head hold half of an iteration's kUnroll values each:
// kRegIters x kUnroll / 2 registers), the head maximum is the butterfly's result in every lane, and pass 2 takes
// p = exp(score - max) from the register, the other lane's by one DPP move: the same function of the same inputs as the
// numerators STREAM stages, each evaluated once. Without the score block (Np x 32 bytes) the same 10 KiB hold 11 resident
// rows per trajectory at N = 100 instead of 6, and the two barriers around the staging leave the step. Not built with
// the top-k / top-p filter (FILT): that instantiation does not fit 128 VGPRs without scratch.
constexpr int kRegIters = 7;                              // outer iterations of a pass held in registers
constexpr int kRegMaxN = kRegIters * 4 * kUnroll;         // 112: 4 rows per load (16-bit planes) x kUnroll loads
// LDS of the REG layout before the row cache: lg | fl | mk | vis
__host__ __device__ inline int stream_reg_lds_bytes(int N) {
  const int Np = lds_pad(N);
  return Np * 4 + Np * 2 + Np + Np;
}

// (REG: the register allocator is held to the 128 VGPRs of four waves per SIMD — left alone it spends the next occupancy
// step's 168 on the held scores, and 4096 trajectories no longer fit the chip in one round)
template <class C, int ENV, bool UNFOLD = false, bool FILT = false, bool REG = false>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(REG ? 4 : 1))) am_decode_kernel(const rl4co_am_decode_args a, const int S) {
  constexpr int EPL = C::EPL;
  constexpr int LPR = kD / EPL;   // lanes per cache row
  constexpr int RPL = 64 / LPR;   // rows per wave-wide load (= row groups G)
  constexpr int LPH = kDH / EPL;  // lanes per head
  constexpr bool kRowCache = !UNFOLD && (ENV == RL4CO_ENV_TSP || ENV == RL4CO_ENV_CVRP);
  static_assert(!REG || (kRowCache && RPL == 4 && LPH == 2 && !FILT), "REG: 16-bit planes, TSP / CVRP, folded, no top-k / top-p");
  constexpr bool kDyn = ENV == RL4CO_ENV_SDVRP;            // dynamic embedding: d_j * (x . u) joins every dot product
  constexpr bool kMtsp = ENV == RL4CO_ENV_MTSP;            // four running scalars in the context, min-max state
  constexpr int NG = ((kDyn || kMtsp) && RPL == 4) ? kUnroll : 1;  // accumulator sets of pass 2 (SDVRP / MTSP, 16-bit planes: one per load)
  // the tree below spells out four loads of four rows: the four-wave kernels' 4 waves x 4 rows, entry c -> group c % 16
  static_assert(NG == 1 || (kUnroll == 4 && kLdsWaves == 4 && kLdsGroups == 16), "SDVRP: STREAM must keep the LDS / WIDE summation tree");
  using elem = typename C::elem;
  using raw_t = typename C::raw;

  extern __shared__ __align__(16) unsigned char smem[];
  const int lane = threadIdx.x;
  const int r = trajectory_of_block(blockIdx.x, a.B, a.B_inst);
  const int N = a.N;
  const int Np = lds_pad(N);
  float* sc = reinterpret_cast<float*>(smem);  // [Np*kH] per-head scores -> softmax numerators, (c*kH + h)
  float* lg = sc + (REG ? 0 : Np * kH);  // [Np] raw logits -> clipped logits -> log-probs (list order)
  float* mh = lg + Np;                         // [8] per-head score maxima
  uint16_t* fl = reinterpret_cast<uint16_t*>(mh + (REG ? 0 : kH));  // [Np] nodes this step reads, ascending
  // (REG: no score block and no mh — stream_reg_lds_bytes; `sc` is not used)
  uint8_t* mk = reinterpret_cast<uint8_t*>(fl + Np);    // [Np] 1 = feasible
  uint8_t* vis = mk + Np;                               // [Np] CVRP visited flags
  elem* rc = reinterpret_cast<elem*>(vis + Np);         // [S][3][128] row cache (16-byte aligned: 40 Np + 32 bytes in)
  uint8_t* rslot = reinterpret_cast<uint8_t*>(rc + S * 3 * kD);  // [Np] slot of each node, kRowCacheNone if not resident
  uint8_t* rpend = rslot + Np;                                    // [S] 1 = slot not filled yet
  float* dd = reinterpret_cast<float*>(vis + Np);                 // [Np] SDVRP (no row cache): remaining demands

  const int cb = r % a.B_inst;  // instance whose cache this trajectory reads
  const int rg = lane / LPR;    // row group inside a wave-wide load
  const int li = lane % LPR;    // lane position inside the row
  const int hd = li / LPH;      // head this lane contributes to
  const int e0 = li * EPL;      // first embedding dim held by this lane

  // (REG: the plane bases stay wave-uniform, in scalar registers; the lane's e0 joins at each load)
  constexpr bool kLateE0 = REG;
  const int pe0 = kLateE0 ? 0 : e0, le0 = kLateE0 ? e0 : 0;
  const elem* Kg = static_cast<const elem*>(a.glimpse_key) + (int64_t)cb * a.kvl_batch_stride + pe0;
  const elem* Vg = static_cast<const elem*>(a.glimpse_val) + (int64_t)cb * a.kvl_batch_stride + pe0;
  const elem* Kl = static_cast<const elem*>(a.logit_key) + (int64_t)cb * a.kvl_batch_stride + pe0;
  const int64_t rs = a.kvl_row_stride;
  const CtxTables<C> ctx(a, cb, N, pe0, le0);  // (UNFOLD: not read)
  const float* hrow = UNFOLD ? a.node_embed + (int64_t)cb * N * kD + e0 : nullptr;

  // ---- load the trajectory state ---------------------------------------------------
  uint8_t* gmask = a.action_mask + (int64_t)r * N;
  for (int j = lane; j < Np; j += 64) mk[j] = (j < N) ? gmask[j] : (uint8_t)0;
  constexpr bool kScalarCtx = ENV == RL4CO_ENV_CVRP || ENV == RL4CO_ENV_OP || ENV == RL4CO_ENV_PCTSP || ENV == RL4CO_ENV_CVRPTW || kDyn || kMtsp;
  constexpr bool kCvrpLike = ENV == RL4CO_ENV_CVRP || ENV == RL4CO_ENV_CVRPTW;
  if (ENV == RL4CO_ENV_PDP) {  // bit 0 = available, bit 1 = to_deliver
    const uint8_t* gv = a.visited + (int64_t)r * N;
    const uint8_t* gt = a.to_deliver + (int64_t)r * N;
    for (int j = lane; j < Np; j += 64) vis[j] = (j < N) ? (uint8_t)((gv[j] != 0 ? 1 : 0) | (gt[j] != 0 ? 2 : 0)) : (uint8_t)0;
  } else if (kDyn) {
    const float* gd = a.demand_state + (int64_t)r * N;
    for (int j = lane; j < Np; j += 64) dd[j] = (j < N) ? gd[j] : 0.0f;
  } else if (ENV != RL4CO_ENV_TSP && !kMtsp) {  // (MTSP: the mask is the state, as in TSP)
    const uint8_t* gv = a.visited + (int64_t)r * N;
    for (int j = lane; j < Np; j += 64) vis[j] = (j < N) ? gv[j] : (uint8_t)1;
  }
  TrajState st;
  st.cur = (int)a.current_node[r];
  st.first = (ENV == RL4CO_ENV_TSP) ? (int)a.first_node[r] : 0;
  st.step_i = !(kCvrpLike || kDyn) ? a.step_i[r] : 0;
  st.time = (ENV == RL4CO_ENV_CVRPTW || kMtsp) ? a.current_time[r] : 0.0f;  // MTSP: max_subtour_length
  st.used = kScalarCtx ? a.used_capacity[r] : 0.0f;  // OP: tour length so far; MTSP: current_length
  st.done = a.done[r] != 0;
  st.errbits = 0;
  st.ent_acc = 0.0f;
  const float* oplocs = (ENV == RL4CO_ENV_OP || ENV == RL4CO_ENV_CVRPTW || kMtsp) ? a.locs + (int64_t)cb * N * 2 : nullptr;
  const float* opmax = (ENV == RL4CO_ENV_OP)       ? a.max_length + (int64_t)cb * N
                       : (ENV == RL4CO_ENV_CVRPTW) ? a.time_windows + (int64_t)cb * N * 2  // (start, end) per node
                                                   : nullptr;
  const float* twdur = (ENV == RL4CO_ENV_CVRPTW) ? a.durations + (int64_t)cb * N : nullptr;
  // the context scalar is cap - used in both depot environments (context.py:147-149, 211-213):
  // OP: longest tour that may still end at the depot (its row of the table) minus the tour so far
  // PCTSP: prize still to collect, clamped at 0 (context.py:184-198)
  const float cap = (kCvrpLike || ENV == RL4CO_ENV_PCTSP || kDyn) ? a.vehicle_capacity[r]
                                                                      : ((ENV == RL4CO_ENV_OP) ? opmax[0] : 0.0f);
  const float* dem = kCvrpLike                  ? a.demand + (int64_t)cb * (N - 1)
                     : (ENV == RL4CO_ENV_PCTSP) ? a.demand + (int64_t)cb * N
                                                : nullptr;
  rl4co::lds_barrier_wave();

  // ---- row cache: the S highest-index candidates, all pending --------------------------------
  const bool list_all = !(a.mask_inner && a.mask_logits);
  auto candidate = [&](int j) -> bool {  // can node j still be listed in a later step?
    return list_all || (ENV == RL4CO_ENV_TSP ? mk[j] != 0 : (j == 0 || vis[j] == 0));
  };
  const bool caching = kRowCache && S > 0;
  if (caching) {
    for (int j = lane; j < Np; j += 64) rslot[j] = (uint8_t)kRowCacheNone;
    rl4co::lds_barrier_wave();
    int k = 0;
    for (int j0 = N - 1; j0 >= 0 && k < S; j0 -= 64) {  // lane l takes node j0 - l: descending in lane order
      const int j = j0 - lane;
      const bool f = j >= 0 && candidate(j);
      const unsigned long long bal = __ballot(f);
      const int s = k + __popcll(bal & ((1ull << lane) - 1ull));
      if (f && s < S) {
        rslot[j] = (uint8_t)s;
        rpend[s] = 1;
      }
      k += __popcll(bal);
    }
    rl4co::lds_barrier_wave();
  }
  auto lds_row = [&](int j, int plane) -> const elem* { return rc + (rslot[j] * 3 + plane) * kD + e0; };
  auto fill_row = [&](int j, int plane, const raw_t& v) {  // a pending (or already filled) slot gets its row
    const int s = rslot[j];
    if (s != kRowCacheNone) *reinterpret_cast<raw_t*>(rc + (s * 3 + plane) * kD + e0) = v;
  };

  float qb[EPL];
  auto load_qb = [&]() {
#pragma unroll
    for (int e = 0; e < EPL; ++e) qb[e] = a.q_bias ? a.q_bias[(int64_t)cb * kD + e0 + e] : 0.0f;
  };
  if constexpr (!REG) load_qb();  // (REG reads it again every step, a cache hit, instead of holding 8 registers through the passes)

  const float* dynv = kDyn ? a.dyn_vectors + e0 : nullptr;  // (u_k, u_v, u_l') [3,128]: this lane's EPL dims of each
  const float* mg = kMtsp ? a.mtsp_ctx + e0 : nullptr;      // MTSP: g [4,128], this lane's EPL dims of each row
  const long long nag = kMtsp ? a.num_agents[cb] : 0;
  const bool single = a.max_steps == 1;
  int t = 0;
  int rows_read = 0;  // cache rows this trajectory streamed from HBM (x 3 planes): the launch's real HBM read volume

  for (; t < a.max_steps && (!st.done || single); ++t) {
    const int F = build_list(a, mk, fl, N, lane);
    // list positions [0, hend) are read from HBM, [hend, F) from the row cache; the HBM rows of [pbeg, hend) are also
    // written into their slots (the pending ones). Resident entries lie in the list's last S positions.
    int hend = F, pbeg = F;
    if (caching) {
      const int c_lo = max(F - S, 0);
      int last_hbm = c_lo - 1, first_pend = F;
      for (int c = c_lo + lane; c < F; c += 64) {
        const int s = rslot[fl[c]];
        const bool pend = s != kRowCacheNone && rpend[s] != 0;
        if (s == kRowCacheNone || pend) last_hbm = c;
        if (pend) first_pend = min(first_pend, c);
      }
      hend = rl4co::bfly_i_max(last_hbm) + 1;
      pbeg = -rl4co::bfly_i_max(-first_pend);
      if constexpr (REG) {  // wave-uniform: scalar registers
        hend = __builtin_amdgcn_readfirstlane(hend);
        pbeg = __builtin_amdgcn_readfirstlane(pbeg);
      }
    }
    rows_read += hend;

    // ---- query: folded context projection + graph context (decoder.py:128-140) ------
    float q[EPL];
    if constexpr (REG) load_qb();
    if constexpr (UNFOLD) {
      // context vector into LDS (the score buffer is dead between steps), then q = W_ctx . ctx + graph context
      float* cv = sc;
      if (rg == 0) {
        if (ENV == RL4CO_ENV_TSP) {
          const bool ph = st.step_i < 1;  // context.py:120-128 placeholder
#pragma unroll
          for (int e = 0; e < EPL; ++e) {
            cv[e0 + e] = ph ? a.w_placeholder[e0 + e] : hrow[(int64_t)st.first * kD + e];
            cv[kD + e0 + e] = ph ? a.w_placeholder[kD + e0 + e] : hrow[(int64_t)st.cur * kD + e];
          }
        } else {  // context.py:70-74,147-149: [h_cur ; cap - used]
#pragma unroll
          for (int e = 0; e < EPL; ++e) cv[e0 + e] = hrow[(int64_t)st.cur * kD + e];
          if (li == 0) cv[kD] = cap - st.used;
        }
      }
      rl4co::lds_barrier_wave();
      gemv_t<EPL>(q, a.w_ctx_t, cv, a.ctx_width, e0);
#pragma unroll
      for (int e = 0; e < EPL; ++e) q[e] = q[e] + qb[e];
      rl4co::lds_barrier_wave();  // cv is overwritten by this step's scores
    } else if constexpr (kMtsp) {  // context.py:246-280, folded: ctx_cur[cur] + sum_k f_k g_k
      const float f0 = (float)(nag - st.step_i);
      const float ddx = oplocs[2 * st.cur] - oplocs[0], ddy = oplocs[2 * st.cur + 1] - oplocs[1];
      const float f3 = sqrtf(fmaf(ddy, ddy, ddx * ddx));
      float cc[EPL];
      ctx.load(ctx.cur, st.cur, cc);
#pragma unroll
      for (int e = 0; e < EPL; ++e) {
        float v = fmaf(mg[e], f0, cc[e]);
        v = fmaf(mg[kD + e], st.used, v);
        v = fmaf(mg[2 * kD + e], st.time, v);
        v = fmaf(mg[3 * kD + e], f3, v);
        q[e] = v + qb[e];
      }
    } else if (ENV == RL4CO_ENV_TSP) {
      if (st.step_i < 1) {  // context.py:120 placeholder context
#pragma unroll
        for (int e = 0; e < EPL; ++e) q[e] = a.q_step0[e0 + e] + qb[e];
      } else {
        float cf[EPL], cc[EPL];
        ctx.load(ctx.first, st.first, cf);
        ctx.load(ctx.cur, st.cur, cc);
#pragma unroll
        for (int e = 0; e < EPL; ++e) q[e] = (cf[e] + cc[e]) + qb[e];
      }
    } else if (ENV == RL4CO_ENV_PDP) {  // context.py:232-243: the current node alone
      float cc[EPL];
      ctx.load(ctx.cur, st.cur, cc);
#pragma unroll
      for (int e = 0; e < EPL; ++e) q[e] = cc[e] + qb[e];
    } else {
      float rem = cap - st.used;  // context.py:147-149
      if (ENV == RL4CO_ENV_PCTSP && !(rem > 0.0f)) rem = 0.0f;
      float cc[EPL];
      ctx.load(ctx.cur, st.cur, cc);
#pragma unroll
      for (int e = 0; e < EPL; ++e) {
        float v = fmaf(a.w_cap[e0 + e], rem, cc[e]);
        if (ENV == RL4CO_ENV_CVRPTW) v = fmaf(a.w_time[e0 + e], st.time, v);  // context.py:152-166
        q[e] = v + qb[e];
      }
    }
#pragma unroll
    for (int e = 0; e < EPL; ++e) q[e] = q[e] * 0.25f;  // 1/sqrt(16), exact

    // ---- pass 1: per-head scores over the glimpse keys of the listed nodes -------------
    float m = kNegInf;
    float kq = 0.0f;  // SDVRP: q_h . u_k,h
    if constexpr (kDyn) {
#pragma unroll
      for (int e = 0; e < EPL; ++e) kq = fmaf(q[e], dynv[e], kq);
      kq = rl4co::bfly_sum<1, LPH>(kq);
    }
    auto score = [&](const raw_t& rw, int c, int j) {  // j < 0: no entry (a no-op)
      const bool valid = j >= 0;
      float k[EPL];
      C::cvt(rw, k);
      float acc = 0.0f;
#pragma unroll
      for (int e = 0; e < EPL; ++e) acc = fmaf(q[e], k[e], acc);
      acc = rl4co::bfly_sum<1, LPH>(acc);
      if constexpr (kDyn) acc = fmaf(j > 0 ? dd[j] : 0.0f, kq, acc);
      const bool feas = valid && (!a.mask_inner || mk[valid ? j : 0] != 0);
      const float sv = feas ? acc : kNegInf;
      if constexpr (!REG) {
        if (valid && (li % LPH) == 0) sc[c * kH + hd] = sv;
      }
      m = fmaxf(m, sv);
      return sv;
    };
    // REG: the scores of the entries this lane's row group owns, of the lane's own head. The two lanes of a head hold the
    // same values, so each keeps half: the first lane those of loads 0 and 1, the second those of loads 2 and 3
    constexpr int kHeld = kUnroll / 2;
    [[maybe_unused]] float sreg[REG ? kRegIters : 1][kHeld];
    [[maybe_unused]] const bool second = (li % LPH) != 0;
    auto score_batch = [&](int c0, float (&keep)[kHeld]) {
      raw_t rw[kUnroll];
      int jj[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int c = c0 + u * RPL + rg;
        jj[u] = (c < F) ? (int)fl[c] : -1;
        rw[u] = (jj[u] < 0) ? C::zero() : (c < hend ? C::ld(Kg + (int64_t)jj[u] * rs + le0) : C::ld(lds_row(jj[u], 0)));
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int c = c0 + u * RPL + rg;
        if (caching && c >= pbeg && c < hend) fill_row(jj[u], 0, rw[u]);
        const float sv = score(rw[u], c, jj[u]);
        if constexpr (REG) keep[u % kHeld] = (u < kHeld || second) ? sv : keep[u % kHeld];
      }
    };
    if constexpr (REG) {
#pragma unroll
      for (int it = 0; it < kRegIters; ++it)
        if (it * RPL * kUnroll < F) score_batch(it * RPL * kUnroll, sreg[it]);
    } else {
      for (int c0 = 0; c0 < F; c0 += RPL * kUnroll) score_batch(c0, sreg[0]);
    }
    m = rl4co::bfly_max<LPR, 64>(m);  // (every lane: the maximum of its own head)
    if constexpr (!REG) {
      if (rg == 0 && (li % LPH) == 0) mh[hd] = m;
      rl4co::lds_barrier_wave();
      // softmax numerators once per (list entry, head) — lane-strided over the F*8 scores, so
      // each exp is evaluated exactly once (index % 8 = head is fixed per lane: 64 % 8 == 0)
      {
        const float mm = mh[lane & (kH - 1)];
        for (int idx = lane; idx < F * kH; idx += 64) sc[idx] = rl4co_expf(sc[idx] - mm);
      }
      rl4co::lds_barrier_wave();
    } else {
      // nothing passes through LDS here; but pass 2 must read its list entries again as STREAM does — carried over from
      // the unrolled pass 1 they would cost four more registers per held iteration
      asm volatile("" ::: "memory");
    }

    // ---- pass 2: softmax-weighted value sum ------------------------------------------------
    float lacc[NG], pdacc[NG];
    float oacc[NG][EPL];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      lacc[g] = 0.0f;
      pdacc[g] = 0.0f;
#pragma unroll
      for (int e = 0; e < EPL; ++e) oacc[g][e] = 0.0f;
    }
    auto accumulate = [&](const raw_t& rw, int c, bool ok, int g, float pr) {  // !ok: no entry (adds exact zeros)
      float v[EPL];
      C::cvt(rw, v);
      float p;
      if constexpr (REG) p = ok ? pr : 0.0f;  // pr: the entry's numerator, from the score held since pass 1
      else p = ok ? sc[c * kH + hd] : 0.0f;
      lacc[g] = lacc[g] + p;
      if constexpr (kDyn) {
        const int j = ok ? (int)fl[c] : 0;
        pdacc[g] = fmaf(p, j > 0 ? dd[j] : 0.0f, pdacc[g]);
      }
#pragma unroll
      for (int e = 0; e < EPL; ++e) oacc[g][e] = fmaf(p, v[e], oacc[g][e]);
    };
    auto value_batch = [&](int c0, const float (&kept)[kHeld]) {
      raw_t rw[kUnroll];
      bool ok[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int c = c0 + u * RPL + rg;
        ok[u] = c < F;
        rw[u] = !ok[u] ? C::zero() : (c < hend ? C::ld(Vg + (int64_t)fl[c] * rs + le0) : C::ld(lds_row(fl[c], 1)));
      }
      [[maybe_unused]] float pr[kUnroll];
      if constexpr (REG) {  // each numerator once per head: exp(score - max) by the lane that holds it, the other's by DPP
#pragma unroll
        for (int k = 0; k < kHeld; ++k) {
          const float own = rl4co_expf(kept[k] - m);
          const float other = rl4co::bfly_f<1>(own);
          pr[k] = second ? other : own;
          pr[kHeld + k] = second ? own : other;
        }
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int c = c0 + u * RPL + rg;
        if (caching && c >= pbeg && c < hend) fill_row(fl[c], 1, rw[u]);
        accumulate(rw[u], c, ok[u], NG > 1 ? u : 0, REG ? pr[u] : 0.0f);
      }
    };
    if constexpr (REG) {
#pragma unroll
      for (int it = 0; it < kRegIters; ++it)
        if (it * RPL * kUnroll < F) value_batch(it * RPL * kUnroll, sreg[it]);
    } else {
      for (int c0 = 0; c0 < F; c0 += RPL * kUnroll) value_batch(c0, sreg[0]);
    }
    // tree over the row groups: the butterfly over a load's rows, then (NG = 4) ((g0 + g1) + (g2 + g3)) over the loads
    auto tree = [&](auto&& term) -> float {
      if constexpr (NG == 1) {
        return rl4co::bfly_sum<LPR, 64>(term(0));
      } else {
        return (rl4co::bfly_sum<LPR, 64>(term(0)) + rl4co::bfly_sum<LPR, 64>(term(1))) +
               (rl4co::bfly_sum<LPR, 64>(term(2)) + rl4co::bfly_sum<LPR, 64>(term(3)));
      }
    };
    const float l = 1.0f / tree([&](int g) { return lacc[g]; });  // one IEEE division per step; heads = o * (1/l)
    float o[EPL];
    if constexpr (kDyn) {
      const float pd = tree([&](int g) { return pdacc[g]; });
#pragma unroll
      for (int e = 0; e < EPL; ++e) o[e] = fmaf(pd, dynv[kD + e], tree([&](int g) { return oacc[g][e]; })) * l;
    } else {
#pragma unroll
      for (int e = 0; e < EPL; ++e) o[e] = tree([&](int g) { return oacc[g][e]; }) * l;
    }
    if constexpr (UNFOLD) {  // glimpse = project_out(heads) (attention.py:287), heads broadcast through LDS
      rl4co::lds_barrier_wave();       // every lane is done with the softmax numerators in sc
      if (rg == 0) {
#pragma unroll
        for (int e = 0; e < EPL; ++e) sc[e0 + e] = o[e];
      }
      rl4co::lds_barrier_wave();
      gemv_t<EPL>(o, a.w_out_t, sc, kD, e0);
    }

    // ---- pass 3: pointer logits against the (project_out-folded) logit key -----------
    float ul = 0.0f;  // SDVRP: heads . u_l'
    if constexpr (kDyn) {
#pragma unroll
      for (int e = 0; e < EPL; ++e) ul = fmaf(o[e], dynv[2 * kD + e], ul);
      ul = rl4co::bfly_sum<1, LPR>(ul);
    }
    auto logit = [&](const raw_t& rw, int c) {
      float k[EPL];
      C::cvt(rw, k);
      float acc = 0.0f;
#pragma unroll
      for (int e = 0; e < EPL; ++e) acc = fmaf(o[e], k[e], acc);
      acc = rl4co::bfly_sum<1, LPR>(acc);
      if constexpr (kDyn) {
        const int j = c < F ? (int)fl[c] : 0;
        acc = fmaf(j > 0 ? dd[j] : 0.0f, ul, acc);
      }
      if (c < F && li == 0) lg[c] = acc;
    };
    for (int c0 = 0; c0 < F; c0 += RPL * kUnroll) {
      raw_t rw[kUnroll];
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int c = c0 + u * RPL + rg;
        rw[u] = (c >= F) ? C::zero() : (c < hend ? C::ld(Kl + (int64_t)fl[c] * rs + le0) : C::ld(lds_row(fl[c], 2)));
      }
#pragma unroll
      for (int u = 0; u < kUnroll; ++u) {
        const int c = c0 + u * RPL + rg;
        if (caching && c >= pbeg && c < hend) fill_row(fl[c], 2, rw[u]);
        logit(rw[u], c);
      }
    }
    if (caching) {
      // the slots of the listed pending nodes now hold all three rows
      for (int c = pbeg + lane; c < hend; c += 64) {
        const int s = rslot[fl[c]];
        if (s != kRowCacheNone) rpend[s] = 0;
      }
    }
    rl4co::lds_barrier_wave();

    const int bi = finalize_and_step<ENV, FILT>(a, st, lg, sc, fl, F, mk, vis, dem, cap, r, t, N, lane, oplocs, opmax, twdur, dd);
    if constexpr (REG) {  // the state is the same in every lane: held in scalar registers across the passes
      st.cur = __builtin_amdgcn_readfirstlane(st.cur);
      st.first = __builtin_amdgcn_readfirstlane(st.first);
      st.errbits = (uint32_t)__builtin_amdgcn_readfirstlane((int)st.errbits);
      st.used = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, st.used)));
      st.ent_acc = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, st.ent_acc)));
    }
    if (caching && rslot[bi] != kRowCacheNone && !candidate(bi)) {
      // the resident node left: its slot goes to the highest candidate not resident, which the next step that lists
      // it reads from HBM anyway
      int nxt = -1;
      for (int j = lane; j < N; j += 64)
        if (candidate(j) && rslot[j] == kRowCacheNone) nxt = j;
      nxt = rl4co::bfly_i_max(nxt);
      const int s = rslot[bi];
      rl4co::lds_barrier_wave();
      if (lane == 0) {
        rslot[bi] = (uint8_t)kRowCacheNone;
        if (nxt >= 0) {
          rslot[nxt] = (uint8_t)s;
          rpend[s] = 1;
        }
      }
      rl4co::lds_barrier_wave();
    }
  }
  if (!single && !st.done && t >= a.max_steps) st.errbits |= RL4CO_EBIT_MAX_STEPS;

  // ---- write the state back ------------------------------------------------------------
  for (int j = lane; j < N; j += 64) gmask[j] = mk[j];
  if (ENV == RL4CO_ENV_PDP) {
    uint8_t* gv = a.visited + (int64_t)r * N;
    uint8_t* gt = a.to_deliver + (int64_t)r * N;
    for (int j = lane; j < N; j += 64) {
      gv[j] = vis[j] & 1;
      gt[j] = (vis[j] >> 1) & 1;
    }
  } else if (kDyn) {
    float* gd = a.demand_state + (int64_t)r * N;
    for (int j = lane; j < N; j += 64) gd[j] = dd[j];
  } else if (ENV != RL4CO_ENV_TSP && !kMtsp) {
    uint8_t* gv = a.visited + (int64_t)r * N;
    for (int j = lane; j < N; j += 64) gv[j] = vis[j];
  }
  if (lane == 0) {
    a.current_node[r] = st.cur;
    a.done[r] = st.done ? 1 : 0;
    if (ENV == RL4CO_ENV_TSP) a.first_node[r] = st.first;
    if (!(kCvrpLike || kDyn)) a.step_i[r] = st.step_i;
    if (ENV == RL4CO_ENV_CVRPTW || kMtsp) a.current_time[r] = st.time;
    if (kScalarCtx) a.used_capacity[r] = st.used;
    if (a.n_steps) a.n_steps[r] = t;
    if (a.steps_summary) {
      atomicMax(a.steps_summary, t);
      atomicAdd(a.steps_summary + 1, t);
      atomicAdd(reinterpret_cast<unsigned long long*>(a.steps_summary + 2), (unsigned long long)rows_read);
    }
    if (a.entropy) a.entropy[r] += st.ent_acc;
    if (st.errbits) atomicOr(a.err, (int)st.errbits);
  }
}

// ================================================================================================
// Four waves per trajectory (bf16 planes), G = 16 row groups: list entry c -> wave (c % 16) / 4,
// row group c % 4; per-group partial sums in ascending c, then the pairwise tree — butterfly
// inside the wave, ((w0 + w1) + (w2 + w3)) across waves through LDS.
//   RESIDENT = true : "LDS-resident" — the three planes are copied into LDS ONCE per rollout and
//                     every step reads them from there (needs them to fit half a CU's LDS).
//                     Wins when there are too few trajectories to fill the chip with one wave
//                     each: 0.65 vs 1.34 ms at 256 trajectories, 1.5 vs 1.8 ms at 1024 (TSP-100);
//                     with thousands of trajectories only two fit per CU and the latency chain
//                     of a step is exposed (5.8 vs 4.4 ms at 4096), so auto picks it for B <= 1024.
//   RESIDENT = false: "wide" streaming — same structure reading the planes from HBM/L2 every
//                     step; for few trajectories whose planes do not fit LDS (CVRP-500 x 1024:
//                     4096 waves instead of 1024, 120 -> 61 us per step).
// ================================================================================================

// The first half of finalize_and_step for the four-wave kernels, bit for bit: the ELEMENTWISE work of a step's N logits
// — clip, the softmax exponentials, log-probs, the sampling keys with their Philox draws: ~200 VALU operations per node —
// is dealt over all 256 threads instead of leaving three waves idle behind wave 0, while every order-dependent reduction
// (the lane-strided sum of the exponentials and its butterfly, the entropy) is still taken by wave 0 in finalize_and_step's
// own order from the staged terms; maxima and the (key, lowest position) arg-max are exact in any order. `xs`: 2 nw + 16
// floats of scratch (the score block, dead between B3 and the next step). Returns the selected list position (wave 0).
template <int ENV, bool FILT = false>
__device__ inline int wide_scores(const rl4co_am_decode_args& a, TrajState& st, float* lg, const uint16_t* fl, int F,
                                  const uint8_t* mk, float* xs, int nw, int r, int t, int N, int tid) {
  constexpr int T = 64 * kLdsWaves;
  const int w = tid >> 6, lane = tid & 63;
  float* ex = xs;             // [nw] softmax exponentials, then sampling keys
  float* xw = xs + 2 * nw;    // [4] wave maxima | [4] NaN flags | [1] log-sum-exp
  bool nan_seen = false;
  float zmax = kNegInf;
  for (int c = tid; c < F; c += T) {
    float z = lg[c] / kSqrtD;
    if (z != z) nan_seen = true;  // attention.py:295-296
    if (a.tanh_clipping > 0.0f) z = rl4co_tanhf(z) * a.tanh_clipping;
    if (a.mask_logits && mk[fl[c]] == 0) z = kNegInf;
    if (a.temperature != 1.0f) z = z / a.temperature;  // x / 1.0f == x exactly
    lg[c] = z;
    zmax = fmaxf(zmax, z);
  }
  zmax = rl4co::bfly_max<1, 64>(zmax);
  const bool wave_nan = __any(nan_seen);
  if (lane == 0) {
    xw[w] = zmax;
    xw[4 + w] = wave_nan ? 1.0f : 0.0f;
  }
  __syncthreads();
  zmax = fmaxf(fmaxf(xw[0], xw[1]), fmaxf(xw[2], xw[3]));
  if ((xw[4] + xw[5]) + (xw[6] + xw[7]) != 0.0f) st.errbits |= RL4CO_EBIT_NAN_LOGIT;
  for (int c = tid; c < F; c += T) ex[c] = rl4co_expf(lg[c] - zmax);
  __syncthreads();
  const int64_t tcol = (int64_t)a.t0 + t;
  constexpr bool filt = FILT;
  if (w == 0) {
    float zsum = 0.0f;
    if (filt) {  // top-k / top-p over the staged terms (wave 0; the other waves wait at the barrier below)
      zsum = rl4co::topkp_filter(lg, ex, F, a.top_k, a.top_p, lane);
      if (a.kept_bits)
        rl4co::topkp_write_bits(a.kept_bits + ((int64_t)r * a.out_stride + tcol) * a.kept_words, a.kept_words, lg, fl,
                                F, N, reinterpret_cast<uint32_t*>(xw + 16), lane);
    } else {
      for (int c = lane; c < F; c += 64) zsum = zsum + ex[c];
      zsum = rl4co::bfly_sum<1, 64>(zsum);
    }
    if (lane == 0) xw[8] = rl4co_logf(zsum);
  }
  __syncthreads();
  const float lse = xw[8];
  float* alp = a.all_logps ? a.all_logps + ((int64_t)r * a.out_stride + tcol) * N : nullptr;
  if (alp && F < N) {  // nodes outside the list have log-prob -inf
    for (int j = tid; j < N; j += T)
      if (mk[j] == 0) alp[j] = kNegInf;
  }
  for (int c = tid; c < F; c += T) {
    const int j = fl[c];
    const float lp = (lg[c] - zmax) - lse;
    lg[c] = lp;
    float key = lp;
    if (a.mode == RL4CO_DECODE_SAMPLE) {
      const float nz = a.exp_noise
                           ? a.exp_noise[((int64_t)t * a.B + r) * N + j]
                           : rl4co_exp1_noise(a.philox_seed ^ (a.philox_seed_dev ? *a.philox_seed_dev : 0ull),
                                              a.philox_offset + (uint64_t)tcol, (uint32_t)r,
                                              (uint32_t)j);
      key = rl4co_expf(lp) / nz;  // multinomial(p,1) == argmax(p / Exp(1))
      if (filt && !(lp > kNegInf)) key = kNegInf;  // a removed entry is never drawn
    }
    ex[c] = key;
    if (alp) alp[j] = lp;
  }
  __syncthreads();
  int bc = 0x7fffffff;
  if (w == 0) {
    float best = kNegInf, ent = 0.0f;
    for (int c = lane; c < F; c += 64) {
      const float key = ex[c];
      if (bc == 0x7fffffff || key > best) {  // strict '>' keeps the lowest index on ties
        best = key;
        bc = c;
      }
      if (a.entropy) {
        const float lp = lg[c];
        if (lp > kNegInf) ent = fmaf(rl4co_expf(lp), lp, ent);
      }
    }
    rl4co::bfly_argmax(best, bc);
    if (a.entropy) st.ent_acc = st.ent_acc - rl4co::bfly_sum<1, 64>(ent);
    rl4co::lds_barrier_wave();
  }
  return bc;
}

__host__ __device__ inline int lds_variant_sc_rows(int N) { return N < 80 ? 80 : N; }
__host__ __device__ inline int wide_scratch_bytes(int N) {
  const int nw = (N + 3) & ~3;
  return lds_variant_sc_rows(N) * kH * 4 + nw * 4 + kLdsWaves * kH * 4 + 32 + 2 * nw + 2 * nw;
}
__host__ __device__ inline int lds_variant_bytes(int N) { return 3 * N * kD * 2 + wide_scratch_bytes(N); }
// SDVRP: the trajectory's remaining demands behind the four-wave kernels' scratch
__host__ __device__ inline int wide_dyn_bytes(int N, int env) { return env == RL4CO_ENV_SDVRP ? ((N + 3) & ~3) * 4 : 0; }

// Four workgroups per CU (<= 128 registers): CVRP-500 x 1024 is 1024 workgroups = exactly four per CU, ONE round. The half
// (fp16) builds took 130 - 138 registers under a bound of two — three per CU, so a quarter of the trajectories waited for
// a second round: 25.3 ms per C5 step against 19.9 with bf16 planes (r04).
template <int ENV, bool RESIDENT, class C = CacheBF16, bool FILT = false>  // C: CacheBF16 or CacheF16 (same 16-byte lanes)
__global__ void __launch_bounds__(64 * kLdsWaves, 4) am_decode_wide_kernel(const rl4co_am_decode_args a) {
  constexpr int EPL = 8, LPR = 16, LPH = 2;
  constexpr int U = 4;  // list entries per wave handled per unrolled block
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x;
  const int w = tid >> 6, lane = tid & 63;
  const int r = trajectory_of_block(blockIdx.x, a.B, a.B_inst);
  const int N = a.N;
  const int nw = (N + 3) & ~3;
  uint16_t* planes = reinterpret_cast<uint16_t*>(smem);             // [3][N][128] bf16 (RESIDENT only)
  float* sc = reinterpret_cast<float*>(planes + (RESIDENT ? 3 * N * kD : 0));  // [max(N,80)][8]; later o/l partials
  float* lg = sc + lds_variant_sc_rows(N) * kH;                     // [nw] logits -> log-probs (list order)
  float* mpart = lg + nw;                                           // [4][8] per-wave head maxima
  int* shi = reinterpret_cast<int*>(mpart + kLdsWaves * kH);        // [8] broadcast: action, done, F
  uint16_t* fl = reinterpret_cast<uint16_t*>(shi + 8);              // [nw] nodes this step reads
  uint8_t* mk = reinterpret_cast<uint8_t*>(fl + nw);                // [nw] 1 = feasible
  uint8_t* vis = mk + nw;                                           // [nw] CVRP visited
  float* dd = reinterpret_cast<float*>(vis + nw);                   // [nw] SDVRP: remaining demands
  constexpr bool kDyn = ENV == RL4CO_ENV_SDVRP;
  constexpr bool kMtsp = ENV == RL4CO_ENV_MTSP;

  const int cb = r % a.B_inst;
  const int rg = lane / LPR, li = lane % LPR, hd = li / LPH, e0 = li * EPL;
  const uint16_t *Kg, *Vg, *Kl;
  int64_t rs;
  if constexpr (RESIDENT) {
    Kg = planes + e0;
    Vg = planes + N * kD + e0;
    Kl = planes + 2 * N * kD + e0;
    rs = kD;
  } else {
    Kg = static_cast<const uint16_t*>(a.glimpse_key) + (int64_t)cb * a.kvl_batch_stride + e0;
    Vg = static_cast<const uint16_t*>(a.glimpse_val) + (int64_t)cb * a.kvl_batch_stride + e0;
    Kl = static_cast<const uint16_t*>(a.logit_key) + (int64_t)cb * a.kvl_batch_stride + e0;
    rs = a.kvl_row_stride;
  }
  const CtxTables<C> ctx(a, cb, N, e0);
  // o/l partial slots inside this wave's own (dead after pass 2) score chunks
  auto opart = [&](int wv, int d) -> float* { return sc + ((16 * (d >> 5) + 4 * wv) * kH) + (d & 31); };
  auto lpart = [&](int wv, int h) -> float* { return sc + ((16 * 4 + 4 * wv) * kH) + h; };
  auto pdpart = [&](int wv, int h) -> float* { return lpart(wv, h) + kH; };  // SDVRP: sum p_c d_c, the row behind

  // ---- planes HBM -> LDS, once per rollout (16-byte coalesced) --------------------------------
  if constexpr (RESIDENT) {
    const uint16_t* src[3] = {static_cast<const uint16_t*>(a.glimpse_key), static_cast<const uint16_t*>(a.glimpse_val),
                              static_cast<const uint16_t*>(a.logit_key)};
    const int chunks = N * (kD / 8);  // 16-byte chunks per plane
    for (int p = 0; p < 3; ++p) {
      const uint16_t* g = src[p] + (int64_t)cb * a.kvl_batch_stride;
      for (int c = tid; c < chunks; c += 64 * kLdsWaves) {
        const int row = c >> 4, col = (c & 15) * 8;
        *reinterpret_cast<uint4*>(planes + (p * N + row) * kD + col) =
            *reinterpret_cast<const uint4*>(g + (int64_t)row * a.kvl_row_stride + col);
      }
    }
  }
  // ---- trajectory state: the same six environments as the streaming kernel (wave 0 owns the transition, the other
  // waves receive the scalars it changes through LDS after every step) ----------------------------------------------
  constexpr bool kScalarCtx = ENV == RL4CO_ENV_CVRP || ENV == RL4CO_ENV_OP || ENV == RL4CO_ENV_PCTSP || ENV == RL4CO_ENV_CVRPTW || kDyn || kMtsp;
  constexpr bool kCvrpLike = ENV == RL4CO_ENV_CVRP || ENV == RL4CO_ENV_CVRPTW;
  uint8_t* gmask = a.action_mask + (int64_t)r * N;
  for (int j = tid; j < nw; j += 64 * kLdsWaves) mk[j] = (j < N) ? gmask[j] : (uint8_t)0;
  if (ENV == RL4CO_ENV_PDP) {  // bit 0 = available, bit 1 = to_deliver
    const uint8_t* gv = a.visited + (int64_t)r * N;
    const uint8_t* gt = a.to_deliver + (int64_t)r * N;
    for (int j = tid; j < nw; j += 64 * kLdsWaves)
      vis[j] = (j < N) ? (uint8_t)((gv[j] != 0 ? 1 : 0) | (gt[j] != 0 ? 2 : 0)) : (uint8_t)0;
  } else if (kDyn) {
    const float* gd = a.demand_state + (int64_t)r * N;
    for (int j = tid; j < nw; j += 64 * kLdsWaves) dd[j] = (j < N) ? gd[j] : 0.0f;
  } else if (ENV != RL4CO_ENV_TSP && !kMtsp) {
    const uint8_t* gv = a.visited + (int64_t)r * N;
    for (int j = tid; j < nw; j += 64 * kLdsWaves) vis[j] = (j < N) ? gv[j] : (uint8_t)1;
  }
  TrajState st;
  st.cur = (int)a.current_node[r];
  st.first = (ENV == RL4CO_ENV_TSP) ? (int)a.first_node[r] : 0;
  st.step_i = !(kCvrpLike || kDyn) ? a.step_i[r] : 0;
  st.time = (ENV == RL4CO_ENV_CVRPTW || kMtsp) ? a.current_time[r] : 0.0f;  // MTSP: max_subtour_length
  st.used = kScalarCtx ? a.used_capacity[r] : 0.0f;  // OP: tour length so far; PCTSP: prize collected
  st.done = a.done[r] != 0;
  st.errbits = 0;
  st.ent_acc = 0.0f;
  const float* oplocs = (ENV == RL4CO_ENV_OP || ENV == RL4CO_ENV_CVRPTW || kMtsp) ? a.locs + (int64_t)cb * N * 2 : nullptr;
  const float* opmax = (ENV == RL4CO_ENV_OP)       ? a.max_length + (int64_t)cb * N
                       : (ENV == RL4CO_ENV_CVRPTW) ? a.time_windows + (int64_t)cb * N * 2
                                                   : nullptr;
  const float* twdur = (ENV == RL4CO_ENV_CVRPTW) ? a.durations + (int64_t)cb * N : nullptr;
  const float cap = (kCvrpLike || ENV == RL4CO_ENV_PCTSP || kDyn) ? a.vehicle_capacity[r] : ((ENV == RL4CO_ENV_OP) ? opmax[0] : 0.0f);
  const float* dem = kCvrpLike                  ? a.demand + (int64_t)cb * (N - 1)
                     : (ENV == RL4CO_ENV_PCTSP) ? a.demand + (int64_t)cb * N
                                                : nullptr;
  __syncthreads();
  if (w == 0) {
    const int F0 = build_list(a, mk, fl, N, lane);
    if (lane == 0) shi[2] = F0;
  }
  __syncthreads();

  float qb[EPL];
#pragma unroll
  for (int e = 0; e < EPL; ++e) qb[e] = a.q_bias ? a.q_bias[(int64_t)cb * kD + e0 + e] : 0.0f;

  const float* dynv = kDyn ? a.dyn_vectors + e0 : nullptr;  // (u_k, u_v, u_l') [3,128]: this lane's EPL dims of each
  const float* mg = kMtsp ? a.mtsp_ctx + e0 : nullptr;      // MTSP: g [4,128], this lane's EPL dims of each row
  const long long nag = kMtsp ? a.num_agents[cb] : 0;
  const bool single = a.max_steps == 1;
  int t = 0;
  int rows_read = 0;

  for (; t < a.max_steps && (!st.done || single); ++t) {
    const int F = shi[2];
    rows_read += F;
    const int iters = (F + kLdsGroups - 1) / kLdsGroups;
    // ---- query ---------------------------------------------------------------------------------
    float q[EPL];
    if constexpr (kMtsp) {  // context.py:246-280, folded: ctx_cur[cur] + sum_k f_k g_k
      const float f0 = (float)(nag - st.step_i);
      const float ddx = oplocs[2 * st.cur] - oplocs[0], ddy = oplocs[2 * st.cur + 1] - oplocs[1];
      const float f3 = sqrtf(fmaf(ddy, ddy, ddx * ddx));
      float cc[EPL];
      ctx.load(ctx.cur, st.cur, cc);
#pragma unroll
      for (int e = 0; e < EPL; ++e) {
        float v = fmaf(mg[e], f0, cc[e]);
        v = fmaf(mg[kD + e], st.used, v);
        v = fmaf(mg[2 * kD + e], st.time, v);
        v = fmaf(mg[3 * kD + e], f3, v);
        q[e] = v + qb[e];
      }
    } else if (ENV == RL4CO_ENV_TSP) {
      if (st.step_i < 1) {
#pragma unroll
        for (int e = 0; e < EPL; ++e) q[e] = a.q_step0[e0 + e] + qb[e];
      } else {
        float cf[EPL], cc[EPL];
        ctx.load(ctx.first, st.first, cf);
        ctx.load(ctx.cur, st.cur, cc);
#pragma unroll
        for (int e = 0; e < EPL; ++e) q[e] = (cf[e] + cc[e]) + qb[e];
      }
    } else if (ENV == RL4CO_ENV_PDP) {  // context.py:232-243: the current node alone
      float cc[EPL];
      ctx.load(ctx.cur, st.cur, cc);
#pragma unroll
      for (int e = 0; e < EPL; ++e) q[e] = cc[e] + qb[e];
    } else {
      float rem = cap - st.used;  // context.py:147-149
      if (ENV == RL4CO_ENV_PCTSP && !(rem > 0.0f)) rem = 0.0f;
      float cc[EPL];
      ctx.load(ctx.cur, st.cur, cc);
#pragma unroll
      for (int e = 0; e < EPL; ++e) {
        float v = fmaf(a.w_cap[e0 + e], rem, cc[e]);
        if (ENV == RL4CO_ENV_CVRPTW) v = fmaf(a.w_time[e0 + e], st.time, v);  // context.py:152-166
        q[e] = v + qb[e];
      }
    }
#pragma unroll
    for (int e = 0; e < EPL; ++e) q[e] = q[e] * 0.25f;

    // ---- pass 1: scores of this wave's list entries ----------------------------------------------
    float m = kNegInf;
    float kq = 0.0f;  // SDVRP: q_h . u_k,h
    if constexpr (kDyn) {
#pragma unroll
      for (int e = 0; e < EPL; ++e) kq = fmaf(q[e], dynv[e], kq);
      kq = rl4co::bfly_sum<1, LPH>(kq);
    }
    for (int i0 = 0; i0 < iters; i0 += U) {
      uint4 rw[U];
      int jj[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int c = kLdsGroups * (i0 + u) + 4 * w + rg;
        jj[u] = (c < F) ? (int)fl[c] : -1;
        rw[u] = (jj[u] >= 0) ? *reinterpret_cast<const uint4*>(Kg + (int64_t)jj[u] * rs) : C::zero();
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int c = kLdsGroups * (i0 + u) + 4 * w + rg;
        const bool valid = jj[u] >= 0;
        float k[EPL];
        C::cvt(rw[u], k);
        float acc = 0.0f;
#pragma unroll
        for (int e = 0; e < EPL; ++e) acc = fmaf(q[e], k[e], acc);
        acc = rl4co::bfly_sum<1, LPH>(acc);
        if constexpr (kDyn) acc = fmaf(jj[u] > 0 ? dd[jj[u]] : 0.0f, kq, acc);
        const bool feas = valid && (!a.mask_inner || mk[valid ? jj[u] : 0] != 0);
        const float sv = feas ? acc : kNegInf;
        if (valid && (li & 1) == 0) sc[c * kH + hd] = sv;
        m = fmaxf(m, sv);
      }
    }
    m = rl4co::bfly_max<LPR, 64>(m);
    if (rg == 0 && (li & 1) == 0) mpart[w * kH + hd] = m;
    __syncthreads();  // B1: all head maxima visible
    // softmax numerators of this wave's entries, each evaluated once (lane-strided over the
    // wave's 4-entry chunks: 32 consecutive floats per chunk, head = index % 8 fixed per lane)
    {
      const int hh = lane & (kH - 1);
      const float mm = fmaxf(fmaxf(mpart[hh], mpart[kH + hh]), fmaxf(mpart[2 * kH + hh], mpart[3 * kH + hh]));
      for (int tix = lane; tix < 32 * iters; tix += 64) {
        const int c0 = kLdsGroups * (tix >> 5) + 4 * w;  // first entry of the chunk
        if (c0 + ((tix & 31) >> 3) < F) {
          float* p = sc + c0 * kH + (tix & 31);
          *p = rl4co_expf(*p - mm);
        }
      }
    }
    rl4co::lds_barrier_wave();  // the numerators are consumed by this same wave only

    // ---- pass 2: softmax weights and weighted values ---------------------------------------------
    float l = 0.0f, pd = 0.0f;
    float o[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) o[e] = 0.0f;
    for (int i0 = 0; i0 < iters; i0 += U) {
      uint4 rw[U];
      bool ok[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int c = kLdsGroups * (i0 + u) + 4 * w + rg;
        ok[u] = c < F;
        rw[u] = ok[u] ? *reinterpret_cast<const uint4*>(Vg + (int64_t)fl[c] * rs) : C::zero();
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int c = kLdsGroups * (i0 + u) + 4 * w + rg;
        float v[EPL];
        C::cvt(rw[u], v);
        const float p = ok[u] ? sc[c * kH + hd] : 0.0f;
        l = l + p;
        if constexpr (kDyn) {
          const int j = ok[u] ? (int)fl[c] : 0;
          pd = fmaf(p, j > 0 ? dd[j] : 0.0f, pd);
        }
#pragma unroll
        for (int e = 0; e < EPL; ++e) o[e] = fmaf(p, v[e], o[e]);
      }
    }
    l = rl4co::bfly_sum<LPR, 64>(l);
    if constexpr (kDyn) pd = rl4co::bfly_sum<LPR, 64>(pd);
#pragma unroll
    for (int e = 0; e < EPL; ++e) o[e] = rl4co::bfly_sum<LPR, 64>(o[e]);
    if (rg == 0) {
#pragma unroll
      for (int e = 0; e < EPL; ++e) *opart(w, e0 + e) = o[e];
      if ((li & 1) == 0) *lpart(w, hd) = l;
      if (kDyn && (li & 1) == 0) *pdpart(w, hd) = pd;
    }
    __syncthreads();  // B2: partials of the four waves visible
    l = 1.0f / ((*lpart(0, hd) + *lpart(1, hd)) + (*lpart(2, hd) + *lpart(3, hd)));
    if constexpr (kDyn) pd = (*pdpart(0, hd) + *pdpart(1, hd)) + (*pdpart(2, hd) + *pdpart(3, hd));
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
      const int d = e0 + e;
      const float os = (*opart(0, d) + *opart(1, d)) + (*opart(2, d) + *opart(3, d));
      o[e] = (kDyn ? fmaf(pd, dynv[kD + e], os) : os) * l;
    }
    float ul = 0.0f;  // SDVRP: heads . u_l'
    if constexpr (kDyn) {
#pragma unroll
      for (int e = 0; e < EPL; ++e) ul = fmaf(o[e], dynv[2 * kD + e], ul);
      ul = rl4co::bfly_sum<1, LPR>(ul);
    }

    // ---- pass 3: logits of this wave's list entries ---------------------------------------------------
    for (int i0 = 0; i0 < iters; i0 += U) {
      uint4 rw[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int c = kLdsGroups * (i0 + u) + 4 * w + rg;
        rw[u] = (c < F) ? *reinterpret_cast<const uint4*>(Kl + (int64_t)fl[c] * rs) : C::zero();
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int c = kLdsGroups * (i0 + u) + 4 * w + rg;
        float k[EPL];
        C::cvt(rw[u], k);
        float acc = 0.0f;
#pragma unroll
        for (int e = 0; e < EPL; ++e) acc = fmaf(o[e], k[e], acc);
        acc = rl4co::bfly_sum<1, LPR>(acc);
        if constexpr (kDyn) {
          const int j = c < F ? (int)fl[c] : 0;
          acc = fmaf(j > 0 ? dd[j] : 0.0f, ul, acc);
        }
        if (c < F && li == 0) lg[c] = acc;
      }
    }
    __syncthreads();  // B3: all logits visible

    // ---- all waves: clip, exponentials, log-probs, sampling keys; wave 0: the reductions, then the environment
    // transition and the next step's list -----------------------------------------------------------------
    const int bc = wide_scores<ENV, FILT>(a, st, lg, fl, F, mk, sc, nw, r, t, N, tid);
    if (w == 0) {
      commit_and_step<ENV>(a, st, lg, fl, F, mk, vis, dem, cap, r, t, N, lane, oplocs, opmax, twdur, bc, dd);
      const int Fn = build_list(a, mk, fl, N, lane);
      if (lane == 0) {  // the scalars the next query is built from, for the other three waves
        shi[0] = st.cur;
        shi[1] = st.done ? 1 : 0;
        shi[2] = Fn;
        shi[3] = st.first;
        shi[4] = (int)st.step_i;
        shi[5] = __float_as_int(st.used);
        shi[6] = __float_as_int(st.time);
      }
    }
    __syncthreads();  // B4: state scalars, mask and list visible to every wave
    if (w != 0) {
      st.cur = shi[0];
      st.done = shi[1] != 0;
      st.first = shi[3];
      st.step_i = shi[4];
      st.used = __int_as_float(shi[5]);
      st.time = __int_as_float(shi[6]);
    }
  }
  if (w == 0) {
    if (!single && !st.done && t >= a.max_steps) st.errbits |= RL4CO_EBIT_MAX_STEPS;
    for (int j = lane; j < N; j += 64) gmask[j] = mk[j];
    if (ENV == RL4CO_ENV_PDP) {
      uint8_t* gv = a.visited + (int64_t)r * N;
      uint8_t* gt = a.to_deliver + (int64_t)r * N;
      for (int j = lane; j < N; j += 64) {
        gv[j] = vis[j] & 1;
        gt[j] = (vis[j] >> 1) & 1;
      }
    } else if (kDyn) {
      float* gd = a.demand_state + (int64_t)r * N;
      for (int j = lane; j < N; j += 64) gd[j] = dd[j];
    } else if (ENV != RL4CO_ENV_TSP && !kMtsp) {
      uint8_t* gv = a.visited + (int64_t)r * N;
      for (int j = lane; j < N; j += 64) gv[j] = vis[j];
    }
    if (lane == 0) {
      a.current_node[r] = st.cur;
      a.done[r] = st.done ? 1 : 0;
      if (ENV == RL4CO_ENV_TSP) a.first_node[r] = st.first;
      if (!(kCvrpLike || kDyn)) a.step_i[r] = st.step_i;
      if (ENV == RL4CO_ENV_CVRPTW || kMtsp) a.current_time[r] = st.time;
      if (kScalarCtx) a.used_capacity[r] = st.used;
      if (a.n_steps) a.n_steps[r] = t;
      if (a.steps_summary) {
        atomicMax(a.steps_summary, t);
        atomicAdd(a.steps_summary + 1, t);
        atomicAdd(reinterpret_cast<unsigned long long*>(a.steps_summary + 2), (unsigned long long)(RESIDENT ? 0 : rows_read));  // resident planes are read once per rollout
      }
      if (a.entropy) a.entropy[r] += st.ent_acc;
      if (st.errbits) atomicOr(a.err, (int)st.errbits);
    }
  }
}

using rl4co::EnvRecord;
using PlanesF32 = rl4co::Planes<RL4CO_DT_F32, CacheF32>;
using PlanesBF16 = rl4co::Planes<RL4CO_DT_BF16, CacheBF16>;
using PlanesF16 = rl4co::Planes<RL4CO_DT_F16, CacheF16>;

template <int ENV, bool RESIDENT, class C, bool FILT>
int launch_wide_f(const rl4co_am_decode_args& a, hipStream_t stream) {
  const int lds = (RESIDENT ? lds_variant_bytes(a.N) : wide_scratch_bytes(a.N)) + wide_dyn_bytes(a.N, ENV);
  if (lds > 64 * 1024) {
    RL4CO_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(am_decode_wide_kernel<ENV, RESIDENT, C, FILT>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  }
  hipLaunchKernelGGL((am_decode_wide_kernel<ENV, RESIDENT, C, FILT>), dim3(a.B), dim3(64 * kLdsWaves), lds, stream, a);
  RL4CO_HIP_TRY(hipGetLastError());
  return RL4CO_OK;
}
template <int ENV, class C>  // RL4CO_VARIANT_LDS (resident planes) / RL4CO_VARIANT_WIDE
int launch_wide(const rl4co_am_decode_args& a, bool resident, hipStream_t stream) {
  const bool filt = rl4co::topkp_on(a);
  if (resident) return filt ? launch_wide_f<ENV, true, C, true>(a, stream) : launch_wide_f<ENV, true, C, false>(a, stream);
  return filt ? launch_wide_f<ENV, false, C, true>(a, stream) : launch_wide_f<ENV, false, C, false>(a, stream);
}

// Which kernel serves these arguments (rules from measurements on MI355X, see the kernel headers; per environment:
// env_table.h).
inline int resolve_variant(const rl4co_am_decode_args& a) {
  const EnvRecord* env = rl4co::env_record(a.env);
  if (env == nullptr) return -1;
  // the unfolded parity mode exists in the streaming kernel only
  if (a.unfold) return (a.variant == RL4CO_VARIANT_AUTO || a.variant == RL4CO_VARIANT_STREAM) ? RL4CO_VARIANT_STREAM : -1;
  const bool f16 = a.cache_dtype == RL4CO_DT_F16;  // fp16 planes: every variant the bf16 planes have
  const bool bf16 = a.cache_dtype == RL4CO_DT_BF16 || f16;  // (16-bit planes)
  // multistart on the matrix cores (am_decode_ms.hip): 16-bit planes, N <= 128, plain outputs
  const bool ms_ok = bf16 && a.N <= 128 && a.B_inst > 0 && a.all_logps == nullptr && a.entropy == nullptr &&
                     !rl4co::topkp_on(a) &&  // the top-k / top-p filter is not in am_decode_ms.hip
                     env->ms;
  if (a.variant == RL4CO_VARIANT_MS) return ms_ok ? RL4CO_VARIANT_MS : -1;
  const bool fits = bf16 && lds_variant_bytes(a.N) + wide_dyn_bytes(a.N, a.env) <= 80 * 1024;
  const bool wide_ok = bf16 && wide_scratch_bytes(a.N) + wide_dyn_bytes(a.N, a.env) <= 64 * 1024;
  // STREAM with the step's scores in registers: 16-bit planes, the row-cache environments, N within its register array
  // (not with the top-k / top-p filter: its instantiation needs 2 to 5 registers past the 128 of four waves per SIMD)
  const bool reg_ok = bf16 && a.N <= kRegMaxN && env->stream_reg && !rl4co::topkp_on(a);
  if (a.variant == RL4CO_VARIANT_STREAM) return RL4CO_VARIANT_STREAM;
  if (a.variant == RL4CO_VARIANT_STREAM_REG) return reg_ok ? RL4CO_VARIANT_STREAM_REG : -1;
  if (a.variant == RL4CO_VARIANT_LDS) return fits ? RL4CO_VARIANT_LDS : -1;
  if (a.variant == RL4CO_VARIANT_WIDE) return wide_ok ? RL4CO_VARIANT_WIDE : -1;
  if (a.max_steps < 4) return RL4CO_VARIANT_STREAM;
  // auto: MS from the start count at which it was measured faster than one wave per trajectory (EnvRecord::ms_from)
  if (ms_ok && env->ms_from > 0 && a.B >= env->ms_from * a.B_inst) return RL4CO_VARIANT_MS;
  if (fits && a.B <= 1024) return RL4CO_VARIANT_LDS;
  // one wave per trajectory needs >= ~16 waves per CU to hide its latency chain: with fewer
  // trajectories than that, four waves per trajectory keep the memory pipes busier
  if (wide_ok && a.B <= 2048) return RL4CO_VARIANT_WIDE;
  return reg_ok ? RL4CO_VARIANT_STREAM_REG : RL4CO_VARIANT_STREAM;
}

// Workgroups of `bytes` LDS one CU holds, at most kStreamWgPerCu: the streaming kernel's register bound (<= 128 VGPRs,
// four waves per SIMD). The LDS allocation granule is taken as 512 B or 1280 B, whichever binds.
constexpr int kStreamWgPerCu = 16;
constexpr int kCuLds = 160 * 1024;
inline int stream_wg_per_cu(int bytes, int gran) {
  const int b = (bytes + gran - 1) / gran * gran;
  return min(kStreamWgPerCu, kCuLds / b);
}

// Row-cache slots of one streaming launch: the most for which the workgroups per CU stay what the scratch alone allows,
// capped at N and at 255 (the slot byte). 0 for single-step calls (nothing is reused), the parity mode and the
// environments whose "can still be listed" set is not kept (OP, PCTSP, PDP, CVRPTW). By default also 0 for fp32 planes:
// their 1536-byte rows leave room for 3 slots at N = 100, 5.9 % of the bytes, and the leg measured slower with them
// (DESIGN 4.1). RL4CO_DECODE_ROW_CACHE = n (read at every launch, so one process can compare) sets at most n slots, fp32
// planes included; 0 turns the cache off.
// `base`: the kernel's LDS without the cache (rl4co_am_decode_lds_bytes for STREAM, stream_reg_lds_bytes for STREAM_REG).
int row_cache_slots(const rl4co_am_decode_args& a, int esz, bool unfold, int base) {
  if (unfold || a.max_steps == 1 || !rl4co::env_served(a.env, &EnvRecord::row_cache)) return 0;  // (SDVRP: a visited node comes back)
  int S = 0;
  while (S < min(a.N, 255)) {
    const int bytes = base + row_cache_bytes(a.N, S + 1, esz);
    if (stream_wg_per_cu(bytes, 512) < stream_wg_per_cu(base, 512) ||
        stream_wg_per_cu(bytes, 1280) < stream_wg_per_cu(base, 1280) || bytes > kCuLds)
      break;
    ++S;
  }
  const char* e = getenv("RL4CO_DECODE_ROW_CACHE");
  if (e && e[0] != '\0') return min(S, max(atoi(e), 0));
  return esz == 4 ? 0 : S;
}

template <class C, int ENV, bool UNFOLD, bool FILT, bool REG = false>
int launch_f(const rl4co_am_decode_args& a, hipStream_t stream) {
  const int base = REG ? stream_reg_lds_bytes(a.N) : rl4co_am_decode_lds_bytes(a.N, ENV);
  const int S = row_cache_slots(a, (int)sizeof(typename C::elem), UNFOLD, base);
  const int lds = base + row_cache_bytes(a.N, S, (int)sizeof(typename C::elem));
  if (lds > 64 * 1024) {
    RL4CO_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(am_decode_kernel<C, ENV, UNFOLD, FILT, REG>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  }
  hipLaunchKernelGGL((am_decode_kernel<C, ENV, UNFOLD, FILT, REG>), dim3(a.B), dim3(64), lds, stream, a, S);
  RL4CO_HIP_TRY(hipGetLastError());
  return RL4CO_OK;
}
template <class C, int ENV, bool UNFOLD = false>
int launch(const rl4co_am_decode_args& a, hipStream_t stream) {
  return rl4co::topkp_on(a) ? launch_f<C, ENV, UNFOLD, true>(a, stream) : launch_f<C, ENV, UNFOLD, false>(a, stream);
}
template <class C, int ENV>  // RL4CO_VARIANT_STREAM_REG
int launch_reg(const rl4co_am_decode_args& a, hipStream_t stream) {
  return launch_f<C, ENV, false, false, true>(a, stream);
}

}  // namespace

extern "C" int rl4co_am_decode_lds_bytes(int N, int env) {
  const int Np = lds_pad(N);
  return Np * kH * 4 + Np * 4 + kH * 4 + Np * 2 + Np + Np + (env == RL4CO_ENV_SDVRP ? Np * 4 : 0);  // SDVRP: + the demands
}

extern "C" int rl4co_am_decode_row_groups(const rl4co_am_decode_args* args) {
  if (args == nullptr) return -1;
  const int v = resolve_variant(*args);
  if (v < 0) return -1;
  if (v == RL4CO_VARIANT_MS) return 0;  // bf16 MFMA variant: tolerance-tested, no specified-order oracle
  if (v == RL4CO_VARIANT_LDS || v == RL4CO_VARIANT_WIDE) return kLdsGroups;
  if (rl4co::env_served(args->env, &EnvRecord::one_acc16) && args->cache_dtype != RL4CO_DT_F32) return kLdsGroups;  // one accumulator per load
  return args->cache_dtype != RL4CO_DT_F32 ? 64 / (kD / CacheBF16::EPL) : 64 / (kD / CacheF32::EPL);
}

extern "C" int rl4co_am_decode_variant(const rl4co_am_decode_args* args) {
  return args == nullptr ? -1 : resolve_variant(*args);
}

extern "C" int rl4co_am_decode(const rl4co_am_decode_args* args, void* stream) {
  RL4CO_REQUIRE(args != nullptr);
  const rl4co_am_decode_args& a = *args;
  RL4CO_REQUIRE(rl4co::env_served(a.env, &EnvRecord::decode));
  RL4CO_REQUIRE(a.B > 0 && a.B_inst > 0 && a.B % a.B_inst == 0);
  RL4CO_REQUIRE(a.N >= 2 && a.N <= 4096);
  RL4CO_REQUIRE(a.max_steps >= 1);
  RL4CO_REQUIRE(a.mode >= RL4CO_DECODE_GREEDY && a.mode <= RL4CO_DECODE_EVALUATE);
  RL4CO_REQUIRE(a.cache_dtype == RL4CO_DT_F32 || a.cache_dtype == RL4CO_DT_BF16 || a.cache_dtype == RL4CO_DT_F16);
  RL4CO_REQUIRE(a.cache_dtype != RL4CO_DT_F16 || !a.unfold);
  RL4CO_REQUIRE(a.glimpse_key && a.glimpse_val && a.logit_key && (a.ctx_cur || a.unfold));
  RL4CO_REQUIRE(a.unfold == 0 || a.unfold == 1);
  // (r06) context tables in the planes' 16-bit type / with their own strides: 16-byte rows for the 8-dim lanes
  RL4CO_REQUIRE(a.ctx_dtype == RL4CO_DT_F32 || (a.ctx_dtype == a.cache_dtype && !a.unfold));
  RL4CO_REQUIRE(a.ctx_row_stride == 0 || (a.ctx_row_stride >= kD && a.ctx_row_stride % 8 == 0));
  RL4CO_REQUIRE(a.ctx_batch_stride == 0 || (a.ctx_batch_stride >= (int64_t)a.N * kD && a.ctx_batch_stride % 8 == 0));
  RL4CO_REQUIRE(a.ctx_dtype == RL4CO_DT_F32 || ((reinterpret_cast<uintptr_t>(a.ctx_cur) | reinterpret_cast<uintptr_t>(a.ctx_first)) & 15) == 0);
  if (a.unfold) {
    RL4CO_REQUIRE(rl4co::env_served(a.env, &EnvRecord::unfold));
    RL4CO_REQUIRE(a.node_embed && a.w_ctx_t && a.w_out_t);
    RL4CO_REQUIRE(a.ctx_width == (a.env == RL4CO_ENV_TSP ? 2 * kD : kD + 1));
    RL4CO_REQUIRE(a.env != RL4CO_ENV_TSP || a.w_placeholder);
  }
  RL4CO_REQUIRE(a.kvl_row_stride >= kD && a.kvl_row_stride % 8 == 0);
  RL4CO_REQUIRE(a.kvl_batch_stride >= (int64_t)a.N * kD && a.kvl_batch_stride % 8 == 0);
  RL4CO_REQUIRE(a.action_mask && a.current_node && a.done && a.actions && a.logps && a.err);
  RL4CO_REQUIRE(a.out_stride >= 1 && a.t0 >= 0 && (int64_t)a.t0 + a.max_steps <= a.out_stride);
  RL4CO_REQUIRE(a.temperature > 0.0f);
  RL4CO_REQUIRE((reinterpret_cast<uintptr_t>(a.steps_summary) & 7) == 0);  // [2..3] is one 64-bit counter
  RL4CO_REQUIRE(a.mode != RL4CO_DECODE_EVALUATE || a.forced_actions != nullptr);
  RL4CO_REQUIRE(a.top_p == a.top_p && a.top_p <= 1.0f);  // decoding.py:147 "top-p should be in (0, 1]."
  RL4CO_REQUIRE(a.kept_bits == nullptr || (a.kept_words >= (a.N + 31) / 32 && a.kept_words % 4 == 0 &&
                                           (reinterpret_cast<uintptr_t>(a.kept_bits) & 3) == 0));
  // the argument slots an environment needs (which state tensor rides in which slot: envspec.py)
  if (a.env == RL4CO_ENV_TSP) {
    RL4CO_REQUIRE(((a.ctx_first && a.q_step0) || a.unfold) && a.first_node && a.step_i);
  } else if (a.env == RL4CO_ENV_CVRP) {
    RL4CO_REQUIRE((a.w_cap || a.unfold) && a.demand && a.used_capacity && a.vehicle_capacity && a.visited);
  } else if (a.env == RL4CO_ENV_CVRPTW) {
    RL4CO_REQUIRE(a.w_cap && a.w_time && a.demand && a.used_capacity && a.vehicle_capacity && a.visited);
    RL4CO_REQUIRE(a.locs && a.time_windows && a.durations && a.current_time);
  } else if (a.env == RL4CO_ENV_SDVRP) {
    RL4CO_REQUIRE(a.w_cap && a.dyn_vectors && a.demand_state && a.used_capacity && a.vehicle_capacity);
    RL4CO_REQUIRE((reinterpret_cast<uintptr_t>(a.dyn_vectors) & 15) == 0);
  } else if (a.env == RL4CO_ENV_MTSP) {
    RL4CO_REQUIRE(a.mtsp_ctx && a.num_agents && a.locs && a.used_capacity && a.current_time && a.step_i);
  } else if (a.env == RL4CO_ENV_PDP) {
    RL4CO_REQUIRE(a.visited && a.to_deliver && a.step_i && (a.N - 1) % 2 == 0);
  } else if (a.env == RL4CO_ENV_PCTSP) {
    RL4CO_REQUIRE(a.w_cap && a.demand && a.used_capacity && a.vehicle_capacity && a.step_i && a.visited);
  } else {
    RL4CO_REQUIRE(a.w_cap && a.locs && a.max_length && a.used_capacity && a.step_i && a.visited);
  }
  RL4CO_REQUIRE(rl4co_am_decode_lds_bytes(a.N, a.env) <= 160 * 1024);
  RL4CO_REQUIRE(a.variant >= RL4CO_VARIANT_AUTO && a.variant <= RL4CO_VARIANT_STREAM_REG);
  const int variant = resolve_variant(a);
  RL4CO_REQUIRE(variant >= 0);  // explicit variant requested that cannot serve these planes
  hipStream_t s = rl4co::as_stream(stream);
  if (variant == RL4CO_VARIANT_MS) return a.cache_dtype == RL4CO_DT_F16 ? rl4co::launch_decode_ms_f16(a, s) : rl4co::launch_decode_ms(a, s);
  // the kernels of this file: plane type, then environment (the builds that exist: the column of env_table.h)
  if (a.unfold)
    return rl4co::dispatch_planes<PlanesF32, PlanesBF16>(a.cache_dtype, [&](auto p) {
      return rl4co::dispatch_env<&EnvRecord::unfold>(a.env, [&](auto e) { return launch<typename decltype(p)::type, decltype(e)::value, true>(a, s); });
    });
  if (variant == RL4CO_VARIANT_STREAM_REG)
    return rl4co::dispatch_planes<PlanesBF16, PlanesF16>(a.cache_dtype, [&](auto p) {
      return rl4co::dispatch_env<&EnvRecord::stream_reg>(a.env, [&](auto e) { return launch_reg<typename decltype(p)::type, decltype(e)::value>(a, s); });
    });
  if (variant == RL4CO_VARIANT_LDS || variant == RL4CO_VARIANT_WIDE)
    return rl4co::dispatch_planes<PlanesBF16, PlanesF16>(a.cache_dtype, [&](auto p) {
      return rl4co::dispatch_env<&EnvRecord::decode>(a.env, [&](auto e) {
        return launch_wide<decltype(e)::value, typename decltype(p)::type>(a, variant == RL4CO_VARIANT_LDS, s);
      });
    });
  return rl4co::dispatch_planes<PlanesF32, PlanesBF16, PlanesF16>(a.cache_dtype, [&](auto p) {
    return rl4co::dispatch_env<&EnvRecord::decode>(a.env, [&](auto e) { return launch<typename decltype(p)::type, decltype(e)::value>(a, s); });
  });
}

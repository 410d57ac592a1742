// aco_tsp_grad.hip — the backward of aco_tsp.hip's SAMPLE phase for DeepACO's training path (models/zoo/deepaco/policy.py:
// 138-163 through ConstructivePolicy.forward): the gradient of the ants' log-likelihoods with respect to the heatmap, fp32,
// one launch for gfx950.
//
// For the ant of row r = j * B + b with tour a_0 .. a_{N-1} and step t = 1 .. N - 1: i = a_{t-1}, F = the nodes not among
// a_0 .. a_{t-1}, p = softmax(heatmap[b, i, F] / temperature), g = grad_ll[r] + grad_steps[r, t], and for n in F
//   grad_heatmap[b, i, n] += g * ((n == a_t) - p_n) / temperature;   every other word is 0.
//
// The kernel owns the heatmap ROW, not the ant. A TSP ant stands on each node exactly once, so for a fixed row i ant j
// contributes exactly one masked softmax, the one of step t = pos_j[i] + 1, over F = {n : pos_j[n] > pos_j[i]} (pos_j: the
// inverse permutation of the ant's tour); the ant whose last node is i contributes nothing.
//   1  the workgroup compares every action of its instance with [0, N) (ant_system.h: check_indices), then builds
//      pos [n_ants, N] uint16: filled with 0xffff, scattered (pos[j][a_t] = t), and read back — a word still 0xffff means the
//      row is no permutation. Either refusal (RL4CO_EBIT_TOUR_INDEX, RL4CO_EBIT_INVALID_TOUR) is decided from one LDS word,
//      before anything is read through an action, and leaves the instance's gradient all zeros.
//   2  a wave takes rows i; lane l holds nodes l, l + 64, ... of row i (divided by the temperature once, the quotient
//      ant_step forms) and their accumulators in registers (KMAX = 1, 2, 4, 8 or 16 words per lane, N <= 64 KMAX), and loops
//      over the ants in ascending j: feasibility bits from pos_j, the log-softmax statistics in ant_step's own text
//      (ant_system.h: log_softmax_max, log_softmax_lse), p_n = rl4co_expf(lp_n) — the probabilities the forward's logps report — and
//      acc[n] = acc[n] + (g * ((n == a_t) - p_n)) / temperature (one multiply, one divide when temperature != 1, one add).
//      A step whose feasible logits are all -inf (the forward flagged it RL4CO_EBIT_INFEASIBLE) contributes nothing; a -inf
//      logit among finite ones has p = 0 and gradient 0.
//   3  the wave stores row i: every word of grad_heatmap is written exactly once, by one lane.
// No float atomics, no [N, N] accumulator: every output word is a sum in ascending ant order, so two launches give the same
// bits, and so does any split of an instance's rows over workgroups. Grid B x S: workgroup s of instance b takes the rows
// i = s (mod S), its four waves alternate over them; each of the S workgroups builds its own pos table.
// No barrier sits inside divergent control flow: the refusals are decided from one LDS word, the row loop has no barrier
// and every branch in it is wave-uniform (pos_j[i], the butterflied maximum).
//
// LDS budget (bytes, dynamic): 256 of scratch words + 2 * n_ants * N for pos while n_ants * N <= kPosLdsEntries = 16 384
// (32 KiB: 30 ants x 100 nodes take 6 000 B); above, pos lives in the caller's `pos_scratch` [B * S, n_ants, N] uint16 (a
// workgroup reads back only what it wrote itself). A non-NULL `pos_scratch` is used at any size.
// Design estimates, NOT measured: the 32 KiB bound (four workgroups' tables per CU) and the launcher-side choice of S (the
// binding aims at two workgroups per CU and at least sixteen rows per workgroup, since each workgroup repeats step 1) rest on
// no profile; nothing about this kernel's occupancy or speed has been measured beyond tools/aco_bench.py --train's
// end-to-end time.
#include <hip/hip_runtime.h>

#include "ant_grad.h"

namespace {

using namespace rl4co::aco;  // ant_system.h: the constants, check_indices, log_softmax_max / _lse, launch; ant_grad.h

constexpr int kPosLdsEntries = 16384;
constexpr uint16_t kNoPos = 0xffff;

// FILTER: each contribution runs over the kept set of its step under `o` (ant_system.h: filter_kept, the forward's text); false
// reads no `o` and is the kernel without it
template <int KMAX, bool LDS, bool FILTER>
__global__ void __launch_bounds__(kThreads) aco_tsp_grad_kernel(const rl4co_aco_tsp_grad_args a,
                                                                const rl4co_heatmap_decode_opts o) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int S = a.row_split, B = a.B, N = a.N, A = a.n_ants;
  int b, s;
  grad_split(S, b, s);
  const int64_t AN = (int64_t)A * N;
  uint16_t* pos = LDS ? reinterpret_cast<uint16_t*>(smem + kScratchBytes) : a.pos_scratch + (int64_t)blockIdx.x * AN;
  float* gout = a.grad_heatmap + (int64_t)b * N * N;

  // ---- 1. the refusals: indices, then permutations (both uniform: one LDS word) --------------------------------------------
  bool ok = check_indices(nullptr, 0, 1, a.actions, N, A, B, b, N, smem, a.err);
  if (ok) {  // (bad_flag is 0 here)
    for (int64_t e = tid; e < AN; e += kThreads) pos[e] = kNoPos;
    __syncthreads();
    for (int64_t e = tid; e < AN; e += kThreads) {
      const int64_t j = e / N;
      const int t = (int)(e - j * N);
      pos[j * N + a.actions[(j * B + b) * N + t]] = (uint16_t)t;  // (a repeated node: either step stays, another word stays empty)
    }
    __syncthreads();
    bool hole = false;
    for (int64_t e = tid; e < AN; e += kThreads) hole |= pos[e] == kNoPos;
    if (hole) *bad_flag(smem) = 1u;
    __syncthreads();
    ok = *bad_flag(smem) == 0u;
    if (!ok && tid == 0) atomicOr(a.err, RL4CO_EBIT_INVALID_TOUR);
  }
  if (!ok) {  // the instance's gradient is all zeros: this workgroup's rows
    grad_zero_rows(gout, N, s, S, w, lane);
    return;
  }

  // ---- 2. one wave, one row of the heatmap; the ants in ascending order ------------------------------------------------------
  const float temp = a.temperature;
  for (int i = s + S * w; i < N; i += S * kWaves) {
    const float* hrow = a.heatmap + ((int64_t)b * N + i) * N;
    float z[KMAX], acc[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      const int n = lane + 64 * k;
      float v = n < N ? hrow[n] : 0.0f;
      if (temp != 1.0f) v = v / temp;
      z[k] = v;
      acc[k] = 0.0f;
    }
    for (int j = 0; j < A; ++j) {
      const uint16_t* pj = pos + (int64_t)j * N;
      const int pi = pj[i];
      if (pi == N - 1) continue;  // (wave-uniform) the ant's last node: no step leaves it
      const int64_t row = (int64_t)j * B + b;
      float g = a.grad_ll[row];
      if (a.grad_steps) g = g + a.grad_steps[row * N + pi + 1];
      uint32_t feas = 0u, hit = 0u;  // bit k: node lane + 64 k is unvisited at that step / is the step's action
#pragma unroll
      for (int k = 0; k < KMAX; ++k) {
        const int n = lane + 64 * k;
        if (n < N) {
          const int pn = pj[n];
          feas |= (pn > pi ? 1u : 0u) << k;
          hit |= (pn == pi + 1 ? 1u : 0u) << k;
        }
      }
      if constexpr (FILTER) feas = filter_kept<KMAX>(z, feas, N, lane, o.top_k, o.top_p);  // removed nodes get 0
      const auto z_of = [&](int k, int) { return z[k]; };
      const auto feas_of = [&](int k) { return ((feas >> k) & 1u) != 0; };
      bool nan_seen;
      const float zmax = log_softmax_max(N, KMAX, lane, z_of, feas_of, nan_seen);
      if (!(zmax > kNegInf)) continue;  // (wave-uniform: a butterflied value) every feasible logit is -inf
      const float lse = log_softmax_lse(N, KMAX, lane, z_of, feas_of, zmax);
#pragma unroll
      for (int k = 0; k < KMAX; ++k) {
        if ((feas >> k) & 1u) {
          const float lp = (z[k] - zmax) - lse;
          const float p = rl4co_expf(lp);
          const float d = (((hit >> k) & 1u) ? 1.0f : 0.0f) - p;
          float c = g * d;
          if (temp != 1.0f) c = c / temp;
          acc[k] = acc[k] + c;
        }
      }
    }
    // ---- 3. the row ------------------------------------------------------------------------------------------------------
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      const int n = lane + 64 * k;
      if (n < N) gout[(int64_t)i * N + n] = acc[k];
    }
  }
}

template <bool LDS, bool FILTER>
int launch_grad(const rl4co_aco_tsp_grad_args& a, const rl4co_heatmap_decode_opts& o, int bytes, hipStream_t s) {
  return grad_ladder(a.N, [&](auto kmax) {
    return launch<aco_tsp_grad_kernel<decltype(kmax)::value, LDS, FILTER>>(a, bytes, s, a.B * a.row_split, o);
  });
}

}  // namespace

extern "C" int rl4co_aco_tsp_grad_lds_entries(void) { return kPosLdsEntries; }

extern "C" int rl4co_aco_tsp_logp_grad(const rl4co_aco_tsp_grad_args* args, void* stream) {
  const rl4co_heatmap_decode_opts off = {};
  return rl4co_aco_tsp_logp_grad_opts(args, &off, stream);
}

extern "C" int rl4co_aco_tsp_logp_grad_opts(const rl4co_aco_tsp_grad_args* args, const rl4co_heatmap_decode_opts* opts,
                                            void* stream) {
  RL4CO_REQUIRE(args != nullptr);
  const rl4co_aco_tsp_grad_args& a = *args;
  if (const int rc = require_decode_opts(opts, nullptr)) return rc;
  const rl4co_heatmap_decode_opts& o = *opts;  // (greedy is the forward's selector: nothing to differentiate)
  RL4CO_REQUIRE(a.B >= 1);
  RL4CO_REQUIRE(a.N >= 2 && a.N <= kMaxNodes);
  RL4CO_REQUIRE(a.n_ants >= 1);
  RL4CO_REQUIRE((int64_t)a.n_ants * a.B <= 2147483647LL);
  RL4CO_REQUIRE(a.row_split >= 1 && a.row_split <= a.N);
  RL4CO_REQUIRE((int64_t)a.B * a.row_split <= 2147483647LL);
  RL4CO_REQUIRE(a.temperature > 0.0f);
  RL4CO_REQUIRE(a.heatmap != nullptr && a.actions != nullptr && a.grad_ll != nullptr);
  RL4CO_REQUIRE(a.grad_heatmap != nullptr);
  RL4CO_REQUIRE(a.err != nullptr);
  const bool lds = a.pos_scratch == nullptr;
  RL4CO_REQUIRE(!lds || (int64_t)a.n_ants * a.N <= kPosLdsEntries);  // above, pos lives in the caller's scratch
  hipStream_t s = rl4co::as_stream(stream);
  const int bytes = lds ? kScratchBytes + 2 * a.n_ants * a.N : kScratchBytes;
  if (decode_filter_on(o)) return lds ? launch_grad<true, true>(a, o, bytes, s) : launch_grad<false, true>(a, o, bytes, s);
  return lds ? launch_grad<true, false>(a, o, bytes, s) : launch_grad<false, false>(a, o, bytes, s);
}

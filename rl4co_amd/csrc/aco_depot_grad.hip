// aco_depot_grad.hip — the backward of the SAMPLE phases of aco_cvrp.hip and aco_prize.hip for DeepACO's training path on the
// depot graphs (CVRP, OP, PCTSP): the gradient of the ants' log-likelihoods with respect to the heatmap, fp32, one launch for
// gfx950, one templated kernel with one instantiation per environment. aco_tsp_grad.hip's design with one more table.
//
// For the ant of row r = j * B + b with actions a_0 .. a_{len-1} (W wide, zero-filled after its length) and every step
// t < len: i = the node the ant leaves (the depot for t = 0, else a_{t-1}), F = the environment's feasible set at that step,
// p = softmax(heatmap[b, i, F] / temperature), g = grad_ll[r] + grad_steps[r, t], and for n in F
//   grad_heatmap[b, i, n] += g * ((n == a_t) - p_n) / temperature;   every other word is 0.
// With `multistart` (CVRP) column 0 is a given customer: it is stepped through the state and contributes nothing.
//
// The kernel owns the heatmap ROW, not the ant. A customer is visited at most once, so a customer's row is left at most once
// per ant: ant j contributes ONE masked softmax to row i, the one of step t = pos_j[i] + 1, over the customers n with
// pos_j[n] > pos_j[i] that pass the environment's test in the state the ant had when it stood on i, plus the depot where the
// rule allows it. Only the depot row is left several times: once per route for CVRP (t = 0 and every t with a_{t-1} == 0,
// state `used` = 0, over the customers with pos_j[n] >= t that fit an empty vehicle; the depot itself only when no customer
// is feasible, which has p = 1 and adds 0), once for OP and PCTSP (t = 0; OP's second departure after a depot taken at step
// 0 has the depot as its single feasible node and adds nothing).
//   1  the workgroup compares every action of its instance with [0, N) (ant_system.h: check_indices), loads the instance's
//      per-node vectors into LDS and replays each ant's row ONCE, a wave per ant, in the forward's own fp32 order
//      (ant_rules.h: the text the sampling kernels execute; the visited set is the forward's per-lane register mask). The
//      replay fills the table — pos[j][n] uint16, the step at which customer n is taken (0xffff: never); state[j][n] fp32, the
//      accumulator when the ant stands on n (CVRP used, OP tour_length, PCTSP cur_total_prize); len[j] — and decides the
//      refusals: RL4CO_EBIT_TOUR_INDEX (an action outside [0, N); a multistart start that is the depot),
//      RL4CO_EBIT_INVALID_TOUR (a customer taken twice; the rest of that row adds no further verdict),
//      RL4CO_EBIT_INFEASIBLE (a taken action that is infeasible under the environment's rule, or a row not done after W actions). The bits meet in ONE LDS word, read after a workgroup
//      barrier and before any gradient is written: a refused instance's gradient is all zeros, others are untouched.
//      CVRP's depot departures are not stored: the depot row's wave finds them in the actions, 64 steps per ballot.
//   2  a wave takes rows i; lane l holds nodes l, l + 64, ... of row i (divided by the temperature once) and their
//      accumulators in registers (KMAX = 1, 2, 4, 8 or 16 words per lane), loops over the ants in ascending j — the depot
//      row over each ant's departures in ascending t — with the log-softmax statistics in ant_step's own text
//      (log_softmax_max / log_softmax_lse), p_n = rl4co_expf(lp_n), acc[n] = acc[n] + (g * ((n == a_t) - p_n)) / temperature.
//      A step whose feasible logits are all -inf contributes nothing; a -inf logit among finite ones has p = 0.
//   3  the wave stores row i: every word of grad_heatmap is written exactly once, by one lane.
// No float atomics, no [N, N] accumulator: every output word is a sum in (ant, step) order held by one lane, so two launches,
// any row_split and either table tier give the same bits. The depot row stays with ONE wave (wave 0 of workgroup s = 0): no
// partial sums to combine. Grid B x S: workgroup s of instance b takes the rows i = s (mod S), its four waves alternate over
// them; each workgroup builds its own table. No barrier sits inside divergent control flow: the refusals are decided from
// one LDS word, the row loop has no barrier and every branch in it is wave-uniform (pos_j[i], len[j], ballots, butterflies).
//
// The state of a depot departure is taken as +0.0f: the forward's cvrp_advance gives (used + demand[0]) * 0.0f, which is
// +0.0f for every finite non-negative load.
//
// LDS budget (bytes, dynamic): 256 of scratch words + 4 V roundup(N, 4) of per-node vectors (CVRP V = 1: demand; OP V = 3: x,
// y, max_length; PCTSP V = 1: prize) + the table, 6 n_ants N + 4 n_ants, while n_ants * N <= kTableLdsEntries = 8 192 (48 KiB:
// 30 ants x 101 nodes take 18 KiB); above, the table lives in the caller's `scratch`
// (rl4co_aco_depot_grad_scratch_bytes(n_ants, N) per workgroup; a workgroup reads back only what it wrote itself). A non-NULL
// `scratch` is used at any size.
// Design estimates, NOT measured: the 48 KiB bound (three workgroups' tables per CU), the launcher-side choice of S
// (aco_tsp_grad.hip's) and the depot row's scheduling (one wave carries up to C softmaxes per ant for CVRP while a customer
// row carries one) rest on no profile; nothing about this kernel's occupancy or speed has been measured beyond
// tools/aco_bench.py --train's end-to-end time.
#include <hip/hip_runtime.h>

#include "ant_grad.h"
#include "ant_rules.h"

namespace {

using namespace rl4co::aco;  // ant_system.h: the constants, check_indices, log_softmax_max / _lse, launch; ant_grad.h; ant_rules.h

constexpr int kTableLdsEntries = 8192;
constexpr uint16_t kNoPos = 0xffff;

__host__ __device__ inline int cvrp_width(int N) {  // aco_cvrp.hip's W
  const int C = N - 1;
  return C + 1 > 2 * C - 1 ? C + 1 : 2 * C - 1;
}
__host__ __device__ inline int row_width(int env, int N) { return env == RL4CO_ENV_CVRP ? cvrp_width(N) : N; }
__host__ __device__ inline int node_vectors(int env) { return env == RL4CO_ENV_OP ? 3 : 1; }  // V
__host__ __device__ inline int node_stride(int N) { return (N + 3) & ~3; }                    // floats per vector
__host__ __device__ inline int node_bytes(int env, int N) { return 4 * node_vectors(env) * node_stride(N); }
// state [A, N] fp32, len [A] int32, pos [A, N] uint16, rounded up to 16 bytes
__host__ __device__ inline int64_t table_bytes(int A, int N) { return ((int64_t)6 * A * N + (int64_t)4 * A + 15) & ~(int64_t)15; }

// FILTER: each contribution runs over the kept set of its step under `o` (ant_system.h: filter_kept, the forward's text); false
// reads no `o` and is the kernel without it
template <int ENV, int KMAX, bool LDS, bool FILTER>
__global__ void __launch_bounds__(kThreads) aco_depot_grad_kernel(const rl4co_aco_depot_grad_args a,
                                                                  const rl4co_heatmap_decode_opts o) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  constexpr bool kCvrp = ENV == RL4CO_ENV_CVRP, kOp = ENV == RL4CO_ENV_OP;

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int S = a.row_split, B = a.B, N = a.N, A = a.n_ants;
  int b, s;
  grad_split(S, b, s);
  const int C = N - 1, W = row_width(ENV, N), NS = node_stride(N), K = (N + 63) >> 6;
  const int64_t AN = (int64_t)A * N;
  float* v0 = reinterpret_cast<float*>(smem + kScratchBytes);  // CVRP: demand (word c is demand[c - 1], word 0 demand[0])
  float* v1 = v0 + NS;                                         // OP: x, y, max_length        PCTSP: prize
  float* v2 = v1 + NS;
  unsigned char* tab = LDS ? smem + kScratchBytes + node_bytes(ENV, N)
                           : reinterpret_cast<unsigned char*>(a.scratch) + (int64_t)blockIdx.x * table_bytes(A, N);
  float* state = reinterpret_cast<float*>(tab);
  int* rlen = reinterpret_cast<int*>(state + AN);
  uint16_t* pos = reinterpret_cast<uint16_t*>(rlen + A);
  float* gout = a.grad_heatmap + (int64_t)b * N * N;
  const bool multistart = kCvrp && a.multistart != 0;
  float thr = 0.0f;  // CVRP: the right side of the capacity test
  if constexpr (kCvrp) thr = cvrp_threshold(a.vehicle_capacity[b]);

  // ---- 1. the refusals: indices, then the replay (both uniform: one LDS word) ----------------------------------------------
  bool ok = check_indices(nullptr, 0, 1, a.actions, W, A, B, b, N, smem, a.err);
  if (ok) {  // (bad_flag is 0 here)
    for (int n = tid; n < N; n += kThreads) {
      if constexpr (kCvrp) {
        v0[n] = a.demand[(int64_t)b * C + (n > 0 ? n - 1 : 0)];  // clamp(a - 1, 0, C - 1)
      } else if constexpr (kOp) {
        v0[n] = a.locs[((int64_t)b * N + n) * 2];
        v1[n] = a.locs[((int64_t)b * N + n) * 2 + 1];
        v2[n] = a.max_length[(int64_t)b * N + n];
      } else {
        v0[n] = a.prize[(int64_t)b * N + n];
      }
    }
    for (int64_t e = tid; e < AN; e += kThreads) pos[e] = kNoPos;
    __syncthreads();

    for (int j = w; j < A; j += kWaves) {  // one wave, one ant: the forward's state, action by action
      const int64_t* act = a.actions + ((int64_t)j * B + b) * W;
      uint16_t* pj = pos + (int64_t)j * N;
      float* sj = state + (int64_t)j * N;
      int cur = 0, left = C, t = 0;
      uint32_t vis = 0u, bits = 0u;  // vis bit k: node lane + 64 k is visited
      float acc = 0.0f;              // CVRP: used; OP: tour_length; PCTSP: cur_total_prize
      bool depot_seen = false, done = false, repeated = false;
      if (multistart) {  // column 0 is given: stepped through the state, no softmax
        const int c = __builtin_amdgcn_readfirstlane((int)act[0]);
        if (c == 0) {
          bits |= RL4CO_EBIT_TOUR_INDEX;  // a start is a customer (the forward's lower bound)
        } else {
          acc = cvrp_advance(acc, v0[c], 1);
          if ((c & 63) == lane) vis |= 1u << (c >> 6);
          left = C - 1;
          if (lane == 0) {
            pj[c] = 0;
            sj[c] = acc;
          }
          cur = c;
        }
        t = 1;
      }
      for (; t < W && !done; ++t) {  // bounded by W whatever the data
        const int c = __builtin_amdgcn_readfirstlane((int)act[t]);
        bool feasible;
        if (c != 0) {
          const uint32_t was = __shfl(vis, c & 63, 64);
          const bool seen = ((was >> (c >> 6)) & 1u) != 0;
          if (seen) {  // what follows in this row is a consequence: no further verdict is added
            bits |= RL4CO_EBIT_INVALID_TOUR;
            repeated = true;
          }
          if constexpr (kCvrp) {
            feasible = cvrp_fits(v0[c], acc, thr);
          } else if constexpr (kOp) {
            feasible = !depot_seen && op_within(op_advance(acc, op_dist(v0[cur], v1[cur], v0[c], v1[c])), v2[c]);
          } else {
            feasible = !depot_seen;
          }
          if (!seen) --left;
        } else {
          if constexpr (kCvrp) {
            bool any_customer = false;
            if (cur == 0) {  // (wave-uniform)
              uint32_t f = 0u;
              for (int k = 0; k < K; ++k) {
                const int n = lane + 64 * k;
                if (n >= 1 && n < N && !((vis >> k) & 1u) && cvrp_fits(v0[n], acc, thr)) f |= 1u << k;
              }
              any_customer = __any(f != 0u);
            }
            feasible = cvrp_depot_ok(cur, any_customer);
          } else if constexpr (kOp) {
            feasible = true;
          } else {
            feasible = pctsp_depot_ok(acc, left);
          }
        }
        if (!feasible && !repeated) bits |= RL4CO_EBIT_INFEASIBLE;
        if constexpr (kCvrp) {
          acc = cvrp_advance(acc, v0[c], c);
        } else if constexpr (kOp) {
          acc = op_advance(acc, op_dist(v0[cur], v1[cur], v0[c], v1[c]));
        } else {
          acc = pctsp_advance(acc, v0[c]);
        }
        if (c == 0) {
          depot_seen = true;
        } else {
          if ((c & 63) == lane) vis |= 1u << (c >> 6);
          if (lane == 0) {
            pj[c] = (uint16_t)t;
            sj[c] = acc;
          }
        }
        cur = c;
        done = kCvrp ? (left == 0 && depot_seen) : (c == 0 && t > 0);
      }
      if (!done && !repeated) bits |= RL4CO_EBIT_INFEASIBLE;  // W actions and not done
      if (lane == 0) {
        rlen[j] = t;
        if (bits) atomicOr(bad_flag(smem), bits);
      }
    }
    __syncthreads();
    const uint32_t bits = *bad_flag(smem);
    ok = bits == 0u;
    if (!ok && tid == 0) atomicOr(a.err, (int)bits);
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
    // one masked softmax: `feas` bit k of a lane: node lane + 64 k is feasible; `at` the action taken; `g` its upstream
    const auto contribute = [&](uint32_t feas, int at, float g) {
      if constexpr (FILTER) feas = filter_kept<KMAX>(z, feas, N, lane, o.top_k, o.top_p);  // removed nodes get 0
      const auto z_of = [&](int k, int) { return z[k]; };
      const auto feas_of = [&](int k) { return ((feas >> k) & 1u) != 0; };
      bool nan_seen;
      const float zmax = log_softmax_max(N, KMAX, lane, z_of, feas_of, nan_seen);
      if (!(zmax > kNegInf)) return;  // (wave-uniform: a butterflied value) every feasible logit is -inf
      const float lse = log_softmax_lse(N, KMAX, lane, z_of, feas_of, zmax);
#pragma unroll
      for (int k = 0; k < KMAX; ++k) {
        if ((feas >> k) & 1u) {
          const float lp = (z[k] - zmax) - lse;
          const float p = rl4co_expf(lp);
          const float d = (lane + 64 * k == at ? 1.0f : 0.0f) - p;
          float c = g * d;
          if (temp != 1.0f) c = c / temp;
          acc[k] = acc[k] + c;
        }
      }
    };
    const auto upstream = [&](int64_t row, int t) {
      float g = a.grad_ll[row];
      if (a.grad_steps) g = g + a.grad_steps[row * W + t];
      return g;
    };

    if (i == 0) {  // (wave-uniform) the depot row: every departure of every ant
      for (int j = 0; j < A; ++j) {
        const uint16_t* pj = pos + (int64_t)j * N;
        const int64_t row = (int64_t)j * B + b;
        const int64_t* act = a.actions + row * W;
        if constexpr (kCvrp) {
          const int len = rlen[j];
          for (int base = 0; base < len; base += 64) {
            const int t = base + lane;
            bool leaves = false;
            if (t < len) leaves = t == 0 ? !multistart : act[t - 1] == 0;
            unsigned long long departures = __ballot(leaves);
            while (departures) {  // (wave-uniform) ascending t
              const int tt = base + __builtin_ctzll(departures);
              departures &= departures - 1;
              uint32_t feas = 0u;
#pragma unroll
              for (int k = 0; k < KMAX; ++k) {
                const int n = lane + 64 * k;
                if (n >= 1 && n < N && (int)pj[n] >= tt && cvrp_fits(v0[n], 0.0f, thr)) feas |= 1u << k;
              }
              const bool any_customer = __any(feas != 0u);
              if (lane == 0 && cvrp_depot_ok(0, any_customer)) feas |= 1u;
              contribute(feas, __builtin_amdgcn_readfirstlane((int)act[tt]), upstream(row, tt));
            }
          }
        } else {  // OP, PCTSP: step 0 (OP's second departure has the depot alone: p = 1, nothing)
          uint32_t feas = 0u;
#pragma unroll
          for (int k = 0; k < KMAX; ++k) {
            const int n = lane + 64 * k;
            if (n >= 1 && n < N) {
              if constexpr (kOp) {
                if (op_within(op_advance(0.0f, op_dist(v0[0], v1[0], v0[n], v1[n])), v2[n])) feas |= 1u << k;
              } else {
                feas |= 1u << k;
              }
            }
          }
          if (lane == 0 && (kOp || pctsp_depot_ok(0.0f, C))) feas |= 1u;
          contribute(feas, __builtin_amdgcn_readfirstlane((int)act[0]), upstream(row, 0));
        }
      }
    } else {  // a customer row: at most one softmax per ant
      for (int j = 0; j < A; ++j) {
        const uint16_t* pj = pos + (int64_t)j * N;
        const int pi = pj[i];
        if (pi == kNoPos) continue;  // (wave-uniform) the ant never stood on i
        const int t = pi + 1;
        if (t >= rlen[j]) continue;  // (wave-uniform) the ant's last action: no step leaves it
        const float st = state[(int64_t)j * N + i];
        const int64_t row = (int64_t)j * B + b;
        uint32_t feas = 0u;
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
          const int n = lane + 64 * k;
          if (n >= 1 && n < N && (int)pj[n] > pi) {
            if constexpr (kCvrp) {
              if (cvrp_fits(v0[n], st, thr)) feas |= 1u << k;
            } else if constexpr (kOp) {
              if (op_within(op_advance(st, op_dist(v0[i], v1[i], v0[n], v1[n])), v2[n])) feas |= 1u << k;
            } else {
              feas |= 1u << k;
            }
          }
        }
        bool depot;
        if constexpr (kCvrp) {
          depot = cvrp_depot_ok(i, true);
        } else if constexpr (kOp) {
          depot = true;
        } else {
          depot = pctsp_depot_ok(st, C - t);  // t customers are visited at step t
        }
        if (lane == 0 && depot) feas |= 1u;
        contribute(feas, __builtin_amdgcn_readfirstlane((int)a.actions[row * W + t]), upstream(row, t));
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

template <int ENV, bool LDS, bool FILTER>
int launch_grad(const rl4co_aco_depot_grad_args& a, const rl4co_heatmap_decode_opts& o, int bytes, hipStream_t s) {
  return grad_ladder(a.N, [&](auto kmax) {
    return launch<aco_depot_grad_kernel<ENV, decltype(kmax)::value, LDS, FILTER>>(a, bytes, s, a.B * a.row_split, o);
  });
}

template <int ENV, bool FILTER>
int launch_tier(const rl4co_aco_depot_grad_args& a, const rl4co_heatmap_decode_opts& o, hipStream_t s) {
  const int fixed = kScratchBytes + node_bytes(ENV, a.N);
  if (a.scratch == nullptr) return launch_grad<ENV, true, FILTER>(a, o, fixed + (int)table_bytes(a.n_ants, a.N), s);
  return launch_grad<ENV, false, FILTER>(a, o, fixed, s);
}

template <int ENV>
int launch_env(const rl4co_aco_depot_grad_args& a, const rl4co_heatmap_decode_opts& o, hipStream_t s) {
  return decode_filter_on(o) ? launch_tier<ENV, true>(a, o, s) : launch_tier<ENV, false>(a, o, s);
}

}  // namespace

extern "C" int rl4co_aco_depot_grad_lds_entries(void) { return kTableLdsEntries; }

extern "C" int64_t rl4co_aco_depot_grad_scratch_bytes(int n_ants, int N) {
  if (n_ants < 1 || N < 2 || N > kMaxNodes) return -1;
  return table_bytes(n_ants, N);
}

extern "C" int rl4co_aco_depot_logp_grad(const rl4co_aco_depot_grad_args* args, void* stream) {
  const rl4co_heatmap_decode_opts off = {};
  return rl4co_aco_depot_logp_grad_opts(args, &off, stream);
}

extern "C" int rl4co_aco_depot_logp_grad_opts(const rl4co_aco_depot_grad_args* args, const rl4co_heatmap_decode_opts* opts,
                                              void* stream) {
  RL4CO_REQUIRE(args != nullptr);
  const rl4co_aco_depot_grad_args& a = *args;
  if (const int rc = require_decode_opts(opts, nullptr)) return rc;
  const rl4co_heatmap_decode_opts& o = *opts;  // (greedy is the forward's selector: nothing to differentiate)
  RL4CO_REQUIRE(a.env == RL4CO_ENV_CVRP || a.env == RL4CO_ENV_OP || a.env == RL4CO_ENV_PCTSP);
  RL4CO_REQUIRE(a.B >= 1);
  RL4CO_REQUIRE(a.N >= 2 && a.N <= kMaxNodes);
  RL4CO_REQUIRE(a.n_ants >= 1);
  RL4CO_REQUIRE((int64_t)a.n_ants * a.B <= 2147483647LL);
  RL4CO_REQUIRE(a.row_split >= 1 && a.row_split <= a.N);
  RL4CO_REQUIRE((int64_t)a.B * a.row_split <= 2147483647LL);
  RL4CO_REQUIRE(a.multistart == 0 || (a.multistart == 1 && a.env == RL4CO_ENV_CVRP));
  RL4CO_REQUIRE(a.temperature > 0.0f);
  RL4CO_REQUIRE(a.heatmap != nullptr && a.actions != nullptr && a.grad_ll != nullptr);
  RL4CO_REQUIRE(a.env != RL4CO_ENV_CVRP || (a.demand != nullptr && a.vehicle_capacity != nullptr));
  RL4CO_REQUIRE(a.env != RL4CO_ENV_OP || (a.locs != nullptr && a.max_length != nullptr));
  RL4CO_REQUIRE(a.env != RL4CO_ENV_PCTSP || a.prize != nullptr);
  RL4CO_REQUIRE(a.grad_heatmap != nullptr);
  RL4CO_REQUIRE(a.err != nullptr);
  RL4CO_REQUIRE(a.scratch != nullptr || (int64_t)a.n_ants * a.N <= kTableLdsEntries);  // above, the table lives in the caller's scratch
  hipStream_t s = rl4co::as_stream(stream);
  if (a.env == RL4CO_ENV_CVRP) return launch_env<RL4CO_ENV_CVRP>(a, o, s);
  if (a.env == RL4CO_ENV_OP) return launch_env<RL4CO_ENV_OP>(a, o, s);
  return launch_env<RL4CO_ENV_PCTSP>(a, o, s);
}

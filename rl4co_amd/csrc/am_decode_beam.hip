// am_decode_beam.hip — beam-search decoding (utils/decoding.py:464-600) as one persistent launch for gfx950.
//
// One workgroup of four waves per INSTANCE carries all W beams of that instance through the whole rollout: per step the
// masked log-prob row of every beam, the top-W selection over the W * N (parent, node) candidates, the re-parenting of
// the beam states and the environment transition; after the last step the parent chain is walked back and the aligned
// actions / log-probs are written. An entry point of its own (rl4co_am_decode_beam): no variant id, TSP and CVRP.
// Shared with am_decode.hip through decode_wave.h: the plane element types (CacheF32 / CacheBF16 / CacheF16), the layout
// constants, the 64-padding and the feasible-list compaction (build_list); the wave barrier is common.h's. The query, the
// three passes, the clip / log-softmax and the two transitions are this file's own text of the STREAM kernel's order:
// an edit to either text must be made in both (tests/test_gpu_beam.py::test_logps_equal_stream_evaluate).
//
// Work split
//   A  log-probs   wave w takes beams w, w + 4, ...: one beam at a time with exactly the one-wave arithmetic of the
//                  STREAM kernel (am_decode.hip header: folded context row + scalar, feasible list ascending, 8-head
//                  glimpse over row groups c % G with G = 64 / (128 / EPL), tanh clip, mask, log-softmax with the
//                  lane-strided sum and the butterfly trees). Same expressions, same order, -ffp-contract=off: a
//                  beam's log-prob of a node is bit for bit what rl4co_am_decode(mode = evaluate, variant = STREAM)
//                  reports for the same prefix. The W beams of an instance read the SAME three planes, but every beam
//                  issues its own global loads of the rows it lists: a row is re-read once per beam and step. Only the
//                  first of those reads can come from HBM; the planes (3 * N * 128 elements: 77 KB at N = 100 in 16 bits)
//                  exceed the CU's 32 KB vector cache, so the others are mostly trips to the XCD's L2 (not measured).
//                  Sharing a row among beams would need the beams' list positions (which fix the summation tree) to be
//                  decoupled from the load order; not done here. The row of a finished beam (CVRP)
//                  is not computed: depot 0.0, every other node -inf — what the reference's padding step gives
//                  (the depot is the only feasible node: log_softmax of one entry is exactly 0).
//   B  selection   candidates v(p, n) = cum[p] + lp[p][n] (one fp32 add, decoding.py:575), flat index p * N + n, dealt
//                  over the 256 threads (thread k holds indices k, k + 256, ...: at most 64 each). W rounds of a
//                  workgroup-wide maximum over 64-bit keys (order-preserving image of v) << 32 | ~index: the largest
//                  value wins, EQUAL VALUES ARE ORDERED BY THE LOWER FLAT INDEX p * N + n (the reference leaves ties to
//                  torch.topk); the winner's thread strikes it and rescans its own candidates. The W survivors come out
//                  in descending order = torch.topk(sorted=True). -inf is below every finite value, so it is chosen only
//                  when fewer than W finite candidates exist: RL4CO_EBIT_BEAM_INFEASIBLE ("infeasible action selected",
//                  decoding.py:485). NaN orders below -inf (torch.topk puts NaN first; either way RL4CO_EBIT_NAN_LOGIT
//                  is raised, "Logits contain NaNs").
//   C  re-parent   beam i takes the state of parent p_i — mask, visited flags, current / first node, step counter, used
//                  capacity, done — from the step's read buffer into the write buffer (double buffered in LDS with a
//                  barrier between: a parent may have several children), then applies the environment's transition for
//                  its node (tsp/env.py:60-86, cvrp/env.py:66-96,126-136: the step logic of am_decode.hip).
//   D  per step    chosen node, parent (int32), chosen log-prob and kept cumulative log-prob of every beam, column t.
//   E  backtrack   (_backtrack, decoding.py:527-557) final beam j: column T from row j, then row = parents[row][k] down to
//                  column 0. Rows are beam-major (s-major): row j * B + b = j-th best final beam of instance b.
// Column 0 is the start node (the state at entry is the one after the imposed start step, decoding.py:496-514) with
// log-prob 0 and parent 0; steps occupy columns 1 .. T, T <= max_steps; columns behind T are not written. T is the
// INSTANCE's horizon (its last beam's done): a CVRP instance that finishes before the batch's longest one leaves its later
// columns as the caller initialised them — zeros are the reference's padding there (depot, log-prob 0; every beam its own
// parent, as the beams are already in descending order) — and its state as it was at its own done.
//
// LDS budget (bytes; nw = N rounded up to 4, Np = N rounded up to 64):
//   log-prob rows        4 W nw
//   masks, visited       2 * 2 W nw            (read / write buffer)
//   beam scalars         56 W                  (8 int + 3 float arrays of W, 3 selection arrays of W)
//   wave scratch         4 * (38 Np + 32)      (scores [Np][8], logits [Np], head maxima [8], list [Np] u16)
//   reduction + flags    80
//   static               256                   (the compiler's scratch of __syncthreads_or: group_segment_fixed_size)
//   total(W, N) = 8 W nw + 56 W + 152 Np + 208 + 256 <= 160 KiB, and W * N <= 16384 (64 candidates per thread, one bit
//   each in the thread's struck set): rl4co_am_decode_beam_max_width(N). N = 100: W <= 163 (159 448 B at 163; W = N = 100
//   takes 105 520 B); N = 20: W <= 711 (LDS-bound). One workgroup per CU above 80 KiB, two below.
#include <hip/hip_runtime.h>

#include "common.h"
#include "decode_wave.h"
#include "env_table.h"
#include "rl4co_math.h"

namespace {

constexpr int kWaves = 4;
constexpr int kThreads = 64 * kWaves;
constexpr int kCandPerThread = 64;
constexpr int kCuLds = 160 * 1024;
constexpr int kStaticLds = 256;  // static LDS of every instantiation beside the dynamic bytes (checked at launch)

__host__ __device__ inline int pad4(int N) { return (N + 3) & ~3; }
__host__ __device__ inline int wave_scratch_bytes(int N) { return 38 * lds_pad(N) + 32; }
__host__ __device__ inline int64_t beam_lds_bytes(int64_t W, int N) {
  return 8 * W * pad4(N) + 56 * W + kWaves * wave_scratch_bytes(N) + 80;
}

// order-preserving image of a float (NaN below everything)
__device__ inline uint32_t ord_key(float v) {
  if (v != v) return 0u;
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// maximum of the (hi, lo) pairs over the wave, in every lane
template <int S = 1>
__device__ inline void bfly_max_u64(uint32_t& hi, uint32_t& lo) {
  if constexpr (S < 64) {
    const uint32_t oh = (uint32_t)rl4co::bfly_i<S>((int)hi), ol = (uint32_t)rl4co::bfly_i<S>((int)lo);
    if (oh > hi || (oh == hi && ol > lo)) {
      hi = oh;
      lo = ol;
    }
    bfly_max_u64<S * 2>(hi, lo);
  }
}

template <class C, int ENV>
__global__ void __launch_bounds__(kThreads) am_decode_beam_kernel(const rl4co_am_decode_beam_args a) {
  constexpr int EPL = C::EPL;
  constexpr int LPR = kD / EPL;   // lanes per cache row
  constexpr int RPL = 64 / LPR;   // rows per wave-wide load (= row groups G)
  constexpr int LPH = kDH / EPL;  // lanes per head
  constexpr bool kTsp = ENV == RL4CO_ENV_TSP;
  using elem = typename C::elem;
  using raw_t = typename C::raw;

  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
  const int b = blockIdx.x, B = a.B_inst, W = a.beam_width, N = a.N;
  const int nw = pad4(N), Np = lds_pad(N);
  const int64_t os = a.out_stride;

  float* lp = reinterpret_cast<float*>(smem);        // [W][nw] log-prob rows by node
  int* ib = reinterpret_cast<int*>(lp + W * nw);     // cur[2][W] first[2][W] step[2][W] done[2][W]
  float* usedb = reinterpret_cast<float*>(ib + 8 * W);  // used[2][W]
  float* cum = usedb + 2 * W;                        // [W] cumulative log-prob of each beam
  int* selp = reinterpret_cast<int*>(cum + W);       // [W] parent of the i-th best candidate
  int* seln = selp + W;                              // [W] its node
  float* selv = reinterpret_cast<float*>(seln + W);  // [W] its cumulative value
  unsigned char* ws = reinterpret_cast<unsigned char*>(selv + W) + w * wave_scratch_bytes(N);
  float* sc = reinterpret_cast<float*>(ws);          // [Np*8] per-head scores -> softmax numerators
  float* lg = sc + Np * kH;                          // [Np] logits (list order)
  float* mh = lg + Np;                               // [8] per-head maxima
  uint16_t* fl = reinterpret_cast<uint16_t*>(mh + kH);  // [Np] feasible nodes, ascending
  unsigned char* tail = reinterpret_cast<unsigned char*>(selv + W) + kWaves * wave_scratch_bytes(N);
  uint32_t* red = reinterpret_cast<uint32_t*>(tail);   // [2][4][2] wave maxima (hi, lo) of a selection round
  uint8_t* mkb = tail + 80;                            // [2][W][nw] 1 = feasible
  uint8_t* visb = mkb + 2 * W * nw;                    // [2][W][nw] CVRP visited flags
  auto icur = [&](int p) { return ib + p * W; };
  auto ifirst = [&](int p) { return ib + (2 + p) * W; };
  auto istep = [&](int p) { return ib + (4 + p) * W; };
  auto idone = [&](int p) { return ib + (6 + p) * W; };

  const int rg = lane / LPR, li = lane % LPR, hd = li / LPH, e0 = li * EPL;
  const elem* Kg = static_cast<const elem*>(a.glimpse_key) + (int64_t)b * a.kvl_batch_stride + e0;
  const elem* Vg = static_cast<const elem*>(a.glimpse_val) + (int64_t)b * a.kvl_batch_stride + e0;
  const elem* Kl = static_cast<const elem*>(a.logit_key) + (int64_t)b * a.kvl_batch_stride + e0;
  const int64_t rs = a.kvl_row_stride;
  const float* ctx_cur = a.ctx_cur + (int64_t)b * N * kD + e0;
  const float* ctx_first = kTsp ? a.ctx_first + (int64_t)b * N * kD + e0 : nullptr;
  const float* dem = kTsp ? nullptr : a.demand + (int64_t)b * (N - 1);
  const float cap = kTsp ? 0.0f : a.vehicle_capacity[b];  // (batchified: the same in every beam row of the instance)
  uint32_t errbits = 0;

  // ---- load the W beam states (rows j * B + b) into buffer 0; column 0 of the per-step outputs ----------------------
  for (int idx = tid; idx < W * nw; idx += kThreads) {
    const int j = idx / nw, n = idx - j * nw;
    const int64_t row = (int64_t)j * B + b;
    mkb[idx] = (n < N) ? a.action_mask[row * N + n] : (uint8_t)0;
    visb[idx] = (!kTsp && n < N) ? a.visited[row * N + n] : (uint8_t)1;
  }
  for (int j = tid; j < W; j += kThreads) {
    const int64_t row = (int64_t)j * B + b;
    const int c = (int)a.current_node[row];
    icur(0)[j] = min(max(c, 0), N - 1);
    ifirst(0)[j] = kTsp ? min(max((int)a.first_node[row], 0), N - 1) : 0;
    const long long si = kTsp ? a.step_i[row] : 0;
    istep(0)[j] = (int)(si < 0 ? 0 : (si > 0x3fffffff ? 0x3fffffff : si));
    idone(0)[j] = a.done[row] != 0;
    usedb[j] = kTsp ? 0.0f : a.used_capacity[row];
    cum[j] = 0.0f;
    a.step_nodes[row * os] = c;
    a.parents[row * os] = 0;
    a.step_logps[row * os] = 0.0f;
    a.cum_logp[row * os] = 0.0f;
  }

  float qb[EPL];
#pragma unroll
  for (int e = 0; e < EPL; ++e) qb[e] = a.q_bias ? a.q_bias[(int64_t)b * kD + e0 + e] : 0.0f;

  const int total = W * N;
  const int s256p = kThreads / N, s256n = kThreads % N;  // flat-index stride of a thread's candidates as (parent, node)
  const int tp0 = tid / N, tn0 = tid % N;
  int t = 0, p = 0;

  for (;;) {
    __syncthreads();
    bool open = false;
    for (int j = tid; j < W; j += kThreads) open |= idone(p)[j] == 0;
    if (!__syncthreads_or(open ? 1 : 0)) break;
    if (t >= a.max_steps) {
      errbits |= RL4CO_EBIT_MAX_STEPS;
      break;
    }
    ++t;
    // ================= A: the log-prob row of every beam (one wave per beam at a time) ==========================
    for (int j = w; j < W; j += kWaves) {
      const uint8_t* mk = mkb + (p * W + j) * nw;
      float* row = lp + j * nw;
      for (int n = lane; n < nw; n += 64) row[n] = kNegInf;
      if (idone(p)[j] != 0) {  // finished (CVRP): the padding step offers the depot alone, log-prob 0
        rl4co::lds_barrier_wave();
        if (lane == 0) row[0] = 0.0f;
        continue;
      }
      const int cur = icur(p)[j], first = ifirst(p)[j], step_i = istep(p)[j];
      const float used = usedb[p * W + j];
      const int F = build_list(a, mk, fl, N, lane);  // feasible nodes, ascending (or all nodes when either mask flag is off)

      // ---- query: folded context row(s) + scalar + graph context, * 1/sqrt(16) ------------------------------------
      float q[EPL];
      if (kTsp) {
        if (step_i < 1) {  // context.py:120 placeholder context
#pragma unroll
          for (int e = 0; e < EPL; ++e) q[e] = a.q_step0[e0 + e] + qb[e];
        } else {
#pragma unroll
          for (int e = 0; e < EPL; ++e) q[e] = (ctx_first[(int64_t)first * kD + e] + ctx_cur[(int64_t)cur * kD + e]) + qb[e];
        }
      } else {
        const float rem = cap - used;  // context.py:147-149
#pragma unroll
        for (int e = 0; e < EPL; ++e) q[e] = fmaf(a.w_cap[e0 + e], rem, ctx_cur[(int64_t)cur * kD + e]) + qb[e];
      }
#pragma unroll
      for (int e = 0; e < EPL; ++e) q[e] = q[e] * 0.25f;

      // ---- pass 1: per-head scores ----------------------------------------------------------------------------
      float m = kNegInf;
      for (int c0 = 0; c0 < F; c0 += RPL * kUnroll) {
        raw_t rw[kUnroll];
        int jj[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
          const int c = c0 + u * RPL + rg;
          jj[u] = (c < F) ? (int)fl[c] : -1;
          rw[u] = (jj[u] < 0) ? C::zero() : C::ld(Kg + (int64_t)jj[u] * rs);
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
          const int c = c0 + u * RPL + rg;
          const bool valid = jj[u] >= 0;
          float k[EPL];
          C::cvt(rw[u], k);
          float acc = 0.0f;
#pragma unroll
          for (int e = 0; e < EPL; ++e) acc = fmaf(q[e], k[e], acc);
          acc = rl4co::bfly_sum<1, LPH>(acc);
          const bool feas = valid && (!a.mask_inner || mk[valid ? jj[u] : 0] != 0);
          const float sv = feas ? acc : kNegInf;
          if (valid && (li % LPH) == 0) sc[c * kH + hd] = sv;
          m = fmaxf(m, sv);
        }
      }
      m = rl4co::bfly_max<LPR, 64>(m);
      if (rg == 0 && (li % LPH) == 0) mh[hd] = m;
      rl4co::lds_barrier_wave();
      {
        const float mm = mh[lane & (kH - 1)];
        for (int idx = lane; idx < F * kH; idx += 64) sc[idx] = rl4co_expf(sc[idx] - mm);
      }
      rl4co::lds_barrier_wave();

      // ---- pass 2: softmax-weighted value sum -----------------------------------------------------------------
      float lacc = 0.0f;
      float oacc[EPL];
#pragma unroll
      for (int e = 0; e < EPL; ++e) oacc[e] = 0.0f;
      for (int c0 = 0; c0 < F; c0 += RPL * kUnroll) {
        raw_t rw[kUnroll];
        bool ok[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
          const int c = c0 + u * RPL + rg;
          ok[u] = c < F;
          rw[u] = !ok[u] ? C::zero() : C::ld(Vg + (int64_t)fl[c] * rs);
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
          const int c = c0 + u * RPL + rg;
          float v[EPL];
          C::cvt(rw[u], v);
          const float pr = ok[u] ? sc[c * kH + hd] : 0.0f;
          lacc = lacc + pr;
#pragma unroll
          for (int e = 0; e < EPL; ++e) oacc[e] = fmaf(pr, v[e], oacc[e]);
        }
      }
      const float l = 1.0f / rl4co::bfly_sum<LPR, 64>(lacc);
      float o[EPL];
#pragma unroll
      for (int e = 0; e < EPL; ++e) o[e] = rl4co::bfly_sum<LPR, 64>(oacc[e]) * l;

      // ---- pass 3: pointer logits -----------------------------------------------------------------------------
      for (int c0 = 0; c0 < F; c0 += RPL * kUnroll) {
        raw_t rw[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
          const int c = c0 + u * RPL + rg;
          rw[u] = (c >= F) ? C::zero() : C::ld(Kl + (int64_t)fl[c] * rs);
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
          const int c = c0 + u * RPL + rg;
          float k[EPL];
          C::cvt(rw[u], k);
          float acc = 0.0f;
#pragma unroll
          for (int e = 0; e < EPL; ++e) acc = fmaf(o[e], k[e], acc);
          acc = rl4co::bfly_sum<1, LPR>(acc);
          if (c < F && li == 0) lg[c] = acc;
        }
      }
      rl4co::lds_barrier_wave();

      // ---- clip, mask, log-softmax (finalize_and_step's order) ------------------------------------------------------
      bool nan_seen = false;
      float zmax = kNegInf;
      for (int c = lane; c < F; c += 64) {
        float z = lg[c] / kSqrtD;
        if (z != z) nan_seen = true;  // attention.py:295-296
        if (a.tanh_clipping > 0.0f) z = rl4co_tanhf(z) * a.tanh_clipping;
        if (a.mask_logits && mk[fl[c]] == 0) z = kNegInf;
        if (a.temperature != 1.0f) z = z / a.temperature;
        lg[c] = z;
        zmax = fmaxf(zmax, z);
      }
      if (__any(nan_seen)) errbits |= RL4CO_EBIT_NAN_LOGIT;
      zmax = rl4co::bfly_max<1, 64>(zmax);
      float zsum = 0.0f;
      for (int c = lane; c < F; c += 64) zsum = zsum + rl4co_expf(lg[c] - zmax);
      zsum = rl4co::bfly_sum<1, 64>(zsum);
      const float lse = rl4co_logf(zsum);
      for (int c = lane; c < F; c += 64) row[fl[c]] = (lg[c] - zmax) - lse;
      rl4co::lds_barrier_wave();
    }
    __syncthreads();

    // ================= B: the W largest of cum[p] + lp[p][n], descending, ties by lower flat index ==============
    unsigned long long struck = 0ull;
    auto scan = [&](uint32_t& bh, uint32_t& bl) {
      bh = 0u;
      bl = 0u;
      int pp = tp0, nn = tn0, k = 0;
      for (int idx = tid; idx < total; idx += kThreads, ++k) {
        if (!((struck >> k) & 1ull)) {
          const uint32_t h = ord_key(cum[pp] + lp[pp * nw + nn]), lo = 0xffffffffu - (uint32_t)idx;
          if (h > bh || (h == bh && lo > bl)) {
            bh = h;
            bl = lo;
          }
        }
        nn += s256n;
        pp += s256p;
        if (nn >= N) {
          nn -= N;
          ++pp;
        }
      }
    };
    uint32_t mh_ = 0u, ml_ = 0u;
    scan(mh_, ml_);
    for (int i = 0; i < W; ++i) {
      uint32_t h = mh_, lo = ml_;
      bfly_max_u64(h, lo);
      uint32_t* slot = red + (i & 1) * 2 * kWaves;
      if (lane == 0) {
        slot[2 * w] = h;
        slot[2 * w + 1] = lo;
      }
      __syncthreads();
      h = slot[0];
      lo = slot[1];
#pragma unroll
      for (int k = 1; k < kWaves; ++k) {
        const uint32_t oh = slot[2 * k], ol = slot[2 * k + 1];
        if (oh > h || (oh == h && ol > lo)) {
          h = oh;
          lo = ol;
        }
      }
      uint32_t idx = 0xffffffffu - lo;
      if (idx >= (uint32_t)total) idx = 0u;  // (cannot happen: W * N >= 2 W candidates)
      if (tid == 0) {
        const int pp = (int)idx / N, nn = (int)idx - pp * N;
        selp[i] = pp;
        seln[i] = nn;
        selv[i] = cum[pp] + lp[pp * nw + nn];
      }
      if ((int)(idx & (kThreads - 1)) == tid) {
        struck |= 1ull << (idx >> 8);
        scan(mh_, ml_);
      }
    }
    __syncthreads();

    // ================= C: re-parent (read buffer p -> write buffer q), D: the step's outputs ======================
    const int q_ = p ^ 1;
    {
      const int wpr = nw >> 2;  // 32-bit words per row
      const uint32_t* ms = reinterpret_cast<const uint32_t*>(mkb + p * W * nw);
      uint32_t* md = reinterpret_cast<uint32_t*>(mkb + q_ * W * nw);
      const uint32_t* vs = reinterpret_cast<const uint32_t*>(visb + p * W * nw);
      uint32_t* vd = reinterpret_cast<uint32_t*>(visb + q_ * W * nw);
      for (int idx = tid; idx < W * wpr; idx += kThreads) {
        const int i = idx / wpr, o = idx - i * wpr;
        const int pp = selp[i];
        md[idx] = ms[pp * wpr + o];
        if (!kTsp) vd[idx] = vs[pp * wpr + o];
      }
    }
    for (int i = tid; i < W; i += kThreads) {
      const int pp = selp[i], nn = seln[i];
      const float v = selv[i], lpv = lp[pp * nw + nn];
      icur(q_)[i] = icur(p)[pp];
      ifirst(q_)[i] = ifirst(p)[pp];
      istep(q_)[i] = istep(p)[pp];
      idone(q_)[i] = idone(p)[pp];
      usedb[q_ * W + i] = usedb[p * W + pp];
      if (mkb[(p * W + pp) * nw + nn] == 0) errbits |= RL4CO_EBIT_INFEASIBLE;  // decoding.py:485
      if (!(v > kNegInf)) errbits |= RL4CO_EBIT_BEAM_INFEASIBLE;                // fewer than W finite candidates
      const int64_t at = ((int64_t)i * B + b) * os + t;
      a.step_nodes[at] = nn;
      a.parents[at] = pp;
      a.step_logps[at] = lpv;
      a.cum_logp[at] = v;
    }
    __syncthreads();
    for (int i = tid; i < W; i += kThreads) cum[i] = selv[i];  // (behind the barrier: every thread has read the old values)

    // ---- the environment's transition of every beam for its node (one wave per beam at a time) ------------------
    for (int i = w; i < W; i += kWaves) {
      uint8_t* mk = mkb + (q_ * W + i) * nw;
      uint8_t* vis = visb + (q_ * W + i) * nw;
      const int bi = seln[i];
      if (kTsp) {
        if (lane == 0) {
          if (istep(q_)[i] == 0) ifirst(q_)[i] = bi;  // tsp/env.py:63
          icur(q_)[i] = bi;
          istep(q_)[i] = min(istep(q_)[i] + 1, 0x3fffffff);
          mk[bi] = 0;
        }
        rl4co::lds_barrier_wave();
        bool any_left = false;
        for (int n = lane; n < N; n += 64) any_left |= mk[n] != 0;
        const bool dn = !__any(any_left);  // tsp/env.py:71
        if (lane == 0) idone(q_)[i] = dn ? 1 : 0;
      } else {
        const int di = min(max(bi - 1, 0), N - 2);                                      // cvrp/env.py:71-73
        const float used = (usedb[q_ * W + i] + dem[di]) * (bi != 0 ? 1.0f : 0.0f);     // cvrp/env.py:76
        rl4co::lds_barrier_wave();  // every lane has read the beam's used capacity
        if (lane == 0) {
          usedb[q_ * W + i] = used;
          icur(q_)[i] = bi;
          vis[bi] = 1;
        }
        rl4co::lds_barrier_wave();
        const float thr = cap + 1e-5f;  // cvrp/env.py:128
        bool any_feasible = false, all_visited = true;
        for (int n = lane; n < N; n += 64) {
          all_visited &= vis[n] != 0;
          if (n >= 1) {
            const bool masked = (vis[n] != 0) || (dem[n - 1] + used > thr);
            mk[n] = masked ? 0 : 1;
            any_feasible |= !masked;
          }
        }
        any_feasible = __any(any_feasible);
        const bool dn = __all(all_visited);  // cvrp/env.py:83
        if (lane == 0) {
          idone(q_)[i] = dn ? 1 : 0;
          mk[0] = ((bi == 0) && any_feasible) ? 0 : 1;  // cvrp/env.py:134-135
        }
      }
    }
    p = q_;
  }

  // ================= E: backtrack the parent chain into the aligned outputs ========================================
  __threadfence_block();
  __syncthreads();
  for (int j = tid; j < W; j += kThreads) {
    int c = j;
    const int64_t out = ((int64_t)j * B + b) * os;
    for (int k = t; k >= 0; --k) {
      const int64_t at = ((int64_t)c * B + b) * os + k;
      const float lpv = a.step_logps[at];
      a.actions[out + k] = (int64_t)a.step_nodes[at];
      a.logps[out + k] = lpv;
      if (k > 0 && !(lpv > -1000.0f)) errbits |= RL4CO_EBIT_NEG_INF_LOGP;  // decoding.py:56
      if (k > 0) c = min(max(a.parents[at], 0), W - 1);
    }
  }

  // ---- write the state back -----------------------------------------------------------------------------------------
  for (int idx = tid; idx < W * nw; idx += kThreads) {
    const int j = idx / nw, n = idx - j * nw;
    if (n < N) {
      const int64_t row = (int64_t)j * B + b;
      a.action_mask[row * N + n] = mkb[p * W * nw + idx];
      if (!kTsp) a.visited[row * N + n] = visb[p * W * nw + idx];
    }
  }
  for (int j = tid; j < W; j += kThreads) {
    const int64_t row = (int64_t)j * B + b;
    a.current_node[row] = icur(p)[j];
    a.done[row] = idone(p)[j] ? 1 : 0;
    if (kTsp) {
      a.first_node[row] = ifirst(p)[j];
      a.step_i[row] = istep(p)[j];
    } else {
      a.used_capacity[row] = usedb[p * W + j];
    }
  }
  if (tid == 0 && a.steps_summary) {
    atomicMax(a.steps_summary, t);
    atomicAdd(a.steps_summary + 1, t);
  }
  if (errbits) atomicOr(a.err, (int)errbits);
}

template <class C, int ENV>
int launch(const rl4co_am_decode_beam_args& a, hipStream_t stream) {
  const int lds = (int)beam_lds_bytes(a.beam_width, a.N);
  hipFuncAttributes fa;
  RL4CO_HIP_TRY(hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(am_decode_beam_kernel<C, ENV>)));
  RL4CO_REQUIRE((int64_t)fa.sharedSizeBytes <= kStaticLds);  // the budget of rl4co_am_decode_beam_max_width holds
  if (lds > 64 * 1024) {
    RL4CO_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(am_decode_beam_kernel<C, ENV>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  }
  hipLaunchKernelGGL((am_decode_beam_kernel<C, ENV>), dim3(a.B_inst), dim3(kThreads), lds, stream, a);
  RL4CO_HIP_TRY(hipGetLastError());
  return RL4CO_OK;
}

}  // namespace

extern "C" int rl4co_am_decode_beam_max_width(int N) {
  if (N < 2 || N > 1024) return 0;
  int W = kCandPerThread * kThreads / N;
  while (W > 0 && beam_lds_bytes(W, N) + kStaticLds > kCuLds) --W;
  return W;
}

extern "C" int rl4co_am_decode_beam(const rl4co_am_decode_beam_args* args, void* stream) {
  RL4CO_REQUIRE(args != nullptr);
  const rl4co_am_decode_beam_args& a = *args;
  RL4CO_REQUIRE(rl4co::env_served(a.env, &rl4co::EnvRecord::beam));
  RL4CO_REQUIRE(a.B_inst > 0);
  RL4CO_REQUIRE(a.N >= 2 && a.N <= 1024);
  RL4CO_REQUIRE(a.beam_width >= 2);  // decoding.py:494 "beam width must be larger than 1"
  RL4CO_REQUIRE(a.beam_width <= rl4co_am_decode_beam_max_width(a.N));
  RL4CO_REQUIRE((int64_t)a.beam_width * a.B_inst <= 0x7fffffff);
  RL4CO_REQUIRE(a.max_steps >= 1);
  RL4CO_REQUIRE(a.out_stride >= 2 && (int64_t)a.max_steps + 1 <= a.out_stride);
  RL4CO_REQUIRE(a.cache_dtype == RL4CO_DT_F32 || a.cache_dtype == RL4CO_DT_BF16 || a.cache_dtype == RL4CO_DT_F16);
  RL4CO_REQUIRE(a.glimpse_key && a.glimpse_val && a.logit_key && a.ctx_cur);
  RL4CO_REQUIRE(((reinterpret_cast<uintptr_t>(a.glimpse_key) | reinterpret_cast<uintptr_t>(a.glimpse_val) |
                  reinterpret_cast<uintptr_t>(a.logit_key)) & 15) == 0);
  RL4CO_REQUIRE(a.kvl_row_stride >= kD && a.kvl_row_stride % 8 == 0);
  RL4CO_REQUIRE(a.kvl_batch_stride >= (int64_t)a.N * kD && a.kvl_batch_stride % 8 == 0);
  RL4CO_REQUIRE(a.temperature > 0.0f);
  RL4CO_REQUIRE(a.action_mask && a.current_node && a.done);
  RL4CO_REQUIRE(a.actions && a.logps && a.step_nodes && a.step_logps && a.parents && a.cum_logp && a.err);
  if (a.env == RL4CO_ENV_TSP) {
    RL4CO_REQUIRE(a.ctx_first && a.q_step0 && a.first_node && a.step_i);
  } else {
    RL4CO_REQUIRE(a.w_cap && a.demand && a.used_capacity && a.vehicle_capacity && a.visited);
  }
  hipStream_t s = rl4co::as_stream(stream);
  using rl4co::Planes;
  return rl4co::dispatch_planes<Planes<RL4CO_DT_F32, CacheF32>, Planes<RL4CO_DT_BF16, CacheBF16>, Planes<RL4CO_DT_F16, CacheF16>>(
      a.cache_dtype, [&](auto p) {
        return rl4co::dispatch_env<&rl4co::EnvRecord::beam>(a.env, [&](auto e) { return launch<typename decltype(p)::type, decltype(e)::value>(a, s); });
      });
}

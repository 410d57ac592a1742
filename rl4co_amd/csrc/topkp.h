// topkp.h — the top-k / top-p (nucleus) filter of one decode step, for one wave (utils/decoding.py:109-188,
// modify_logits_for_top_k_filtering / modify_logits_for_top_p_filtering). The order of every sum is the one written down
// in the am_decode.hip header; this file only restates it.
//
// Bounded work, no sort: the k-th largest logit is found by bisecting its order-preserving uint32 image (32 counting
// passes), the top-p cut by bisecting the same image against the mass below it (32 passes) and then the rank inside the
// tie group at the cut (ceil(log2(F + 1)) passes). Each pass is a lane-strided walk over the list plus one butterfly.
#ifndef RL4CO_TOPKP_H
#define RL4CO_TOPKP_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"

namespace rl4co {

// Order-preserving image of a non-NaN float: a < b <=> okey(a) < okey(b), -0 and +0 equal (x + 0.0f is +0 for both)
__device__ inline uint32_t topkp_key(float x) {
  const uint32_t u = __float_as_uint(x + 0.0f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// Whether `a` asks for the filter path at all (k >= N and p outside (0, 1) remove nothing; the kept-set output alone
// also takes it). Uniform over the launch.
__host__ __device__ inline bool topkp_on(const rl4co_am_decode_args& a) {
  return (a.top_k > 0 && a.top_k < a.N) || (a.top_p > 0.0f && a.top_p < 1.0f) || a.kept_bits != nullptr;
}

// One wave. z[0..F): the step's processed logits in list order (-inf = masked), e[0..F): rl4co_expf(z - zmax) staged by
// the caller. Removes what top-k (0 < k < F) and then top-p (0 < p < 1) remove: z = -inf, e = 0; the largest z (the last
// entry in the (z, c) order) is never removed. Returns the sum of the
// kept e in the log-sum-exp order (lane-strided, then the butterfly) — the unfiltered sum, bit for bit, when nothing is
// removed. Every lane touches only its own list entries c = lane + 64 i.
__device__ inline float topkp_filter(float* z, float* e, int F, int k, float p, int lane) {
  constexpr float kNegInf = -__builtin_huge_valf();
  if (k > 0 && k < F) {
    // tau = largest T with #{c : key_c >= T} >= k = the key of the k-th largest z, counted with multiplicity
    uint32_t tau = 0;
#pragma unroll 1
    for (int b = 31; b >= 0; --b) {
      const uint32_t cand = tau | (1u << b);
      int n = 0;
#pragma unroll 1
      for (int c = lane; c < F; c += 64) n += topkp_key(z[c]) >= cand ? 1 : 0;
      if (bfly_i_sum(n) >= k) tau = cand;
    }
    for (int c = lane; c < F; c += 64) {
      if (topkp_key(z[c]) < tau) {  // the reference removes logits < tau: ties at tau stay
        z[c] = kNegInf;
        e[c] = 0.0f;
      }
    }
  }
  auto mass = [&](uint32_t below, uint32_t at, int upto) {  // sum of e over key < below, or key == at and c <= upto
    float s = 0.0f;
#pragma unroll 1
    for (int c = lane; c < F; c += 64) {
      const uint32_t kc = topkp_key(z[c]);
      s = s + ((kc < below || (kc == at && c <= upto)) ? e[c] : 0.0f);
    }
    return bfly_sum<1, 64>(s);
  };
  if (p > 0.0f && p < 1.0f) {
    // entries ordered by (z, c) ascending; c is removed iff A_c = mass of the entries up to c <= (1 - p) Z
    const float zall = mass(0xFFFFFFFFu, 0xFFFFFFFFu, 0x7fffffff);
    // (1 - p) rounds to 1 for p below ~6e-8: keep the threshold under Z so that the last entry in the order — the largest
    // z — always survives (zall >= 1: the maximum's own term is exp(0))
    const float thr = fminf((1.0f - p) * zall, __uint_as_float(__float_as_uint(zall) - 1u));
    uint32_t cut = 0;  // largest T with mass(key < T) <= thr: below it all removed, above it all kept
#pragma unroll 1
    for (int b = 31; b >= 0; --b) {
      const uint32_t cand = cut | (1u << b);
      if (mass(cand, 0u, -1) <= thr) cut = cand;
    }
    int lo = -1, hi = F;  // the tie group at the cut, by list position: the largest lo with A(lo) <= thr
#pragma unroll 1
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (mass(cut, cut, mid) <= thr) lo = mid; else hi = mid;
    }
    for (int c = lane; c < F; c += 64) {
      const uint32_t kc = topkp_key(z[c]);
      if (kc < cut || (kc == cut && c <= lo)) {
        z[c] = kNegInf;
        e[c] = 0.0f;
      }
    }
  }
  float s = 0.0f;
  for (int c = lane; c < F; c += 64) s = s + e[c];
  return bfly_sum<1, 64>(s);
}

// One wave: the kept set of a step as bits by node — word w, bit b = node 32 w + b listed with a finite filtered logit —
// into out[0..words) (words a multiple of 4, bits >= N zero). `flags`: N words of scratch.
__device__ inline void topkp_write_bits(uint32_t* out, int words, const float* z, const uint16_t* fl, int F, int N,
                                        uint32_t* flags, int lane) {
  constexpr float kNegInf = -__builtin_huge_valf();
  for (int j = lane; j < N; j += 64) flags[j] = 0u;
  lds_barrier_wave();
  for (int c = lane; c < F; c += 64)
    if (z[c] > kNegInf) flags[fl[c]] = 1u;
  lds_barrier_wave();
  for (int j0 = 0; j0 < 32 * words; j0 += 64) {
    const int j = j0 + lane;
    const unsigned long long bal = __ballot(j < N && flags[j] != 0u);
    if (lane < 2) out[j0 / 32 + lane] = (uint32_t)(bal >> (32 * lane));
  }
  lds_barrier_wave();
}

}  // namespace rl4co

#endif

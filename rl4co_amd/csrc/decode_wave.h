// decode_wave.h — what a one-wave decode step is built from, shared by am_decode.hip (STREAM and the four-wave kernels)
// and am_decode_beam.hip (one wave per beam): the plane element types with their exact widening, the layout constants,
// the trajectory state and the feasible-list compaction. The arithmetic order stated in am_decode.hip's header is the
// parity contract; a block here is the ONE text of its part of it.
//
// Condition for editing this file: the gfx950 device assembly of am_decode.hip (compiled with build.COMPILE_FLAGS) must
// stay identical to the parent commit's unless the change is meant to alter the hot kernels ("decode_wave.h").
// Moving the clip / log-sum-exp loop or the environment transition here changed that assembly (instruction order, SGPR
// numbering), so those two stay in am_decode.hip and am_decode_beam.hip keeps its own text of them.
//
// Everything sits in the unnamed namespace, as it did in the two sources: internal to each translation unit.
#ifndef RL4CO_DECODE_WAVE_H
#define RL4CO_DECODE_WAVE_H

#include <hip/hip_runtime.h>

#include "common.h"
#include "rl4co_math.h"

namespace {

constexpr int kD = RL4CO_EMBED_DIM;
constexpr int kH = RL4CO_NUM_HEADS;
constexpr int kDH = kD / kH;
constexpr int kUnroll = 4;  // wave-wide 1 KiB loads kept in flight per pass
constexpr float kNegInf = -__builtin_huge_valf();
constexpr float kSqrtD = 11.3137084989847604f;  // fl32(sqrt(128)), attention.py:293

struct CacheF32 {
  using elem = float;
  using raw = float4;
  static constexpr int EPL = 4;
  __device__ static inline raw zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
  __device__ static inline raw ld(const elem* p) { return *reinterpret_cast<const float4*>(p); }
  __device__ static inline void cvt(const raw& t, float (&v)[4]) {
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  }
};

struct CacheBF16 {
  using elem = uint16_t;
  using raw = uint4;
  static constexpr int EPL = 8;
  __device__ static inline raw zero() { return make_uint4(0u, 0u, 0u, 0u); }
  __device__ static inline raw ld(const elem* p) { return *reinterpret_cast<const uint4*>(p); }
  __device__ static inline void cvt(const raw& t, float (&v)[8]) {
    v[0] = __uint_as_float(t.x << 16); v[1] = __uint_as_float(t.x & 0xffff0000u);
    v[2] = __uint_as_float(t.y << 16); v[3] = __uint_as_float(t.y & 0xffff0000u);
    v[4] = __uint_as_float(t.z << 16); v[5] = __uint_as_float(t.z & 0xffff0000u);
    v[6] = __uint_as_float(t.w << 16); v[7] = __uint_as_float(t.w & 0xffff0000u);
  }
};

// IEEE half planes (torch.float16: the reference's default "16-mixed" precision, utils/trainer.py:57): same 16-byte
// lanes as bf16, converted with v_cvt_f32_f16 — exact, like the bf16 shift
struct CacheF16 {
  using elem = uint16_t;
  using raw = uint4;
  static constexpr int EPL = 8;
  typedef _Float16 half2_t __attribute__((ext_vector_type(2)));
  __device__ static inline raw zero() { return make_uint4(0u, 0u, 0u, 0u); }
  __device__ static inline raw ld(const elem* p) { return *reinterpret_cast<const uint4*>(p); }
  __device__ static inline void cvt(const raw& t, float (&v)[8]) {
    const half2_t a = __builtin_bit_cast(half2_t, t.x), b = __builtin_bit_cast(half2_t, t.y);
    const half2_t c = __builtin_bit_cast(half2_t, t.z), d = __builtin_bit_cast(half2_t, t.w);
    v[0] = (float)a[0]; v[1] = (float)a[1]; v[2] = (float)b[0]; v[3] = (float)b[1];
    v[4] = (float)c[0]; v[5] = (float)c[1]; v[6] = (float)d[0]; v[7] = (float)d[1];
  }
};

__host__ __device__ inline int lds_pad(int N) { return (N + 63) & ~63; }

struct TrajState {
  int cur, first;
  long long step_i;
  float used;
  float time;  // CVRPTW: current time
  bool done;
  uint32_t errbits;
  float ent_acc;
};

// One wave: compact the nodes this step has to read (ascending) into fl[0..F).
template <class Args>
__device__ inline int build_list(const Args& a, const uint8_t* mk, uint16_t* fl, int N, int lane) {
  int F = 0;
  if (a.mask_inner && a.mask_logits) {
    for (int j0 = 0; j0 < N; j0 += 64) {
      const int j = j0 + lane;
      const bool f = j < N && mk[j] != 0;
      const unsigned long long bal = __ballot(f);
      if (f) fl[F + __popcll(bal & ((1ull << lane) - 1ull))] = (uint16_t)j;
      F += __popcll(bal);
    }
  } else {
    for (int j = lane; j < N; j += 64) fl[j] = (uint16_t)j;
    F = N;
  }
  rl4co::lds_barrier_wave();
  return F;
}

}  // namespace

#endif

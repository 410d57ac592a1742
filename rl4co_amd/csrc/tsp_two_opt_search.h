// tsp_two_opt_search.h — the ONE text of the best-improvement 2-opt search on a tour held in LDS, shared by
// tsp_two_opt.hip (one search per tour) and tsp_nls.hip (a sequence of searches over two matrices per tour). The rules are
// the ones tsp_two_opt.hip's header states (association of `change`, the 64-bit key, the lowest (i, j) on ties, the double
// comparison against -1e-6, no barrier in divergent control flow); nothing here may change without that comment and the
// two-opt tests (CPU and GPU).
#pragma once

#include <hip/hip_runtime.h>

#include "common.h"

namespace rl4co {
namespace two_opt {

constexpr int kWaves = 4;
constexpr int kThreads = 64 * kWaves;
constexpr int kMaxTour = 1024;
constexpr int kCuLds = 160 * 1024;
constexpr int kRedBytes = 64;
constexpr int kTourBytes = 2 * kMaxTour;
constexpr int kStaticLds = 64;  // static LDS allowed beside the dynamic bytes (checked at launch)
constexpr uint64_t kNoPair = ~0ull;

enum Source { kMatrix = 0, kCoords = 1, kGlobal = 2 };

__host__ __device__ inline int64_t two_opt_lds_bytes(int src, int N) {
  return kRedBytes + kTourBytes + (src == kMatrix ? (int64_t)4 * N * N : src == kCoords ? (int64_t)8 * N : 0);
}

// order-preserving image of a float, ascending (NaN above everything)
__device__ inline uint32_t ord_key(float v) {
  if (v != v) return 0xffffffffu;
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ inline float ord_value(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// minimum of the 64-bit keys over the wave, in every lane
template <int S = 1>
__device__ inline uint64_t bfly_min_u64(uint64_t key) {
  if constexpr (S < 64) {
    const uint32_t oh = (uint32_t)rl4co::bfly_i<S>((int)(uint32_t)(key >> 32));
    const uint32_t ol = (uint32_t)rl4co::bfly_i<S>((int)(uint32_t)key);
    const uint64_t o = ((uint64_t)oh << 32) | ol;
    return bfly_min_u64<S * 2>(o < key ? o : key);
  } else {
    return key;
  }
}

__device__ inline float coord_distance(float2 pa, float2 pb) {
  const float dx = pa.x - pb.x;
  const float dy = pa.y - pb.y;
  return sqrtf(fmaf(dy, dy, dx * dx));
}

// d[a][b] of the instance with 1e9 added on the diagonal, from the template's source
template <int SRC>
struct Distances {
  const float* mat;     // kMatrix: LDS [N,N]; kGlobal: the instance's global [N,N]
  const float2* xy;     // kCoords: LDS [N]
  int N;
  __device__ inline float operator()(int a, int b) const {
    if constexpr (SRC == kMatrix) {
      return mat[a * N + b];
    } else if constexpr (SRC == kCoords) {
      return a == b ? 1e9f : coord_distance(xy[a], xy[b]);
    } else {
      return mat[a * N + b] + (a == b ? 1e9f : 0.0f);
    }
  }
};

// kMatrix staging: the instance's N x N matrix with its 1e9 diagonal into LDS `payload`, built from the coordinates `xy`
// [N] or loaded (coalesced) from the global matrix `g` [N,N]. The caller's workgroup barrier follows.
__device__ inline void stage_matrix_from_locs(float* payload, const float2* xy, int N, int tid) {
  const int nn = N * N;
  for (int e = tid; e < nn; e += kThreads) {
    const int p = e / N, q = e - p * N;
    payload[e] = p == q ? 1e9f : coord_distance(xy[p], xy[q]);
  }
}

__device__ inline void stage_matrix_from_distances(float* payload, const float* g, int N, int tid) {
  const int nn = N * N;
  for (int e = tid; e < nn; e += kThreads) {
    const int p = e / N, q = e - p * N;
    payload[e] = g[e] + (p == q ? 1e9f : 0.0f);
  }
}

// The search: scans of the pair list until the best change is not below -1e-6 or `max_iterations` scans ran; returns the
// number of scans (the last, non-improving one included). EVERY thread of the workgroup calls it with the same arguments;
// `tour` [T] (LDS) and the distances are in place behind a workgroup barrier of the caller's, `red` [kWaves] is LDS scratch.
// On return the tour is final and visible to every thread. The caller puts a workgroup barrier between two calls (red[] is
// read after the last barrier in here).
template <int SRC>
__device__ inline int search(const Distances<SRC>& dist, uint16_t* tour, uint64_t* red, int T, int max_iterations, int tid) {
  const int last = T - 1;  // pairs 1 <= i < j <= last; row i of the pair list holds j = i + 1 .. last
  int it = 0;
  while (it < max_iterations) {
    uint64_t best = kNoPair;
    // pair `tid` of the list, then every 256th: (i, j) advanced over the row ends
    int i = 1, j = 2 + tid;
    for (;;) {
      while (i < last && j > last) {
        j -= last - i - 1;  // (j - last - 1) past the row's end = the offset behind i + 2, the next row's first j
        ++i;
      }
      if (i >= last) break;
      const int ni = tour[i], nj = tour[j], np = tour[i - 1], nn = tour[j == last ? 0 : j + 1];
      if (np != nj && nn != ni) {
        const float change = ((dist(np, nj) + dist(ni, nn)) - dist(np, ni)) - dist(nj, nn);
        if (change < 0.0f) {
          const uint64_t key = ((uint64_t)ord_key(change) << 32) | (uint32_t)((i << 16) | j);
          best = key < best ? key : best;
        }
      }
      j += kThreads;
    }
    best = bfly_min_u64(best);
    if ((tid & 63) == 0) red[tid >> 6] = best;
    __syncthreads();
    uint64_t win = red[0];
    for (int w = 1; w < kWaves; ++w) win = red[w] < win ? red[w] : win;
    ++it;
    // every thread holds the same `win` (the same four LDS words, the same fold): a uniform decision
    if (win == kNoPair || !((double)ord_value((uint32_t)(win >> 32)) < -1e-6)) break;
    const int wi = (int)((uint32_t)win >> 16), wj = (int)((uint32_t)win & 0xffffu);
    const int half = (wj - wi + 1) >> 1;
    for (int k = tid; k < half; k += kThreads) {
      const uint16_t lo = tour[wi + k], hi = tour[wj - k];
      tour[wi + k] = hi;
      tour[wj - k] = lo;
    }
    __syncthreads();  // the reversal is in place before the next scan; red[] is rewritten only behind this barrier
  }
  return it;
}

}  // namespace two_opt
}  // namespace rl4co

// lds_tour_reward.h — minus the closed length of a tour held in LDS, computed by one wave: tour_length.hip's
// arithmetic RESTATED in the same order (ATen's vector_norm over two elements, then SumKernel's 8-lane / 4-ILP / 4-level
// cascade; lanes 0..7 of the wave play the SIMD lanes). The expression text is kept equal to that file's TourView::seg,
// lane_row_sum and kernel epilogue — change both together. Bit-equal to TSPEnv.get_reward / rl4co_tour_length_f32 (tested
// through aco_tsp.hip, tsp_nls.hip and aco_cvrp.hip; aco_cvrp.hip passes [depot, actions] with n = W + 1:
// rl4co_tour_length_f32 with prepend_depot on the W-wide row). aco_prize.hip also sums other terms in the same order.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rl4co {

struct AntTour {
  const uint16_t* tour;  // [n] in LDS
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

// `Terms` is any view with `n` terms and `seg(t)`, term t: AntTour's segments, or (aco_prize.hip) a vector gathered along a row
template <typename Terms>
__device__ inline float lane_row_sum(const Terms& tv, int lane8, int nvec) {
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
    for (int k = 0; k < kIlp; ++k) acc[0][k] = acc[0][k] + acc[j][k];
  for (int v = size * kIlp; v < nvec; ++v) acc[0][0] = acc[0][0] + tv.seg(8 * v + lane8);
  for (int k = 1; k < kIlp; ++k) acc[0][0] = acc[0][0] + acc[0][k];
  return acc[0][0];
}

// minus the closed tour length, valid in lane 0; the whole wave calls it (tour_length_kernel's body for one trajectory)
template <typename Terms>
__device__ inline float ant_reward(const Terms& tv, int lane) {
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

}  // namespace rl4co

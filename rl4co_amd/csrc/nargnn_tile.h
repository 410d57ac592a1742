// nargnn_tile.h — what the two heatmap-encoder kernels (nargnn.hip: the regular TSP graph; nargnn_depot.hip: the depot graph
// of CVRP, OP and PCTSP) share: the 68-float row, the fp32 MFMA tile product and the four node GEMMs' building block.
//
// MFMA v_mfma_f32_16x16x4_f32, operands as csrc/enc_f32.h states them: lane = 16 g + c holds A[row c][k-slot g] and
// B[k-slot g][col c]; a lane's 16-byte fragment (k = 16 j + 4 g .. + 3) feeds four steps, component s of both operands in
// step s. B is the weight row-major as torch keeps it ([out][in]): lane (c, g) of column tile ct reads
// W[16 ct + c][16 j + 4 g ..]. A wave holds one matrix (16 fragments, 64 VGPRs) for all of its row tiles. D[row 4 g + r]
// [col 16 ct + c] arrives in register r of accumulator ct. The sum over the 64 inputs is the hardware's (16 steps of 4).
#pragma once
#include <hip/hip_runtime.h>

namespace rl4co {
namespace nargnn {

constexpr int kD = 64;
constexpr int kRS = kD + 4;  // a row of 68 floats: the 16 lanes of one g read 16 distinct bank quads

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ inline float sigmoidf(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ inline float siluf(float x) { return x / (1.0f + expf(-x)); }

__device__ inline f32x4 mfma4(float a, float b, const f32x4& c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// the wave's copy of one 64 x 64 weight, row-major [out][in]: fragment [ct][j] of lane (c, g) is W[16 ct + c][16 j + 4 g ..]
__device__ inline void load_wfrags(f32x4 (&wf)[4][4], const float* W, int lane) {
  const float* row = W + (lane & 15) * kD + 4 * (lane >> 4);
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
#pragma unroll
    for (int j = 0; j < 4; ++j) wf[ct][j] = *reinterpret_cast<const f32x4*>(row + 16 * ct * kD + 16 * j);
}

// acc[ct] = (16 rows) . W^T for the four column tiles; `arow` is the lane's row c at float 4 g
__device__ inline void gemm_tile(f32x4 (&acc)[4], const f32x4 (&wf)[4][4], const float* arow) {
  f32x4 a[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) a[j] = *reinterpret_cast<const f32x4*>(arow + 16 * j);
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) acc[ct] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) acc[ct] = mfma4(a[j][s], wf[ct][j][s], acc[ct]);
}

// Y[n] = X[n] . W^T + bias for the node tiles tile0, tile0 + 2, ...
__device__ inline void node_gemm(float* Y, const float* X, const float* W, const float* bias, int N, int tile0, int lane) {
  const int c = lane & 15, g = lane >> 4;
  f32x4 wf[4][4];
  load_wfrags(wf, W, lane);
  float bcol[4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) bcol[ct] = bias[16 * ct + c];
  const int tiles = (N + 15) >> 4;
  for (int t = tile0; t < tiles; t += 2) {
    const int row = min(16 * t + c, N - 1);  // rows past N repeat the last node and are not stored
    f32x4 acc[4];
    gemm_tile(acc, wf, X + row * kRS + 4 * g);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = 16 * t + 4 * g + r;
      if (n < N) {
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) Y[n * kRS + 16 * ct + c] = acc[ct][r] + bcol[ct];
      }
    }
  }
}

}  // namespace nargnn
}  // namespace rl4co

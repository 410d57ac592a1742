// nargnn_logz.hip — GFACS's log-partition head (the reference's models/zoo/gfacs/encoder.py:45-47, 62) on the edge state the
// train-mode GNN stack leaves (nargnn_train.hip), forward and backward, for gfx950, fp32:
//   score[r] = W2 silu(W1 w[r] + b1) + b2        for every edge row r of the batch, rows = B E, Z = 1 or 2 outputs
//   logZ[b]  = mean of score over b's group      REFERENCE: the rows r with r % B == b (encoder.py:62 read literally: the
//                                                reshape(-1, B, Z) strides over the instances); INSTANCE: b's own E rows
// The C contract is in include/rl4co_amd.h (rl4co_nargnn_logz_args); the MFMA tile product and its operand convention are
// nargnn_shared.h's, the split of the rows over workgroups and waves is nargnn_train.hip's: four waves a workgroup, rows cut
// into P = min(ceil(rows / 64), 1024) workgroups, each of the 4 P waves a contiguous run of 16-row tiles.
//
// Forward (2 launches):
//   scores  W1 is staged in LDS once per workgroup (rows of 68 floats) and every wave takes its 16 fragments from there; per
//           tile the 16 x 64 hidden arrives in the accumulators, SiLU and the 64 -> Z product run on them in registers (a
//           lane's four columns, then the butterfly over the 16 lanes of a row) and lane 0 of a row stores its Z scores.
//           The hidden never goes to memory.
//   pool    one workgroup of 256 threads per instance: thread t sums the group's terms t, t + 256, ... in that order, the
//           256 sums are halved 128, 64, ... in LDS, all in float64. The order depends on (B, E, the rule) alone, never on
//           the grid; with B = 1 the two rules walk the same rows, so their results are the same bits.
// Backward (2 launches), ds[r] = grad_logZ[group of r] / E:
//   bwd       the hidden is recomputed per tile; dpre = (ds W2) silu'(pre) goes through a 16 x 68 LDS tile of the wave into
//             the A layout; grad_w = dpre W1 (MFMA, the transposed fragments), dW1 += dpre^T w (MFMA, the tile's rows are
//             the k dimension), db1, dW2 = ds^T h and db2 in float64 per lane; the four waves' sums are added wave 0 first
//             and written as one partial per workgroup
//   finalize  the partials in ascending order, float64
// No floating-point atomic, no grid barrier: every sum has a fixed order and every output is bit-identical run to run.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.h"
#include "nargnn_shared.h"
#include "rl4co_math.h"

namespace {

using namespace rl4co::nargnn;

constexpr int kT = 256;          // threads of a workgroup
constexpr int kW = kT / 64;      // waves
constexpr int kMaxGroups = 1024;
constexpr int kZ = 2;            // the widest head
constexpr int kMaxRows = 1 << 24;
constexpr int kPart = kD * kD + kD + kZ * kD + kZ;  // one workgroup's partial: dW1 [64][64], db1 [64], dW2 [2][64], db2 [2]

__device__ inline float sigm(float x) { return 1.0f / (1.0f + rl4co_expf(-x)); }
__device__ inline float silu(float x) { return x / (1.0f + rl4co_expf(-x)); }

inline int groups_of(int64_t rows) { return (int)std::min<int64_t>((rows + 63) / 64, kMaxGroups); }
inline int tiles_per_wave(int64_t rows, int P) {
  const int64_t tiles = (rows + 15) / 16, waves = (int64_t)kW * P;
  return (int)((tiles + waves - 1) / waves);
}
// the workspace (floats): the scores [rows][2], then the backward's partials [P][kPart]
inline int64_t workspace_floats(int64_t rows) { return kZ * rows + (int64_t)groups_of(rows) * kPart; }

// fragment [ct][j] of lane (c, g) from W staged in LDS in rows of kRS floats: W[16 ct + c][16 j + 4 g ..]
__device__ inline void load_wfrags_lds(f32x4 (&wf)[4][4], const float* W, int lane) {
  const float* row = W + (lane & 15) * kRS + 4 * (lane >> 4);
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
#pragma unroll
    for (int j = 0; j < 4; ++j) wf[ct][j] = *reinterpret_cast<const f32x4*>(row + 16 * ct * kRS + 16 * j);
}
// the transposed fragments from global memory (nargnn_train.hip's): gemm_tile with them gives (16 rows) . W
__device__ inline void load_wfrags_t(f32x4 (&wf)[4][4], const float* W, int lane) {
  const int c = lane & 15, g = lane >> 4;
#pragma unroll
  for (int ct = 0; ct < 4; ++ct)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int s = 0; s < 4; ++s) wf[ct][j][s] = W[(16 * j + 4 * g + s) * kD + 16 * ct + c];
}
__device__ inline void stage_w1(float* sW1, const float* W1) {
  for (int at = threadIdx.x; at < kD * (kD / 4); at += kT) {
    const int row = at >> 4, q = at & 15;
    *reinterpret_cast<f32x4*>(sW1 + row * kRS + 4 * q) = *reinterpret_cast<const f32x4*>(W1 + row * kD + 4 * q);
  }
  __syncthreads();
}

struct HeadArgs {
  const float *w, *W1, *b1, *W2, *b2;
  float* scores;        // forward: [rows][Z]
  const float* gz;      // backward: grad_logZ [B][Z]
  float *gw, *part;     // backward: grad_w [rows][64], [P][kPart]
  int64_t rows;
  int tpw, B, E, Z, pooling;
};

// ---- forward --------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kT) k_logz_scores(const HeadArgs a) {
  __shared__ __attribute__((aligned(16))) float sW1[kD * kRS];
  const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  const int64_t wg = (int64_t)blockIdx.x * kW + (threadIdx.x >> 6);
  stage_w1(sW1, a.W1);
  f32x4 wf[4][4];
  load_wfrags_lds(wf, sW1, lane);
  float b1c[4], w2c[kZ][4];
#pragma unroll
  for (int ct = 0; ct < 4; ++ct) {
    b1c[ct] = a.b1[16 * ct + c];
    w2c[0][ct] = a.W2[16 * ct + c];
    w2c[1][ct] = a.Z > 1 ? a.W2[kD + 16 * ct + c] : 0.0f;
  }
  const float b20 = a.b2[0], b21 = a.Z > 1 ? a.b2[1] : 0.0f;
  const int64_t tiles = (a.rows + 15) >> 4;
  const int64_t t1 = min(tiles, (wg + 1) * a.tpw);
  for (int64_t t = wg * a.tpw; t < t1; ++t) {
    const int64_t row = min(16 * t + c, a.rows - 1);  // rows past the end repeat the last one and are not stored
    f32x4 acc[4];
    gemm_tile(acc, wf, a.w + row * kD + 4 * g);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float s0 = 0.0f, s1 = 0.0f;
#pragma unroll
      for (int ct = 0; ct < 4; ++ct) {
        const float h = silu(acc[ct][r] + b1c[ct]);
        s0 += h * w2c[0][ct];
        s1 += h * w2c[1][ct];
      }
      s0 = rl4co::bfly_sum<1, 16>(s0);  // the 16 lanes of row 4 g + r
      s1 = rl4co::bfly_sum<1, 16>(s1);
      const int64_t n = 16 * t + 4 * g + r;
      if (c == 0 && n < a.rows) {
        a.scores[n * a.Z] = s0 + b20;
        if (a.Z > 1) a.scores[n * a.Z + 1] = s1 + b21;
      }
    }
  }
}

__global__ void __launch_bounds__(kT) k_logz_pool(const HeadArgs a, float* logZ) {
  __shared__ double sh[kZ][kT];
  const int b = blockIdx.x, tid = threadIdx.x;
  const bool strided = a.pooling == RL4CO_LOGZ_POOL_REFERENCE;
  const int64_t first = strided ? b : (int64_t)b * a.E, step = strided ? a.B : 1;
  double s0 = 0.0, s1 = 0.0;
  for (int t = tid; t < a.E; t += kT) {
    const float* p = a.scores + (first + (int64_t)t * step) * a.Z;
    s0 += (double)p[0];
    if (a.Z > 1) s1 += (double)p[1];
  }
  sh[0][tid] = s0;
  sh[1][tid] = s1;
  __syncthreads();
  for (int half = kT / 2; half > 0; half >>= 1) {
    if (tid < half) {
      sh[0][tid] += sh[0][tid + half];
      sh[1][tid] += sh[1][tid + half];
    }
    __syncthreads();
  }
  if (tid < a.Z) logZ[b * a.Z + tid] = (float)(sh[tid][0] / (double)a.E);
}

// ---- backward -------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kT) k_logz_bwd(const HeadArgs a) {
  __shared__ float sdw[kD * kD];
  __shared__ __attribute__((aligned(16))) float stile[kW][16 * kRS];
  __shared__ double sdb[kW][4][kD];
  __shared__ double sdw2[kW][4][kZ][kD];
  __shared__ double sdb2[kW][4][kZ];
  const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
  const int w = threadIdx.x >> 6;
  const int64_t wg = (int64_t)blockIdx.x * kW + w;
  float* tile = stile[w];
  f32x4 dw[4][4];
  double db[4], dw2[kZ][4], db2[kZ] = {0.0, 0.0};
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    db[mt] = 0.0;
    dw2[0][mt] = dw2[1][mt] = 0.0;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) dw[mt][nt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
  }
  {
    f32x4 wf[4][4], wft[4][4];
    load_wfrags(wf, a.W1, lane);
    load_wfrags_t(wft, a.W1, lane);
    float b1c[4], w2c[kZ][4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
      b1c[ct] = a.b1[16 * ct + c];
      w2c[0][ct] = a.W2[16 * ct + c];
      w2c[1][ct] = a.Z > 1 ? a.W2[kD + 16 * ct + c] : 0.0f;
    }
    const float count = (float)a.E;
    const int64_t tiles = (a.rows + 15) >> 4;
    const int64_t t1 = min(tiles, (wg + 1) * a.tpw);
    for (int64_t t = wg * a.tpw; t < t1; ++t) {
      const int64_t row = min(16 * t + c, a.rows - 1);
      f32x4 acc[4];
      gemm_tile(acc, wf, a.w + row * kD + 4 * g);
      // dpre of the tile's rows, in the accumulators' layout, into the wave's LDS tile; a row past the end holds zeros
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t n = 16 * t + 4 * g + r;
        float ds0 = 0.0f, ds1 = 0.0f;
        if (n < a.rows) {
          const int64_t grp = a.pooling == RL4CO_LOGZ_POOL_REFERENCE ? n % a.B : n / a.E;
          ds0 = a.gz[grp * a.Z] / count;
          if (a.Z > 1) ds1 = a.gz[grp * a.Z + 1] / count;
        }
        db2[0] += (double)ds0;
        db2[1] += (double)ds1;
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
          const float p = acc[ct][r] + b1c[ct], sg = sigm(p);
          const float h = p * sg;
          dw2[0][ct] += (double)(ds0 * h);
          dw2[1][ct] += (double)(ds1 * h);
          const float dh = ds0 * w2c[0][ct] + ds1 * w2c[1][ct];
          tile[(4 * g + r) * kRS + 16 * ct + c] = dh * (sg * (1.0f + p * (1.0f - sg)));
        }
      }
      rl4co::lds_barrier_wave();  // written in one lane layout, read in two others, by this wave only
      // grad_w = dpre . W1
      f32x4 gw[4];
      gemm_tile(gw, wft, tile + c * kRS + 4 * g);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t n = 16 * t + 4 * g + r;
        if (n < a.rows) {
#pragma unroll
          for (int ct = 0; ct < 4; ++ct) a.gw[n * kD + 16 * ct + c] = gw[ct][r];
        }
      }
      // dW1[n][k] += sum over the tile's rows of dpre[row][n] w[row][k]: the rows are the MFMA's k dimension, four a step
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int64_t rr = 16 * t + 4 * s + g;
        const bool ok = rr < a.rows;
        const int64_t at = (ok ? rr : 0) * kD + c;
        float av[4], bv[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          av[q] = tile[(4 * s + g) * kRS + c + 16 * q];
          bv[q] = ok ? a.w[at + 16 * q] : 0.0f;
          db[q] += (double)av[q];
        }
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
          for (int nt = 0; nt < 4; ++nt) dw[mt][nt] = mfma4(av[mt], bv[nt], dw[mt][nt]);
      }
      rl4co::lds_barrier_wave();  // the tile is rewritten by the next one
    }
  }
  // the four waves' sums, wave 0 first
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    sdb[w][g][16 * mt + c] = db[mt];
    sdw2[w][g][0][16 * mt + c] = dw2[0][mt];
    sdw2[w][g][1][16 * mt + c] = dw2[1][mt];
  }
  if (c == 0) {  // (every lane of a row holds the same sum)
    sdb2[w][g][0] = db2[0];
    sdb2[w][g][1] = db2[1];
  }
  for (int turn = 0; turn < kW; ++turn) {
    if (w == turn) {
#pragma unroll
      for (int mt = 0; mt < 4; ++mt)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int at = (16 * mt + 4 * g + r) * kD + 16 * nt + c;
            sdw[at] = turn == 0 ? dw[mt][nt][r] : sdw[at] + dw[mt][nt][r];
          }
    }
    __syncthreads();
  }
  float* part = a.part + (int64_t)blockIdx.x * kPart;
  for (int at = threadIdx.x; at < kD * kD; at += kT) part[at] = sdw[at];
  if (threadIdx.x < kD) {
    double s = 0.0, u0 = 0.0, u1 = 0.0;
    for (int ww = 0; ww < kW; ++ww)
      for (int gg = 0; gg < 4; ++gg) {
        s += sdb[ww][gg][threadIdx.x];
        u0 += sdw2[ww][gg][0][threadIdx.x];
        u1 += sdw2[ww][gg][1][threadIdx.x];
      }
    part[kD * kD + threadIdx.x] = (float)s;
    part[kD * kD + kD + threadIdx.x] = (float)u0;
    part[kD * kD + 2 * kD + threadIdx.x] = (float)u1;
  }
  if (threadIdx.x < kZ) {
    double s = 0.0;
    for (int ww = 0; ww < kW; ++ww)
      for (int gg = 0; gg < 4; ++gg) s += sdb2[ww][gg][threadIdx.x];
    part[kD * kD + kD + kZ * kD + threadIdx.x] = (float)s;
  }
}

struct FinalArgs {
  const float* part;  // [P][kPart]
  int P, Z;
  float *gW1, *gb1, *gW2, *gb2;
};
__global__ void __launch_bounds__(kT) k_logz_finalize(const FinalArgs a) {
  const int at = blockIdx.x * kT + threadIdx.x;
  if (at >= kPart) return;
  double s = 0.0;
  for (int p = 0; p < a.P; ++p) s += (double)a.part[(int64_t)p * kPart + at];
  const int w2 = at - (kD * kD + kD), b2 = w2 - kZ * kD;
  if (at < kD * kD) a.gW1[at] = (float)s;
  else if (w2 < 0) a.gb1[at - kD * kD] = (float)s;
  else if (b2 < 0) {
    if (w2 < a.Z * kD) a.gW2[w2] = (float)s;
  } else if (b2 < a.Z) a.gb2[b2] = (float)s;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
int require_common(const rl4co_nargnn_logz_args& a) {
  RL4CO_REQUIRE(a.Z == 1 || a.Z == 2);
  RL4CO_REQUIRE(a.rows == (int64_t)a.B * a.E);
  RL4CO_REQUIRE(a.w != nullptr && a.W1 != nullptr && a.b1 != nullptr && a.W2 != nullptr && a.b2 != nullptr);
  RL4CO_REQUIRE(a.workspace != nullptr);
  RL4CO_REQUIRE(a.rows >= 1 && a.B >= 1 && a.E >= 1);
  RL4CO_REQUIRE(a.rows <= kMaxRows);  // the stack's own limit: row counts are exact in fp32
  RL4CO_REQUIRE(a.pooling == RL4CO_LOGZ_POOL_REFERENCE || a.pooling == RL4CO_LOGZ_POOL_INSTANCE);
  RL4CO_REQUIRE(a.workspace_bytes >= workspace_floats(a.rows) * 4);
  const uintptr_t all = reinterpret_cast<uintptr_t>(a.w) | reinterpret_cast<uintptr_t>(a.W1) | reinterpret_cast<uintptr_t>(a.workspace);
  RL4CO_REQUIRE((all & 15) == 0);  // 16-byte fragments
  return RL4CO_OK;
}

HeadArgs head_args(const rl4co_nargnn_logz_args& a, int P) {
  HeadArgs h{};
  h.w = a.w, h.W1 = a.W1, h.b1 = a.b1, h.W2 = a.W2, h.b2 = a.b2;
  h.scores = a.workspace;
  h.part = a.workspace + kZ * a.rows;
  h.rows = a.rows, h.tpw = tiles_per_wave(a.rows, P), h.B = a.B, h.E = a.E, h.Z = a.Z, h.pooling = a.pooling;
  return h;
}

}  // namespace

extern "C" int64_t rl4co_nargnn_logz_workspace_bytes(int64_t rows) {
  return rows < 1 || rows > kMaxRows ? 0 : workspace_floats(rows) * 4;
}

extern "C" int rl4co_nargnn_logz_forward(const rl4co_nargnn_logz_args* args, void* stream) {
  RL4CO_REQUIRE(args != nullptr);
  const rl4co_nargnn_logz_args& a = *args;
  if (const int rc = require_common(a)) return rc;
  RL4CO_REQUIRE(a.logZ != nullptr);
  hipStream_t s = rl4co::as_stream(stream);
  const int P = groups_of(a.rows);
  const HeadArgs h = head_args(a, P);
  hipLaunchKernelGGL(k_logz_scores, dim3(P), dim3(kT), 0, s, h);
  hipLaunchKernelGGL(k_logz_pool, dim3(a.B), dim3(kT), 0, s, h, a.logZ);
  RL4CO_HIP_TRY(hipGetLastError());
  return RL4CO_OK;
}

extern "C" int rl4co_nargnn_logz_backward(const rl4co_nargnn_logz_args* args, void* stream) {
  RL4CO_REQUIRE(args != nullptr);
  const rl4co_nargnn_logz_args& a = *args;
  if (const int rc = require_common(a)) return rc;
  RL4CO_REQUIRE(a.grad_logZ != nullptr && a.grad_w != nullptr);
  RL4CO_REQUIRE(a.grad_W1 != nullptr && a.grad_b1 != nullptr && a.grad_W2 != nullptr && a.grad_b2 != nullptr);
  RL4CO_REQUIRE((reinterpret_cast<uintptr_t>(a.grad_w) & 15) == 0);
  hipStream_t s = rl4co::as_stream(stream);
  const int P = groups_of(a.rows);
  HeadArgs h = head_args(a, P);
  h.gz = a.grad_logZ, h.gw = a.grad_w;
  hipLaunchKernelGGL(k_logz_bwd, dim3(P), dim3(kT), 0, s, h);
  FinalArgs f{h.part, P, a.Z, a.grad_W1, a.grad_b1, a.grad_W2, a.grad_b2};
  hipLaunchKernelGGL(k_logz_finalize, dim3((kPart + kT - 1) / kT), dim3(kT), 0, s, f);
  RL4CO_HIP_TRY(hipGetLastError());
  return RL4CO_OK;
}

// tsp_two_opt.hip — TSP local search: best-improvement 2-opt (envs/routing/tsp/local_search.py) as one launch for gfx950.
//
// One workgroup of four waves per TOUR runs the whole search of that tour: per iteration the arg-min of `change` over the
// (T-1)(T-2)/2 position pairs 1 <= i < j <= T-1 and, when the winner is below -1e-6, the reversal of tour[i..j]; it ends
// at the first iteration without such a move or at max_iterations. The answer is fully determined — the reference's
// sequential scan keeps the FIRST pair of the smallest change — and the kernel reproduces it bit for bit:
//   change   ((d[prev][tour[j]] + d[tour[i]][next]) - d[prev][tour[i]]) - d[tour[j]][next], prev = tour[i-1],
//            next = tour[(j+1) % T]: fp32, one rounding per operation, this association, this index order (an asymmetric
//            matrix is served), -ffp-contract=off. A pair with prev == tour[j] or next == tour[i] is skipped.
//   winner   the lexicographically smallest (change, i, j) among the pairs with change < 0 (NaN and -0.0 are not below 0).
//            Each thread keeps the minimum of a 64-bit key: the order-preserving image of `change` (NaN above everything)
//            in the high word, (i << 16) | j in the low word, so equal changes go to the lowest (i, j) however the pairs
//            are dealt. Pairs are dealt flat: thread k takes pairs k, k + 256, ... of the (i, j)-ordered list.
//   reduce   wave butterfly (common.h), lane 0 of each wave stores its key, workgroup barrier, EVERY thread reads the same
//            four LDS words and folds them in the same order: the move / stop decision is uniform by construction.
//   move     widened to double, change < -1e-6 (the reference compares in double): threads k < (j - i + 1) / 2 swap
//            tour[i + k] and tour[j - k]; workgroup barrier; next iteration. `iterations` counts the last, non-improving
//            scan too. No barrier sits inside divergent control flow; the only loop is bounded by max_iterations.
//
// Distances (one kernel template over the three sources, one text of the search loop):
//   kMatrix   N <= rl4co_tsp_two_opt_lds_nodes(): the N x N fp32 matrix of the instance in LDS, 1e9 added on its diagonal —
//             built by the workgroup from `locs`, or staged once from `distances` with coalesced loads.
//   kCoords   above that, from `locs`: the coordinates in LDS (8 N bytes), every d[a][b] computed where it is used.
//   kGlobal   above that, from `distances`: entries read from global memory (the caches serve the re-reads).
//   From coordinates d[a][b] = sqrtf(fmaf(dy, dy, dx * dx)), dx = x_a - x_b, dy = y_a - y_b: the expression of
//   tour_length.hip, bit-identical to ATen's norm(p=2) over two elements, in kMatrix and kCoords alike; d[a][a] = 1e9.
//
// A tour holding an index outside [0, N) raises RL4CO_EBIT_TOUR_INDEX and is copied through unchanged with 0 iterations:
// the index is only compared, nothing is read through it.
//
// LDS budget (bytes, all dynamic; the kernel declares no static LDS and the launcher checks that the compiler added none
// beyond kStaticLds):
//   reduction scratch    64             (four 64-bit wave keys, the bad-index flag)
//   tour                 2 * 1024       (uint16_t, T <= 1024)
//   distances            4 N^2 (kMatrix) | 8 N (kCoords) | 0 (kGlobal)
//   static               <= 64
//   4 N^2 + 2 * 1024 + 64 + 64 <= 160 KiB  =>  N <= 201 (4 * 201^2 = 161 604): rl4co_tsp_two_opt_lds_nodes().
// Design estimates, NOT measured: at N = 100 a workgroup takes 42 112 B of LDS, so three workgroups (12 waves) share a
// CU; above N = 142 (80 KiB) one workgroup per CU. Nothing about this kernel's occupancy or time has been profiled
// (tools/two_opt_bench.py records the end-to-end time only).
#include <hip/hip_runtime.h>

#include "common.h"

namespace {

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

template <int SRC>
__global__ void __launch_bounds__(kThreads) tsp_two_opt_kernel(const rl4co_tsp_two_opt_args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint64_t* red = reinterpret_cast<uint64_t*>(smem);                   // [kWaves]
  uint32_t* bad_flag = reinterpret_cast<uint32_t*>(smem + 8 * kWaves);
  uint16_t* tour = reinterpret_cast<uint16_t*>(smem + kRedBytes);      // [T]
  float* payload = reinterpret_cast<float*>(smem + kRedBytes + kTourBytes);

  const int tid = threadIdx.x;
  const int N = a.N, T = a.T;
  const int64_t row = (int64_t)blockIdx.x * T;
  const int64_t* in = a.actions + row;
  int64_t* out = a.out_actions + row;

  // ---- the tour: range check, then uint16_t in LDS -----------------------------------------------------------------
  if (tid == 0) *bad_flag = 0u;
  __syncthreads();
  bool bad = false;
  for (int t = tid; t < T; t += kThreads) {
    const int64_t v = in[t];
    if (v < 0 || v >= N) bad = true;
    tour[t] = (uint16_t)v;
  }
  if (bad) *bad_flag = 1u;
  __syncthreads();
  if (*bad_flag) {  // (uniform: one LDS word) the tour goes through as it came; every thread moves its own elements
    if (out != in)
      for (int t = tid; t < T; t += kThreads) out[t] = in[t];
    if (tid == 0) {
      if (a.iterations) a.iterations[blockIdx.x] = 0;
      atomicOr(a.err, RL4CO_EBIT_TOUR_INDEX);
    }
    return;
  }

  // ---- the distances ----------------------------------------------------------------------------------------------
  Distances<SRC> dist;
  dist.N = N;
  dist.mat = nullptr;
  dist.xy = nullptr;
  if constexpr (SRC == kMatrix) {
    const int nn = N * N;
    if (a.locs) {
      const float2* xy = reinterpret_cast<const float2*>(a.locs) + (int64_t)blockIdx.x * N;
      for (int e = tid; e < nn; e += kThreads) {
        const int p = e / N, q = e - p * N;
        payload[e] = p == q ? 1e9f : coord_distance(xy[p], xy[q]);
      }
    } else {
      const float* g = a.distances + (int64_t)blockIdx.x * nn;
      for (int e = tid; e < nn; e += kThreads) {
        const int p = e / N, q = e - p * N;
        payload[e] = g[e] + (p == q ? 1e9f : 0.0f);
      }
    }
    dist.mat = payload;
  } else if constexpr (SRC == kCoords) {
    const float2* xy = reinterpret_cast<const float2*>(a.locs) + (int64_t)blockIdx.x * N;
    float2* lxy = reinterpret_cast<float2*>(payload);
    for (int e = tid; e < N; e += kThreads) lxy[e] = xy[e];
    dist.xy = lxy;
  } else {
    dist.mat = a.distances + (int64_t)blockIdx.x * N * N;
  }
  __syncthreads();

  // ---- the search -------------------------------------------------------------------------------------------------
  const int last = T - 1;  // pairs 1 <= i < j <= last; row i of the pair list holds j = i + 1 .. last
  int it = 0;
  while (it < a.max_iterations) {
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

  for (int t = tid; t < T; t += kThreads) out[t] = (int64_t)tour[t];
  if (tid == 0 && a.iterations) a.iterations[blockIdx.x] = it;
}

template <int SRC>
int launch(const rl4co_tsp_two_opt_args& a, hipStream_t stream) {
  const int lds = (int)two_opt_lds_bytes(SRC, a.N);
  hipFuncAttributes fa;
  RL4CO_HIP_TRY(hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(tsp_two_opt_kernel<SRC>)));
  RL4CO_REQUIRE((int64_t)fa.sharedSizeBytes <= kStaticLds);  // the budget of rl4co_tsp_two_opt_lds_nodes holds
  if (lds > 64 * 1024) {
    RL4CO_HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(tsp_two_opt_kernel<SRC>),
                                      hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  }
  hipLaunchKernelGGL((tsp_two_opt_kernel<SRC>), dim3(a.B), dim3(kThreads), lds, stream, a);
  RL4CO_HIP_TRY(hipGetLastError());
  return RL4CO_OK;
}

}  // namespace

extern "C" int rl4co_tsp_two_opt_lds_nodes(void) {
  int n = kMaxTour;
  while (n > 0 && two_opt_lds_bytes(kMatrix, n) + kStaticLds > kCuLds) --n;
  return n;
}

extern "C" int rl4co_tsp_two_opt(const rl4co_tsp_two_opt_args* args, void* stream) {
  RL4CO_REQUIRE(args != nullptr);
  const rl4co_tsp_two_opt_args& a = *args;
  RL4CO_REQUIRE(a.B >= 1);
  RL4CO_REQUIRE(a.N >= 2 && a.N <= 1024);
  RL4CO_REQUIRE(a.T >= 1 && a.T <= 1024);
  RL4CO_REQUIRE(a.max_iterations >= 0);
  RL4CO_REQUIRE((a.locs != nullptr) != (a.distances != nullptr));  // exactly one distance source
  RL4CO_REQUIRE(a.actions != nullptr);
  RL4CO_REQUIRE(a.out_actions != nullptr);
  RL4CO_REQUIRE(a.err != nullptr);
  hipStream_t s = rl4co::as_stream(stream);
  if (a.N <= rl4co_tsp_two_opt_lds_nodes()) return launch<kMatrix>(a, s);
  return a.locs ? launch<kCoords>(a, s) : launch<kGlobal>(a, s);
}

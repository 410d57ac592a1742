// ant_grad.h — what the two backward kernels of the ants' log-likelihoods (aco_tsp_grad.hip, aco_depot_grad.hip) share and
// can state once without a change to either kernel's generated text: the workgroup's (instance, part) split, the zeroing of
// a refused instance's rows and the KMAX launch ladder. A kernel keeps its step 1 (the table it builds and the refusals it
// decides), its choice of feasible sets and — because moving them reorders instructions — the row load, the
// masked-softmax contribution and the row store.
#pragma once

#include <type_traits>

#include "ant_system.h"

namespace rl4co::aco {

// Grid B x S: workgroup blockIdx.x is part s of instance b and takes the rows i = s (mod S), its waves alternating.
__device__ inline void grad_split(int S, int& b, int& s) {
  b = (int)(blockIdx.x / (unsigned)S);
  s = (int)(blockIdx.x - (unsigned)b * (unsigned)S);
}

// a refused instance's gradient is all zeros: this workgroup's rows of `gout` [N, N]
__device__ inline void grad_zero_rows(float* gout, int N, int s, int S, int w, int lane) {
  for (int i = s + S * w; i < N; i += S * kWaves)
    for (int n = lane; n < N; n += 64) gout[(int64_t)i * N + n] = 0.0f;
}

// ---- host side -------------------------------------------------------------------------------------------------------------
// KMAX = 1, 2, 4, 8 or 16 words per lane, N <= 64 KMAX: launch_kmax(std::integral_constant<int, KMAX>) launches the kernel
template <typename LaunchFn>
int grad_ladder(int N, LaunchFn launch_kmax) {
  const int K = (N + 63) >> 6;
  if (K <= 1) return launch_kmax(std::integral_constant<int, 1>{});
  if (K <= 2) return launch_kmax(std::integral_constant<int, 2>{});
  if (K <= 4) return launch_kmax(std::integral_constant<int, 4>{});
  if (K <= 8) return launch_kmax(std::integral_constant<int, 8>{});
  return launch_kmax(std::integral_constant<int, 16>{});
}

}  // namespace rl4co::aco

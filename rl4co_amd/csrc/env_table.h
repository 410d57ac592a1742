// env_table.h — host only: which builds serve an environment, stated once per RL4CO_ENV_*, and the two dispatchers that turn
// a runtime environment id / plane dtype into template arguments. The launchers of am_decode.hip, am_decode_ms.hip,
// am_decode_beam.hip, am_teacher.hip and am_teacher_mma.hip read it; they ask for an environment by name only where its
// required argument slots are stated (one literal RL4CO_REQUIRE per environment). envspec.py is the same statement for
// Python (kernels.beam_served, EnvSpec.unfold / .teacher). Adding an environment: a record here, its slots at the entries.
#ifndef RL4CO_ENV_TABLE_H
#define RL4CO_ENV_TABLE_H

#include <type_traits>

#include "common.h"

namespace rl4co {

struct EnvRecord {
  int env;          // RL4CO_ENV_*: its own index in kEnvTable
  bool decode;      // am_decode.hip: STREAM / LDS / WIDE
  bool ms;          // am_decode_ms.hip: multistart on the matrix cores
  bool stream_reg;  // RL4CO_VARIANT_STREAM_REG
  bool row_cache;   // the streaming kernels' LDS row cache: the "can still be listed" set is kept and only shrinks
  bool unfold;      // the unfolded parity mode of the streaming kernel
  bool beam;        // am_decode_beam.hip
  bool teacher;     // am_teacher.hip / am_teacher_mma.hip: the teacher-forced backward
  int ms_from;      // starts per instance from which auto picks MS; 0 = never chosen by auto
  bool one_acc16;   // 16-bit planes: one accumulator per load in the streaming kernel (the oracle's row groups)
};

// ms_from: auto picks MS where it was measured faster than one wave per trajectory (N = 100, 4096 instances, sampling, r02;
// M trajectory-steps/s MS vs STREAM): TSP 8 starts 667 vs 276; pickup-delivery 8 starts 633 vs 379; prize-collecting TSP 8
// starts 442 vs 178; CVRP 8 starts 254 vs 277 but 16 starts 463 vs 276 (a full 16-column tile). Orienteering (7-step
// ragged tours under random weights: 84 vs 162) and CVRP with time windows (111 vs 278: the per-step mask over all
// nodes with a square root each, replicated in every lane of the column) stay on STREAM unless MS is asked for.
// r03, with two instances per column tile at <= 8 starts (a launch then costs ~3.3 ms for 4096 instances whatever
// the start count; tools/ms_bench.py, sampling, 4096 x S): TSP 3 starts 3.26 vs 5.11 ms (2: 3.24 vs 3.59), prize-
// collecting TSP 3 starts 3.38 vs 5.09, pickup-delivery 3 starts 3.43 vs 3.64 (2: 3.42 vs 2.58 — STREAM), CVRP 8 starts
// 13.6 vs 14.3 (4: 13.3 vs 7.8 — STREAM: every column of a tile runs to the tile's longest tour).
// SDVRP: the dynamic embedding is in the decode kernels alone, and a visited node comes back (no row cache). mTSP: so are
// the four-scalar context and the min-max state.
constexpr EnvRecord kEnvTable[] = {
    //                 decode ms     reg    cache  unfold beam   teacher ms_from one_acc16
    {RL4CO_ENV_TSP,    true,  true,  true,  true,  true,  true,  true,   3,      false},
    {RL4CO_ENV_CVRP,   true,  true,  true,  true,  true,  true,  true,   8,      false},
    {RL4CO_ENV_OP,     true,  true,  false, false, false, false, true,   0,      false},
    {RL4CO_ENV_PCTSP,  true,  true,  false, false, false, false, true,   3,      false},
    {RL4CO_ENV_PDP,    true,  true,  false, false, false, false, true,   3,      false},
    {RL4CO_ENV_CVRPTW, true,  true,  false, false, false, false, true,   0,      false},
    {RL4CO_ENV_SDVRP,  true,  false, false, false, false, false, false,  0,      true},
    {RL4CO_ENV_MTSP,   true,  false, false, false, false, false, false,  0,      true},
};
constexpr int kNumEnvs = sizeof(kEnvTable) / sizeof(kEnvTable[0]);

constexpr bool env_table_in_order(int i = 0) { return i == kNumEnvs || (kEnvTable[i].env == i && env_table_in_order(i + 1)); }
static_assert(env_table_in_order(), "kEnvTable is indexed by RL4CO_ENV_*");

// The record of `env`; nullptr for an id that is no environment.
inline const EnvRecord* env_record(int env) { return env >= 0 && env < kNumEnvs ? &kEnvTable[env] : nullptr; }
// Does the build `by` (a bool of EnvRecord) serve `env`? No build serves an id that is no environment.
inline bool env_served(int env, bool EnvRecord::*by) { return env_record(env) != nullptr && env_record(env)->*by; }

// dispatch_env<&EnvRecord::ms>(a.env, f): calls f(std::integral_constant<int, ENV>) for the runtime `env` and returns its
// int. `f` is instantiated for the environments whose record has SERVED set and for no other: the column of the table is
// the list of kernels a launcher builds. An id outside it is an argument error, never a launch.
template <bool EnvRecord::*SERVED, int ENV = 0, class F>
int dispatch_env(int env, F&& f) {
  if constexpr (ENV == kNumEnvs) {
    return record_arg_error("no build of this kernel serves the environment");
  } else {
    if constexpr (kEnvTable[ENV].*SERVED) {
      if (env == ENV) return f(std::integral_constant<int, ENV>{});
    }
    return dispatch_env<SERVED, ENV + 1>(env, f);
  }
}

// A plane dtype with the element type that reads it (decode_wave.h), and dispatch_planes<PlanesBF16, PlanesF16>(dtype, f):
// calls f(P{}) for the P of the pack whose dtype it is (`typename decltype(p)::type` is the element type).
template <int DT, class C>
struct Planes : std::integral_constant<int, DT> {
  using type = C;
};
template <class P, class... REST, class F>
int dispatch_planes(int cache_dtype, F&& f) {
  if (cache_dtype == P::value) return f(P{});
  if constexpr (sizeof...(REST) > 0) {
    return dispatch_planes<REST...>(cache_dtype, f);
  } else {
    return record_arg_error("no build of this kernel reads the plane dtype");
  }
}

}  // namespace rl4co

#endif

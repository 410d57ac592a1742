// ant_rules.h — the depot environments' transition rules as the Ant System kernels execute them, stated once: the feasibility
// of a customer and of the depot, and the advance of the one fp32 word of state an ant carries (CVRP `used`, OP
// `tour_length`, PCTSP `cur_total_prize`). aco_cvrp.hip and aco_prize.hip (the sampling kernels) and aco_depot_grad.hip (their
// backward, which replays the rows and rebuilds each step's feasible set) call the same text, so the backward's mask IS the
// forward's. Every expression is part of the parity contract (-ffp-contract=off): one operation, one rounding, in this order.
#pragma once

#include <hip/hip_runtime.h>

namespace rl4co::aco {

// ---- CVRP (cvrp/env.py:66-136, env_step.hip's cvrp_step_body) -------------------------------------------------------------
// the right side of the capacity test: ONE fp32 add (cvrp/env.py:129)
__device__ inline float cvrp_threshold(float vehicle_capacity) { return vehicle_capacity + 1e-5f; }
// an unvisited customer of demand `demand` fits the load `used`
__device__ inline bool cvrp_fits(float demand, float used, float thr) { return !(demand + used > thr); }
// the load after action a of demand `demand` (the depot's word is the clamp's demand[0]); the depot empties the vehicle
__device__ inline float cvrp_advance(float used, float demand, int a) { return (used + demand) * (a != 0 ? 1.0f : 0.0f); }
// the depot is infeasible while the ant stands on it and some customer is feasible
__device__ inline bool cvrp_depot_ok(int cur, bool any_customer) { return !(cur == 0 && any_customer); }

// ---- OP (op/env.py:67-154, env_step.hip's op_step_body) ---------------------------------------------------------------------
// d(i, j) = sqrtf(fmaf(dy, dy, dx * dx)), dx = x_j - x_i, dy = y_j - y_i: torch's norm over a dim of two
__device__ inline float op_dist(float xi, float yi, float xj, float yj) {
  const float dx = xj - xi, dy = yj - yi;
  return sqrtf(fmaf(dy, dy, dx * dx));
}
// the tour length after walking `dist` (one fp32 add): the state's advance and the left side of the budget test
__device__ inline float op_advance(float tour_length, float dist) { return tour_length + dist; }
// an unvisited customer is within the budget: `reach` = op_advance(tour_length, d(cur, j)) against max_length[j]
__device__ inline bool op_within(float reach, float max_length) { return !(reach > max_length); }

// ---- PCTSP (pctsp/env.py:62-144, pctsp_step_body) -----------------------------------------------------------------------------
__device__ inline float pctsp_advance(float total_prize, float prize) { return total_prize + prize; }
// the depot is infeasible while the collected prize is below 1 and an unvisited customer remains
__device__ inline bool pctsp_depot_ok(float total_prize, int left) { return !(total_prize < 1.0f && left > 0); }

}  // namespace rl4co::aco

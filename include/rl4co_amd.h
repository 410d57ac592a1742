/*
 * rl4co_amd.h — C-ABI of the MI355X-native autoregressive rollout engine.
 *
 * This is the drop-in boundary for ONE hot path of ai4co/rl4co: the batched
 * TSP/CVRP environment step + AttentionModel decode loop + tour-length reward.
 * Every entry point below names the reference function(s) it replaces
 * (paths relative to the reference checkout, `rl4co/...:line`).
 *
 * Conventions
 *   - all pointers are DEVICE pointers into caller-owned buffers (the Python
 *     boundary hands in torch tensors' data_ptr()); the library allocates
 *     nothing persistent and keeps no threads;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream);
 *   - every function returns an int status (RL4CO_OK = 0) and never throws;
 *   - the reference raises Python `assert`s from inside the loop (one host
 *     sync each). Here those conditions are recorded as sticky bits
 *     OR-ed into the caller's `int32_t* err` word, which the host checks ONCE
 *     per rollout and converts back into the reference's assertion messages;
 *   - masks are uint8 with 1 = feasible (torch.bool storage), indices int64,
 *     payload float32 unless a dtype tag says otherwise.
 */
#ifndef RL4CO_AMD_H
#define RL4CO_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- ABI version ----------------------------------------------------------
 * Bumped whenever an exported signature or struct layout changes. A binding compares rl4co_abi_version() (what the
 * loaded library was built with) against the RL4CO_ABI_VERSION of the header it was written for and refuses to run on a
 * mismatch: a changed argument list under an unchanged symbol name still links (r05: rl4co_attn_bwd_* gained `out` in
 * second position — a caller built for the old list would pass dout as out and lse as dout).
 *   6: rl4co_attn_bwd_{bf16,f16} take the forward's `out`; rl4co_abi_version() itself.
 *   7: rl4co_am_decode_args / rl4co_am_teacher_args end in the context tables' dtype and strides (ctx_dtype ...).
 *   8: the 16 rl4co_<op>_bf16 / rl4co_<op>_f16 pairs are ONE rl4co_<op>(int dtype, ...) each.
 *  13: rl4co_am_decode_args ends in the top-k / top-p filter (top_k, top_p) and its optional kept-set output
 *      (kept_bits, kept_words); zero-initialised = no filter.
 *  14: rl4co_am_decode_args carries the split-delivery VRP's dynamic-embedding vectors and per-trajectory remaining
 *      demand (dyn_vectors, demand_state, behind w_time); rl4co_sdvrp_step.
 *  15: rl4co_am_decode_args carries the multi-agent TSP's folded context table and agent counts (mtsp_ctx, num_agents,
 *      behind err); rl4co_mtsp_step.
 *  16: rl4co_am_decode_beam / rl4co_am_decode_beam_max_width (beam search, rl4co_am_decode_beam_args);
 *      RL4CO_EBIT_BEAM_INFEASIBLE.
 *  17: rl4co_tsp_two_opt / rl4co_tsp_two_opt_lds_nodes (TSP local search, rl4co_tsp_two_opt_args);
 *      RL4CO_EBIT_TOUR_INDEX.
 *  18: rl4co_aco_tsp / rl4co_aco_tsp_lds_nodes (Ant System search on a heatmap, rl4co_aco_tsp_args, RL4CO_ACO_*).
 *  19: rl4co_aco_cvrp / rl4co_aco_cvrp_lds_nodes (the same search for CVRP, rl4co_aco_cvrp_args).
 *  20: rl4co_tsp_nls / rl4co_tsp_nls_lds_nodes (neural-guided local search for TSP, rl4co_tsp_nls_args).
 *  21: rl4co_nargnn_heatmap / rl4co_nargnn_lds_nodes / rl4co_nargnn_scratch_bytes (DeepACO's heatmap encoder,
 *      rl4co_nargnn_args).
 *  22: rl4co_aco_prize / rl4co_aco_prize_lds_nodes (the Ant System search for OP and PCTSP, rl4co_aco_prize_args).
 *  23: rl4co_nargnn_depot_heatmap / rl4co_nargnn_depot_lds_nodes / rl4co_nargnn_depot_scratch_bytes (the heatmap encoder
 *      for the depot graphs of CVRP, OP and PCTSP, rl4co_nargnn_depot_args).
 *  24: rl4co_aco_tsp_logp_grad / rl4co_aco_tsp_grad_lds_entries (the backward of the ants' log-likelihoods with respect
 *      to the heatmap, DeepACO's training path, rl4co_aco_tsp_grad_args).
 *  25: rl4co_aco_depot_logp_grad / rl4co_aco_depot_grad_lds_entries / rl4co_aco_depot_grad_scratch_bytes (the same backward
 *      for the depot graphs of CVRP, OP and PCTSP, rl4co_aco_depot_grad_args).
 *  26: rl4co_nargnn_train_forward / rl4co_nargnn_train_backward / rl4co_nargnn_train_workspace_bytes (the heatmap
 *      encoder's GNN stack in train mode and its backward, rl4co_nargnn_train_args).
 *  27: rl4co_nargnn_depot_train_forward / rl4co_nargnn_depot_train_backward / rl4co_nargnn_depot_train_workspace_bytes
 *      (the same stack on the depot graphs of CVRP, OP and PCTSP, rl4co_nargnn_depot_train_args).
 *  28: rl4co_nargnn_logz_forward / rl4co_nargnn_logz_backward / rl4co_nargnn_logz_workspace_bytes (GFACS's log-partition
 *      head on the stack's edge state, rl4co_nargnn_logz_args, RL4CO_LOGZ_POOL_*).
 *  29: rl4co_aco_tsp_opts / rl4co_aco_cvrp_opts / rl4co_aco_prize_opts / rl4co_aco_tsp_logp_grad_opts /
 *      rl4co_aco_depot_logp_grad_opts (greedy and top-k / top-p decoding of a heatmap, rl4co_heatmap_decode_opts). */
#define RL4CO_ABI_VERSION 29

/* ---- status codes ------------------------------------------------------ */
#define RL4CO_OK 0
#define RL4CO_ERR_ARG 1     /* bad argument (null pointer, size out of range)  */
#define RL4CO_ERR_HIP 2     /* HIP runtime error, see rl4co_last_error()       */
#define RL4CO_ERR_UNSUPPORTED 3

/* ---- sticky error bits written to `err` (device int32) ------------------ */
#define RL4CO_EBIT_NAN_LOGIT 1   /* nn/attention.py:295-296 "Logits contain NaNs"        */
#define RL4CO_EBIT_INFEASIBLE 2  /* utils/decoding.py:393,409 "infeasible action selected" */
#define RL4CO_EBIT_INVALID_TOUR 4 /* tsp/env.py:161, cvrp/env.py:157-163 "Invalid tour"   */
#define RL4CO_EBIT_CAPACITY 8    /* cvrp/env.py:175-177 "Used more than capacity"         */
#define RL4CO_EBIT_MAX_STEPS 16  /* constructive/base.py:236-238 max_steps exceeded       */
#define RL4CO_EBIT_NEG_INF_LOGP 32 /* utils/decoding.py:56 "Logprobs should not be -inf"  */
#define RL4CO_EBIT_DUPLICATES 64  /* op/env.py:178-181 "Duplicates"                        */
#define RL4CO_EBIT_MAX_LENGTH 128 /* op/env.py:192-194 "Max length exceeded"               */
#define RL4CO_EBIT_PRIZE 256      /* pctsp/env.py:192-201 "Total prize does not satisfy min total prize" */
#define RL4CO_EBIT_NOT_ALL_NODES 512   /* pdp/env.py:208-213 "Not visiting all nodes"                  */
#define RL4CO_EBIT_DEPOT_MIDDLE 1024   /* pdp/env.py:216-218 "Going back to depot in the middle ..."   */
#define RL4CO_EBIT_NO_PICKUP 2048      /* pdp/env.py:220-223 "Deliverying without pick-up"             */
#define RL4CO_EBIT_TW_NEGATIVE 4096    /* cvrptw/env.py:153 "Time windows must be non-negative."       */
#define RL4CO_EBIT_TW_RETURN 8192      /* cvrptw/env.py:154-157 "vehicle cannot perform service and get back to depot in time." */
#define RL4CO_EBIT_TW_DURATION 16384   /* cvrptw/env.py:158 "Service durations must be non-negative."  */
#define RL4CO_EBIT_TW_EMPTY 32768      /* cvrptw/env.py:159-161 "there are unfeasible time windows"    */
#define RL4CO_EBIT_TW_DEADLINE 65536   /* cvrptw/env.py:176-179 "vehicle cannot start service before deadline" */
#define RL4CO_EBIT_BEAM_INFEASIBLE 131072 /* utils/decoding.py:485 "infeasible action selected": beam search kept a -inf candidate (fewer than beam_width finite ones) */
#define RL4CO_EBIT_TOUR_INDEX 262144 /* rl4co_tsp_two_opt: a tour holds a node index outside [0, N) (the reference would index its distance matrix out of bounds); that tour is returned unchanged */

/* ---- enums --------------------------------------------------------------- */
#define RL4CO_ENV_TSP 0
#define RL4CO_ENV_CVRP 1
#define RL4CO_ENV_OP 2 /* orienteering problem: STREAM / LDS / WIDE decode variants */
#define RL4CO_ENV_PCTSP 3 /* prize-collecting TSP (same row): STREAM / LDS / WIDE decode variants */
#define RL4CO_ENV_PDP 4 /* pickup and delivery (same row): STREAM / LDS / WIDE decode variants */
#define RL4CO_ENV_CVRPTW 5 /* CVRP with time windows (same row): STREAM / LDS / WIDE decode variants */
/* Split-delivery VRP (envs/routing/sdvrp/env.py): the one environment with a dynamic embedding (the remaining demand moves
 * the keys and values every step). Decode only — STREAM / LDS / WIDE; not the multistart variant, the unfolded mode, the
 * replay or the teacher kernels, whose six environments are the ids above. */
#define RL4CO_ENV_SDVRP 6
/* Multi-agent TSP, min-max (envs/routing/mtsp/env.py): up to num_agents subtours from the depot (node 0), the reward is the
 * longest subtour and is carried in the state. Decode only — STREAM / LDS / WIDE; not the multistart variant, the unfolded
 * mode, the replay or the teacher kernels. */
#define RL4CO_ENV_MTSP 7

#define RL4CO_DECODE_GREEDY 0   /* utils/decoding.py:387-397 */
#define RL4CO_DECODE_SAMPLE 1   /* utils/decoding.py:399-413 */
#define RL4CO_DECODE_EVALUATE 2 /* utils/decoding.py:448-461 */

#define RL4CO_DT_F32 0
#define RL4CO_DT_BF16 1
#define RL4CO_DT_F16 2 /* IEEE half planes: the reference's default "16-mixed" regime (utils/trainer.py:57); served by the
                          fused encoder, the streaming and the multistart (MS) decode kernels and both teacher-forced
                          backward variants */

/* kernel variants of rl4co_am_decode (same results up to the documented summation tree) */
#define RL4CO_VARIANT_AUTO 0
#define RL4CO_VARIANT_STREAM 1 /* planes streamed from HBM every step, 1 wave per trajectory     */
#define RL4CO_VARIANT_LDS 2    /* bf16 planes loaded into LDS once per rollout, 4 waves / trajectory */
#define RL4CO_VARIANT_WIDE 3   /* bf16 planes streamed every step, 4 waves / trajectory (few trajectories, large N) */
#define RL4CO_VARIANT_MS 4     /* multistart on the matrix cores: one workgroup per (instance, column tile of 16
                                  starts), glimpse planes in LDS, logit-key tile in registers, two workgroups per
                                  CU; bf16 query / glimpse (pinned to the rounding-model oracle, 5e-3); every
                                  environment; auto where measured faster: TSP / PDP / PCTSP from 8 starts per
                                  instance, CVRP from 16 */
#define RL4CO_VARIANT_STREAM_REG 5 /* STREAM with a step's per-head scores held in registers instead of LDS, whose
                                  bytes go to a larger row cache (11 resident rows per trajectory at N = 100 instead
                                  of 6); 16-bit planes, TSP / CVRP, N <= 112, not the unfolded mode; bit for bit
                                  STREAM's results */

#define RL4CO_EMBED_DIM 128 /* the engine is specialised for the AM default d=128, H=8 */
#define RL4CO_NUM_HEADS 8

/* Library identification. */
const char* rl4co_version(void);
/* RL4CO_ABI_VERSION of the header the loaded library was compiled against (see above). */
int rl4co_abi_version(void);
/* Last HIP error string seen by the calling thread ("" if none). */
const char* rl4co_last_error(void);

/* --------------------------------------------------------------------------
 * a1  gather_by_index(src, idx, dim=1)            rl4co/utils/ops.py:54-66
 * out[b,k,:] = src[b, idx[b,k], :]   src [B,N,D] f32, idx [B,K] i64, out [B,K,D]
 * -------------------------------------------------------------------------- */
int rl4co_gather_by_index_f32(const float* src, const int64_t* idx, int B, int N, int D,
                              int K, float* out, int32_t* err, void* stream);

/* --------------------------------------------------------------------------
 * a2/a3  get_tour_length / TSPEnv._get_reward / CVRPEnv._get_reward
 *        rl4co/utils/ops.py:77-90, envs/routing/tsp/env.py:150-156,
 *        envs/routing/cvrp/env.py:138-147
 * out[b] = (negate ? -1 : 1) * sum_t || p[t+1 mod n] - p[t] ||_2  over the closed
 * tour p = (prepend_depot ? locs[b,0] : -) ++ locs[b, actions[b,:]]  (n = T + prepend).
 * Bit-exact restatement of ATen's CPU arithmetic: per segment
 * sqrt(fma(dy,dy,fl(dx*dx))), row sum in the 8-lane x 4-ILP cascade order of
 * aten/src/ATen/native/cpu/SumKernel.cpp.
 * locs [B_locs,N,2] f32 with trajectory b reading instance b % B_locs
 * (multistart: s-major batchify, ops.py:10-28); actions [B,T] i64.
 * -------------------------------------------------------------------------- */
int rl4co_tour_length_f32(const float* locs, const int64_t* actions, int B, int B_locs, int N,
                          int T, int prepend_depot, int negate, float* out, void* stream);
/* Same arithmetic with the horizon read ON THE DEVICE: actions is a [B,row_stride] buffer whose first
 * T = t_add + *steps_dev columns (clamped to row_stride) are the tour — steps_dev is word [0] of the decode launch's
 * steps_summary. Lets the reward of a data-dependent horizon (CVRP) go out before the rollout's single read-back and
 * inside a captured HIP graph; the row-sum association follows the real T exactly as above. */
int rl4co_tour_length_dyn_f32(const float* locs, const int64_t* actions, int B, int B_locs, int N, int row_stride,
                              const int32_t* steps_dev, int t_add, int prepend_depot, int negate, float* out,
                              void* stream);

/* --------------------------------------------------------------------------
 * a4  check_solution_validity   tsp/env.py:158-164, cvrp/env.py:149-177
 * TSP : every row of actions [B,T==N] is a permutation of 0..N-1.
 * CVRP: customers 1..N-1 appear exactly once, everything else is 0, and the
 *       running load (reset at the depot, clamped at 0) never exceeds
 *       vehicle_capacity + 1e-5.  demand [B_inst,N-1], capacity [B_inst].
 * Violations set RL4CO_EBIT_INVALID_TOUR / RL4CO_EBIT_CAPACITY in *err.
 * -------------------------------------------------------------------------- */
int rl4co_tsp_check_solution(const int64_t* actions, int B, int N, int T, int32_t* err,
                             void* stream);
int rl4co_cvrp_check_solution(const int64_t* actions, const float* demand,
                              const float* vehicle_capacity, int B, int B_inst, int N, int T,
                              int32_t* err, void* stream);

/* --------------------------------------------------------------------------
 * a6  TSPEnv._step              envs/routing/tsp/env.py:60-86
 * first = (i==0) ? action : first ; cur = action ; mask[action] = 0 ; i += 1 ;
 * done = !any(mask).   action/first/cur/i int64 [B], mask/done uint8.
 * (a5 TSPEnv._reset is pure allocation and lives in the host mirror.)
 * -------------------------------------------------------------------------- */
int rl4co_tsp_step(const int64_t* action, uint8_t* action_mask, int64_t* first_node,
                   int64_t* current_node, int64_t* step_i, uint8_t* done, int B, int N,
                   int32_t* err, void* stream);

/* --------------------------------------------------------------------------
 * a8+a9  CVRPEnv._step + get_action_mask   envs/routing/cvrp/env.py:66-96,126-136
 * used = (used + demand[clamp(a-1,0,n-1)]) * (a != 0); visited[a] = 1; cur = a;
 * done = (sum visited == N); mask_loc = visited[1:] | (demand + used > cap + 1e-5);
 * mask[0] = !((cur==0) & any(!mask_loc)); mask[1:] = !mask_loc.
 * demand [B_inst,N-1] (trajectory b reads row b % B_inst), used/cap f32 [B].
 * Passing action == NULL only recomputes the mask (a9 / a7's reset mask).
 * -------------------------------------------------------------------------- */
/* In-place SDVRPEnv._step + get_action_mask (sdvrp/env.py:56-123); action == NULL: mask only. demand_with_depot [B,N]. */
int rl4co_sdvrp_step(const int64_t* action, float* demand_with_depot, float* used_capacity, const float* vehicle_capacity,
                     int64_t* current_node, uint8_t* action_mask, uint8_t* done, int B, int N, int32_t* err, void* stream);

/* In-place MTSPEnv._step (mtsp/env.py:63-131; the mask is the state); locs [B_inst,N,2], num_agents [B_inst] (trajectory b
 * reads row b % B_inst); agent_idx i64 [B], current_length / max_subtour_length f32 [B]. */
int rl4co_mtsp_step(const int64_t* action, const float* locs, const int64_t* num_agents, int64_t* agent_idx,
                    float* current_length, float* max_subtour_length, int64_t* current_node, uint8_t* action_mask,
                    uint8_t* done, int B, int B_inst, int N, int32_t* err, void* stream);

int rl4co_cvrp_step(const int64_t* action, const float* demand, float* used_capacity,
                    const float* vehicle_capacity, uint8_t* visited, int64_t* current_node,
                    uint8_t* action_mask, uint8_t* done, int B, int B_inst, int N,
                    int32_t* err, void* stream);

/* --------------------------------------------------------------------------
 * N4  OPEnv (orienteering)      envs/routing/op/env.py:67-194
 * reset: max_length_table[b,j] = (max_length[b] - |loc_0 - loc_j|) - 1e-6  (op/env.py:118-122)
 * step : tour += |loc_a - loc_cur| ; visited[a] = 1 ; done = (a == 0) & (i > 0) ; i += 1 ; cur = a ;
 *        mask[j] = !(visited[j] | visited[0] | tour + |loc_j - loc_cur| > max_length_table[j]) ; mask[0] = 1
 *        (action == NULL: mask only). Distances are sqrt(fma(dy,dy,dx*dx)) like the tour length.
 * reward: out[b] = sum_t prize[b % B_values, actions[b,t]] in ATen's inner-dim sum order (op/env.py:156-166)
 * check : no customer twice (RL4CO_EBIT_DUPLICATES), closed tour length <= max_length + 1e-5 measured
 *         at every node as the reference does (RL4CO_EBIT_MAX_LENGTH)   (op/env.py:168-194)
 * locs [B_inst,N,2], max_length_table / prize [B_inst,N] (trajectory b reads row b % B_inst).
 * -------------------------------------------------------------------------- */
int rl4co_op_max_length(const float* locs, const float* max_length, int B, int N, float* table, void* stream);
int rl4co_op_step(const int64_t* action, const float* locs, const float* max_length_table, float* tour_length,
                  uint8_t* visited, int64_t* current_node, int64_t* step_i, uint8_t* action_mask, uint8_t* done,
                  int B, int B_inst, int N, int32_t* err, void* stream);
int rl4co_gather_sum_f32(const float* values, const int64_t* actions, int B, int B_values, int N, int T, float* out,
                         void* stream);
int rl4co_op_check_solution(const int64_t* actions, const float* locs, const float* max_length_table, int B, int B_inst,
                            int N, int T, int32_t* err, void* stream);

/* --------------------------------------------------------------------------
 * N4  PCTSPEnv (prize-collecting TSP)   envs/routing/pctsp/env.py:62-201
 * step : prize += real_prize[a] ; visited[a] = 1 ; done = (i > 0) & (a == 0) ; i += 1 ; cur = a ;
 *        mask[j>=1] = !(visited[j] | visited[0]) ; mask[0] = !((prize < 1.0) & (some customer unvisited))
 *        (action == NULL: mask only). real_prize [B_inst,N] with 0 for the depot.
 * reward (host composition, fp32): gather_sum(penalty, actions) - (tour_length(depot ++ tour) +
 *        gather_sum(penalty, 1..N-1)) — three ATen-order sums, pctsp/env.py:150-173.
 * check : no customer twice (RL4CO_EBIT_DUPLICATES); collected prize >= 1 - 1e-5 or every customer
 *         visited (RL4CO_EBIT_PRIZE)   pctsp/env.py:175-201. Trailing depot zeros are neutral.
 * -------------------------------------------------------------------------- */
int rl4co_pctsp_step(const int64_t* action, const float* real_prize, float* cur_total_prize, uint8_t* visited,
                     int64_t* current_node, int64_t* step_i, uint8_t* action_mask, uint8_t* done, int B, int B_inst,
                     int N, int32_t* err, void* stream);
/* prize_sum [B] = rl4co_gather_sum_f32(real_prize, actions) (the reference's summation order) */
int rl4co_pctsp_check_solution(const int64_t* actions, const float* prize_sum, int B, int N, int T, int32_t* err,
                               void* stream);

/* --------------------------------------------------------------------------
 * N4  PDPEnv (pickup and delivery)   envs/routing/pdp/env.py:64-99,204-223
 * Nodes: 0 = depot, 1..n/2 pickups, n/2+1..n their deliveries (n = N - 1 even).
 * step : available[a] = 0 ; to_deliver[(a + n/2) % (n + 1)] = 1 ; mask = available & to_deliver ;
 *        done = no node available ; i += 1 ; cur = a   (action == NULL: mask only).
 * check (actions [B,T]; a depot visit is prepended unless force_start_at_depot): every node exactly once
 *        (RL4CO_EBIT_NOT_ALL_NODES), no depot visit strictly inside the tour (RL4CO_EBIT_DEPOT_MIDDLE),
 *        every pickup before its delivery (RL4CO_EBIT_NO_PICKUP).
 * reward: rl4co_tour_length_f32(prepend_depot = 1, negate = 1)   pdp/env.py:191-202
 * -------------------------------------------------------------------------- */
int rl4co_pdp_step(const int64_t* action, uint8_t* available, uint8_t* to_deliver, int64_t* current_node, int64_t* step_i,
                   uint8_t* action_mask, uint8_t* done, int B, int N, int32_t* err, void* stream);
int rl4co_pdp_check_solution(const int64_t* actions, int B, int N, int T, int force_start_at_depot, int32_t* err,
                             void* stream);

/* --------------------------------------------------------------------------
 * T transitions of given trajectories in ONE launch, with what the decoder saw before each of them
 * (the `evaluate` decoding strategy's state sequence: utils/decoding.py:448-461, models/common/constructive/base.py:226-263
 * with `actions` given; rl/ppo/ppo.py:128-170 re-evaluates stored actions the same way). Equivalent to, for t in [0, T):
 *   masks[:, t] = action_mask ; prev[:, t] = current_node ;
 *   TSP: first[:, t] = first_node ; use_placeholder[:, t] = (i < 1)                     (env_embeddings/context.py:86-103)
 *   CVRP / CVRPTW / OP / PCTSP: rem[:, t] = rem_base - scalar (PCTSP: clamped at 0)     (context.py:105-213)
 *   CVRPTW: now[:, t] = current_time ;
 *   rl4co_<env>_step(actions[:, t], state ...)
 * on the same state arrays (updated in place; the step semantics are those entry points', literally the same device code).
 * `scalar` = used_capacity (CVRP, CVRPTW), tour_length (OP), cur_total_prize (PCTSP); `visited` = `available` for PDP;
 * `demand` = real_prize [B_inst, N] for PCTSP; `max_length` = the OP entry-limit table of rl4co_op_max_length.
 * -------------------------------------------------------------------------- */
typedef struct rl4co_env_replay_args {
  int32_t env;    /* RL4CO_ENV_* */
  int32_t B;      /* trajectories (rows of the state) */
  int32_t B_inst; /* instances (rows of the instance data); B % B_inst == 0, row b reads instance b % B_inst */
  int32_t N;      /* nodes */
  int32_t T;      /* steps to replay */
  int32_t reserved0;
  const int64_t* actions; /* [B, T] */
  /* state, updated in place */
  uint8_t* action_mask;  /* [B, N] */
  int64_t* current_node; /* [B] */
  uint8_t* done;         /* [B] */
  int64_t* first_node;   /* [B]    TSP */
  int64_t* step_i;       /* [B]    TSP, OP, PCTSP, PDP */
  uint8_t* visited;      /* [B, N] CVRP, CVRPTW, OP, PCTSP; PDP: available */
  uint8_t* to_deliver;   /* [B, N] PDP */
  float* scalar;         /* [B]    see above */
  float* current_time;   /* [B]    CVRPTW */
  /* instance data */
  const float* vehicle_capacity; /* [B]             CVRP, CVRPTW */
  const float* demand;           /* [B_inst, N - 1] CVRP, CVRPTW; PCTSP: real prize [B_inst, N] */
  const float* locs;             /* [B_inst, N, 2]  OP, CVRPTW */
  const float* max_length;       /* [B_inst, N]     OP */
  const float* time_windows;     /* [B_inst, N, 2]  CVRPTW */
  const float* durations;        /* [B_inst, N]     CVRPTW */
  const float* rem_base;         /* [B] minuend of the context scalar: capacity / max_length[:, 0] / prize_required */
  /* outputs */
  uint8_t* masks;           /* [B, T, N] */
  int64_t* prev;            /* [B, T] */
  int64_t* first;           /* [B, T] TSP */
  uint8_t* use_placeholder; /* [B, T] TSP */
  float* rem;               /* [B, T] CVRP, CVRPTW, OP, PCTSP */
  float* now;               /* [B, T] CVRPTW */
  int32_t* err;             /* sticky bits (RL4CO_EBIT_INFEASIBLE: an action out of range), may be NULL */
  uint32_t* mask_bits;      /* [B, T, mask_words] optional: `masks` as bits (bit j of word j / 32 = node j feasible; the
                               padding bits are 0) — rl4co_cross_attn_*'s mask */
  int32_t mask_words;       /* >= ceil(N / 32) */
  int32_t reserved1;
} rl4co_env_replay_args;

int rl4co_env_replay(const rl4co_env_replay_args* args, void* stream);

/* --------------------------------------------------------------------------
 * N4  CVRPTWEnv (CVRP + time windows)   envs/routing/cvrptw/env.py:83-190
 * step : d = |loc_a - loc_cur| ; time = (a != 0) * (max(time + d, tw_start[a]) + duration[a]) ; then the CVRP
 *        transition (a8) ; mask = cvrp_mask & (time + |loc_j - loc_a| <= tw_end[j])   (action == NULL: mask only).
 *        Distances are sqrt(fma(dy, dy, dx * dx)) like the tour-length kernel.
 * check: the instance-data assertions (RL4CO_EBIT_TW_NEGATIVE / _RETURN / _DURATION / _EMPTY; `max_time` is
 *        tw_end of instance 0's depot, as in the reference) and the deadline replay
 *        t = max(trunc(t + d), tw_start) <= tw_end ; t += duration ; t = 0 at the depot (RL4CO_EBIT_TW_DEADLINE).
 *        The CVRP part of the check is rl4co_cvrp_check_solution. Trailing depot zeros are neutral.
 * -------------------------------------------------------------------------- */
int rl4co_cvrptw_step(const int64_t* action, const float* demand, const float* locs, const float* time_windows,
                      const float* durations, float* used_capacity, const float* vehicle_capacity, float* current_time,
                      uint8_t* visited, int64_t* current_node, uint8_t* action_mask, uint8_t* done, int B, int B_inst, int N,
                      int32_t* err, void* stream);
int rl4co_cvrptw_check_solution(const int64_t* actions, const float* locs, const float* time_windows,
                                const float* durations, int B, int B_inst, int N, int T, int32_t* err, void* stream);

/* --------------------------------------------------------------------------
 * a13-a21  AttentionModel decode: one step, or the whole autoregressive loop.
 *
 * Replaces, per step: TSPContext/VRPContext (env_embeddings/context.py:105-149),
 * AttentionModelDecoder._compute_q/_compute_kvl/forward (zoo/am/decoder.py:128-193),
 * PointerAttention.forward (nn/attention.py:274-320), process_logits
 * (utils/decoding.py:138-188), Greedy/Sampling/Evaluate (decoding.py:344-461),
 * TSPEnv._step / CVRPEnv._step (+ get_action_mask); and, with max_steps > 1, the
 * `while not td["done"].all()` loop of ConstructivePolicy.forward
 * (models/common/constructive/base.py:226-238).
 *
 * The cache is the *folded* form of PrecomputedCache (zoo/am/decoder.py:21-40,
 * 201-228) — algebraically identical, built once per rollout by dense GEMMs:
 *   glimpse_key = h Wk^T, glimpse_val = h Wv^T                     [B_inst,N,128]
 *   logit_key   = h (W_out^T Wl)^T   (project_out folded into the logit key)
 *   ctx_first   = h W_ctx[:, :128]^T, ctx_cur = h W_ctx[:,128:256]^T (TSP)
 *   ctx_cur     = h W_ctx[:, :128]^T, w_cap = W_ctx[:,128]           (CVRP)
 *   q_bias      = project_fixed_context(mean_j h_j) or NULL (POMO)  [B_inst,128]
 *   q_step0     = W_ctx W_placeholder (TSP, step i==0)               [128]
 * so that one decode step is a pure stream over the three [N,128] planes.
 * Trajectory r (0..B-1) uses instance r % B_inst (s-major multistart layout).
 * -------------------------------------------------------------------------- */
typedef struct rl4co_am_decode_args {
  /* problem */
  int32_t env;         /* RL4CO_ENV_*                                            */
  int32_t B;           /* trajectories = instances x starts                      */
  int32_t B_inst;      /* instances owning cache rows                            */
  int32_t N;           /* nodes incl. depot                                      */
  /* decode configuration */
  int32_t mode;        /* RL4CO_DECODE_*                                         */
  int32_t max_steps;   /* 1 = single step; >= horizon = full rollout             */
  int32_t mask_inner;  /* PointerAttention(mask_inner=True) default 1            */
  int32_t mask_logits; /* process_logits(mask_logits=True) default 1             */
  float tanh_clipping; /* 10.0 default (am/policy.py:74); 0 disables             */
  float temperature;   /* 1.0 default                                            */
  /* folded cache */
  int32_t cache_dtype; /* RL4CO_DT_F32 | RL4CO_DT_BF16 for the three planes      */
  int32_t variant;     /* RL4CO_VARIANT_*: 0 = let the library choose              */
  const void* glimpse_key;
  const void* glimpse_val;
  const void* logit_key;
  int64_t kvl_row_stride;   /* elements between node rows   (128 planar, 384 interleaved) */
  int64_t kvl_batch_stride; /* elements between instances                                  */
  const void* ctx_first;    /* [B_inst,N,128] TSP only; element type ctx_dtype (fp32 unless set) */
  const void* ctx_cur;      /* [B_inst,N,128]                                              */
  const float* q_bias;      /* [B_inst,128] or NULL                                        */
  const float* q_step0;     /* [128] TSP only                                              */
  const float* w_cap;       /* [128] CVRP only                                             */
  /* "unfolded" parity mode (unfold = 1; TSP / CVRP, streaming variant): the three batch-shared matrices are
   * applied PER STEP in the reference's association instead of being folded into per-node rows —
   * q = project_context([h_first ; h_cur] | W_placeholder | [h_cur ; cap - used]) + graph context
   * (env_embeddings/context.py:61-74,120-134), glimpse = project_out(heads) (nn/attention.py:287), logits =
   * glimpse . K_l with logit_key the RAW third chunk of project_node_embeddings (zoo/am/decoder.py:201-228);
   * each GEMV is one fma chain over the input dims in ascending order, starting from 0. ctx_first / ctx_cur /
   * q_step0 / w_cap are not read. Measures how many greedy near-tie flips the fold itself causes. */
  int32_t unfold;
  int32_t ctx_width;          /* input width of project_context: 256 TSP, 129 CVRP              */
  const float* node_embed;    /* [B_inst,N,128] encoder output h                               */
  const float* w_ctx_t;       /* [ctx_width,128] project_context.weight transposed             */
  const float* w_out_t;       /* [128,128] project_out.weight transposed                       */
  const float* w_placeholder; /* [256] TSP first-step context (context.py:120-128)             */
  /* environment state, read at entry and written back at exit */
  uint8_t* action_mask;     /* [B,N] 1 = feasible                                          */
  int64_t* first_node;      /* [B] TSP                                                     */
  int64_t* current_node;    /* [B]                                                         */
  int64_t* step_i;          /* [B] TSP                                                     */
  uint8_t* done;            /* [B]                                                         */
  const float* demand;      /* [B_inst,N-1] CVRP                                           */
  float* used_capacity;     /* [B] CVRP                                                    */
  const float* vehicle_capacity; /* [B] CVRP                                               */
  uint8_t* visited;         /* [B,N] CVRP, OP                                              */
  /* OP (orienteering, envs/routing/op/env.py): used_capacity carries the tour length so far, step_i
   * the step counter; the depot row of max_length plays the vehicle capacity in the context scalar */
  const float* locs;        /* [B_inst,N,2] OP                                             */
  const float* max_length;  /* [B_inst,N] OP: longest tour with which node j may be entered */
  /* PCTSP (envs/routing/pctsp/env.py): demand = real prize WITH the depot column [B_inst,N],
   * used_capacity = prize collected so far, vehicle_capacity = prize_required [B], step_i, visited */
  /* PDP (envs/routing/pdp/env.py): visited carries the `available` flags (1 = not yet visited), to_deliver
   * the precedence flags; step_i; the context is the current node's row alone (no scalar, w_cap NULL) */
  uint8_t* to_deliver;      /* [B,N] PDP                                                   */
  /* CVRPTW (envs/routing/cvrptw/env.py): the CVRP fields plus locs, time_windows, durations, current_time; the
   * context carries two scalars, q = w_time * time + (w_cap * (cap - used) + ctx_cur[cur]) (context.py:152-166) */
  const float* time_windows; /* [B_inst,N,2] (start, end), fp32                             */
  const float* durations;    /* [B_inst,N] service times                                    */
  float* current_time;       /* [B]                                                         */
  const float* w_time;       /* [128] = W_ctx[:, 129]                                       */
  /* SDVRP (envs/routing/sdvrp/env.py): used_capacity, vehicle_capacity as CVRP; no visited. The dynamic embedding
   * Linear(1 -> 3 * 128)(remaining demand) (env_embeddings/dynamic.py:60-78, zoo/am/decoder.py:142-152) is rank one per
   * node, so it travels as three batch-shared vectors and the kernel adds d_j * (x . u) to each dot product */
  const float* dyn_vectors;  /* [3,128] fp32 whatever the planes: (u_k, u_v, W_out^T u_l)      */
  float* demand_state;       /* [B,N] remaining demand with the depot column, read and written  */
  /* decoding inputs */
  const float* exp_noise;   /* [max_steps,B,N] Exp(1) draws (parity mode) or NULL          */
  uint64_t philox_seed;     /* in-kernel Exp(1) noise when exp_noise == NULL               */
  uint64_t philox_offset;
  const uint64_t* philox_seed_dev; /* optional device word XOR-ed into philox_seed at kernel entry: a captured HIP
                                    * graph bakes the argument block, the word lets every replay draw fresh noise */
  const int64_t* forced_actions; /* [B,out_stride] for RL4CO_DECODE_EVALUATE               */
  /* outputs */
  int32_t t0;               /* column of the first step in actions/logps                   */
  int32_t out_stride;       /* row stride (Tmax) of actions/logps/forced_actions           */
  int64_t* actions;         /* [B,out_stride]                                              */
  float* logps;             /* [B,out_stride] log p(a_t)                                   */
  float* all_logps;         /* [B,out_stride,N] or NULL (store_all_logp / entropy)         */
  float* entropy;           /* [B] accumulated -sum p log p, or NULL                       */
  int32_t* n_steps;         /* [B] steps actually taken by each trajectory, or NULL        */
  int32_t* steps_summary;   /* [4], 8-byte aligned, or NULL (zero-initialised by the caller): [0] = max and [1] += sum
                             * over the trajectories of the steps taken — what the host needs of n_steps without a
                             * reduction launch; [2..3] = ONE 64-bit counter (little endian: low word, high word) += cache
                             * rows the launch streamed per plane from HBM (feasible rows of every step; 0 for the
                             * variants whose planes are LDS-resident): the measured numerator of the decode kernel's
                             * roofline in bench.py. 64 bits: 409 600 trajectories x 5050 rows already reach 2.07e9.
                             * A misaligned pointer is refused (RL4CO_STATUS_INVALID_ARGUMENT)                       */
  int32_t* err;             /* sticky error bits                                           */
  /* MTSP (envs/routing/mtsp/env.py): locs as OP; agent_idx in step_i, current_length in used_capacity, max_subtour_length
   * in current_time, all [B], read and written. The context W_ctx [h_cur ; W_dyn f] of the four running scalars
   * f = (num_agents - agent_idx, current_length, max_subtour_length, |loc_cur - loc_0|) (env_embeddings/context.py:246-280)
   * travels folded: q = ctx_cur[cur] + sum_k f_k g_k */
  const float* mtsp_ctx;     /* [4,128] fp32 whatever the planes: g = W_ctx[:, 128:] W_dyn, row k for f_k */
  const int64_t* num_agents; /* [B_inst]                                                     */
  /* (r06) the folded context tables in the element type of the planes: ctx_dtype = RL4CO_DT_BF16 / _F16 (0 = RL4CO_DT_F32,
   * the default) with their own strides in ELEMENTS (0 = dense: row 128, instance N * 128) — e.g. columns 3 and 4 of the
   * ONE [B_inst * N, 5 * 128] 16-bit matrix a fused cache-fold GEMM writes (row stride 640): no fp32 copies of the tables.
   * The rows are widened to fp32 on load; everything downstream is the fp32 arithmetic of the fp32 tables. Multistart
   * variant (am_decode_ms.hip); the other variants require RL4CO_DT_F32. */
  int32_t ctx_dtype;
  int32_t reserved0;
  int64_t ctx_row_stride;
  int64_t ctx_batch_stride;
  /* (v13) top-k / top-p (nucleus) filter of utils/decoding.py:109-188 between temperature and log_softmax, in the order
   * specified in the am_decode.hip header. top_k <= 0: no top-k (k >= the step's candidates: nothing removed); top_p <= 0
   * or >= 1: no top-p. Removed nodes get log-prob -inf and are never selected. STREAM / LDS / WIDE variants and the
   * unfolded mode; an explicit RL4CO_VARIANT_MS with an active filter is refused and the auto choice avoids it. */
  int32_t top_k;
  float top_p;
  uint32_t* kept_bits; /* [B,out_stride,kept_words] or NULL: bit j % 32 of word j / 32 = node j has a finite log-prob
                        * after mask and filter (the layout of rl4co_env_replay's mask bits); written per step taken */
  int32_t kept_words;  /* words per (trajectory, step): a multiple of 4 covering N                                    */
  int32_t reserved1;
} rl4co_am_decode_args;

int rl4co_am_decode(const rl4co_am_decode_args* args, void* stream);

/* Bytes of LDS one trajectory needs for N nodes (for occupancy planning / tests). */
int rl4co_am_decode_lds_bytes(int N, int env);

/* Number of row groups G the kernel that will serve `args` splits a trajectory's cache rows
 * into (row j -> group j % G). G fixes the fp32 summation tree of the glimpse (am_decode.hip
 * header), so the specified-order oracle asks for it instead of guessing. -1 on bad args. */
int rl4co_am_decode_row_groups(const rl4co_am_decode_args* args); /* 0: variant without such a contract (MS) */
/* The variant (RL4CO_VARIANT_STREAM / _LDS / ...) rl4co_am_decode will run for `args`; -1: an explicit variant that
 * cannot serve them. */
int rl4co_am_decode_variant(const rl4co_am_decode_args* args);

/* --------------------------------------------------------------------------
 * Beam-search decoding: BeamSearch (utils/decoding.py:464-600 — pre_decoder_hook's start nodes, _make_beam_step's
 * torch.topk over the beam_width * N candidates, the re-indexing of the state by beam parent, _backtrack) with the decode
 * step of rl4co_am_decode, as ONE launch: one workgroup per instance carries its beam_width beams through the whole
 * rollout (am_decode_beam.hip). TSP and CVRP; fp32 / bf16 / fp16 planes; fp32 dense context tables.
 *
 * Rows are beam-major (s-major, the reference's batchify): row j * B_inst + b is beam j of instance b, in the state
 * tensors ([beam_width * B_inst, ...], the state AFTER the imposed start step, read at entry and written back at exit) and
 * in every output. Column 0 of the outputs is the start node (current_node at entry) with log-prob 0 and parent 0; the
 * decode steps fill columns 1 .. T, T <= max_steps. T is PER INSTANCE: the step at which the instance's last beam is done
 * (a finished CVRP beam keeps offering the depot at log-prob 0 until then). Columns behind an instance's own T are not
 * written, in the aligned and in the per-step outputs: zero-initialised actions / logps read as the reference's padding
 * (depot, log-prob 0); parents / cum_logp there are NOT the padding's values (identity, unchanged). steps_summary[0] is
 * the batch's longest T. Equal candidates are ordered by the lower flat index parent * N + node.
 * A beam's per-step log-probs are bit for bit those of rl4co_am_decode(RL4CO_DECODE_EVALUATE, RL4CO_VARIANT_STREAM) on
 * the same actions. Sticky bits: RL4CO_EBIT_BEAM_INFEASIBLE (fewer than beam_width finite candidates at a step),
 * RL4CO_EBIT_INFEASIBLE, RL4CO_EBIT_NAN_LOGIT, RL4CO_EBIT_NEG_INF_LOGP, RL4CO_EBIT_MAX_STEPS.
 * -------------------------------------------------------------------------- */
typedef struct rl4co_am_decode_beam_args {
  int32_t env;         /* RL4CO_ENV_TSP | RL4CO_ENV_CVRP                         */
  int32_t B_inst;      /* instances (= workgroups)                               */
  int32_t N;           /* nodes incl. depot                                      */
  int32_t beam_width;  /* 2 .. rl4co_am_decode_beam_max_width(N)                 */
  int32_t max_steps;   /* decode steps after the start node, <= out_stride - 1   */
  int32_t mask_inner;  /* as rl4co_am_decode_args                                */
  int32_t mask_logits;
  int32_t cache_dtype; /* RL4CO_DT_F32 | RL4CO_DT_BF16 | RL4CO_DT_F16            */
  float tanh_clipping;
  float temperature;
  /* folded cache, as rl4co_am_decode_args (16-byte aligned planes) */
  const void* glimpse_key;
  const void* glimpse_val;
  const void* logit_key;
  int64_t kvl_row_stride;
  int64_t kvl_batch_stride;
  const float* ctx_first;   /* [B_inst,N,128] TSP                                          */
  const float* ctx_cur;     /* [B_inst,N,128]                                              */
  const float* q_bias;      /* [B_inst,128] or NULL                                        */
  const float* q_step0;     /* [128] TSP                                                   */
  const float* w_cap;       /* [128] CVRP                                                  */
  /* environment state of the beam_width * B_inst beam rows (the slots of rl4co_am_decode_args) */
  uint8_t* action_mask;     /* [W*B_inst,N] 1 = feasible                                   */
  int64_t* first_node;      /* [W*B_inst] TSP                                              */
  int64_t* current_node;    /* [W*B_inst]                                                  */
  int64_t* step_i;          /* [W*B_inst] TSP                                              */
  uint8_t* done;            /* [W*B_inst]                                                  */
  const float* demand;      /* [B_inst,N-1] CVRP                                           */
  float* used_capacity;     /* [W*B_inst] CVRP                                             */
  const float* vehicle_capacity; /* [W*B_inst] CVRP (row b is read for every beam of instance b) */
  uint8_t* visited;         /* [W*B_inst,N] CVRP                                           */
  /* outputs, all [W*B_inst, out_stride] */
  int32_t out_stride;
  int32_t reserved0;
  int64_t* actions;         /* aligned (backtracked) actions of the final beams, best first */
  float* logps;             /* aligned log p(a_t)                                          */
  int32_t* step_nodes;      /* per step, before alignment: node chosen by beam j           */
  float* step_logps;        /* ... its log-prob under its parent                           */
  int32_t* parents;         /* ... the beam of the previous column it extends              */
  float* cum_logp;          /* ... its cumulative log-prob (the kept top-W values, descending in j) */
  int32_t* steps_summary;   /* [2] or NULL (zero-initialised by the caller): [0] = max, [1] += T per instance */
  int32_t* err;             /* sticky error bits                                           */
} rl4co_am_decode_beam_args;

int rl4co_am_decode_beam(const rl4co_am_decode_beam_args* args, void* stream);
/* Largest beam_width rl4co_am_decode_beam serves for N nodes (the kernel's LDS budget, am_decode_beam.hip header); 0 if N
 * itself is out of range. */
int rl4co_am_decode_beam_max_width(int N);

/* --------------------------------------------------------------------------
 * TSP local search: best-improvement 2-opt (envs/routing/tsp/local_search.py:16-81) as ONE launch, one workgroup per
 * tour (tsp_two_opt.hip). Per iteration every pair of positions 1 <= i < j <= T-1 is scored,
 *   change = ((d[prev][tour[j]] + d[tour[i]][next]) - d[prev][tour[i]]) - d[tour[j]][next],
 *   prev = tour[i-1], next = tour[(j+1) % T], pairs with prev == tour[j] or next == tour[i] skipped,
 * in fp32 with one rounding per operation; the smallest change wins, EQUAL CHANGES GO TO THE LOWEST (i, j) (the
 * reference's sequential scan keeps the first); if it is below -1e-6 (compared in double) tour[i..j] is reversed and the
 * search goes on, otherwise it ends. `iterations` counts the final, non-improving scan too; max_iterations = 0 returns
 * the input. The result equals the reference's bit for bit.
 * d is `distances` with 1e9 added on its diagonal, or from `locs`: d[a][b] = sqrtf(fmaf(dy, dy, dx * dx)) (ATen's
 * norm(p=2) over two elements), d[a][a] = 1e9. Exactly one of the two is given. Up to rl4co_tsp_two_opt_lds_nodes() nodes
 * the matrix is kept in LDS; above, up to 1024, distances are computed from coordinates in LDS or read from global memory.
 * A tour with an index outside [0, N) sets RL4CO_EBIT_TOUR_INDEX and is copied through unchanged (0 iterations).
 * out_actions == actions (in place) is allowed.
 * -------------------------------------------------------------------------- */
typedef struct rl4co_tsp_two_opt_args {
  int32_t B;                /* tours (= workgroups), >= 1; instance b serves tour b        */
  int32_t N;                /* nodes, 2 .. 1024                                            */
  int32_t T;                /* tour length, 1 .. 1024                                      */
  int32_t max_iterations;   /* >= 0                                                        */
  const float* locs;        /* [B,N,2] or NULL                                             */
  const float* distances;   /* [B,N,N] or NULL (may be asymmetric)                         */
  const int64_t* actions;   /* [B,T]                                                       */
  int64_t* out_actions;     /* [B,T]                                                       */
  int32_t* iterations;      /* [B] or NULL: scans run per tour                             */
  int32_t* err;             /* sticky error bits                                           */
} rl4co_tsp_two_opt_args;

int rl4co_tsp_two_opt(const rl4co_tsp_two_opt_args* args, void* stream);
/* Largest N whose distance matrix rl4co_tsp_two_opt keeps in LDS (the kernel's LDS budget, tsp_two_opt.hip header). */
int rl4co_tsp_two_opt_lds_nodes(void);

/* --------------------------------------------------------------------------
 * Ant System search on a heatmap for TSP (models/zoo/deepaco/antsystem.py, DeepACO's test-time loop) as ONE launch, one
 * workgroup per instance (aco_tsp.hip). Rows are ant-major: row j * B + b is ant j of instance b, rows = n_ants * B.
 * An iteration is
 *   SAMPLE  L = alpha * log(pheromone) + beta * log_heuristic (two multiplies and an add, each rounded once); every ant
 *           starts at start_nodes[it][row] (column 0 of `actions`, log-prob 0) and takes N - 1 steps: log-softmax of row
 *           `cur` of L over the unvisited nodes (divided by `temperature` first), then the argmax over them of
 *           lp[n] - ln_noise[n], the lowest node on equal keys. ln_noise is the caller's (parity mode: the natural log of
 *           Exp(1) draws) or drawn in the kernel from Philox (step counter philox_offset + it * N + t, trajectory = row).
 *           With forced_actions the given tours are followed and only their log-probs are computed. The reward, minus the
 *           closed tour length from `locs`, is bit-equal to rl4co_tour_length_f32's.
 *   UPDATE  the reference's _update_results, _reward_map and _update_pheromone bit for bit: M, m = max, min reward of the
 *           instance's ants; the lowest ant with reward M is the iteration's best and replaces final_reward /
 *           final_actions when has_best == 0 (first iteration) or final_reward <= M; v_j = ((r_j - m) / (M - m))^2 * Q
 *           (NaN when M == m, as the reference); delta[a_t][a_t+1] += v_j for ants in ascending order over the N - 1
 *           directed edges t = 0 .. N - 2 (no closing edge, nothing symmetric); delta[0][0] = 0;
 *           pheromone = pheromone * decay + delta.
 * phases = SAMPLE | UPDATE runs `iterations` whole iterations (locs required). One phase alone runs once (iterations == 1):
 * SAMPLE writes actions / reward (reward only with locs), UPDATE reads them.
 * Up to rl4co_aco_tsp_lds_nodes() nodes L and the pheromone live in LDS; above, up to 1024, `pheromone` is updated in place
 * and L / delta use `logits_scratch`.
 * Sticky bits: RL4CO_EBIT_NAN_LOGIT (a feasible logit is NaN), RL4CO_EBIT_NEG_INF_LOGP (chosen log-prob not above -1000),
 * RL4CO_EBIT_INFEASIBLE (every feasible logit -inf: the lowest feasible node is taken; or a forced node already visited),
 * RL4CO_EBIT_TOUR_INDEX (a start node, forced action or UPDATE-only input action outside [0, N): that instance is left
 * untouched).
 * -------------------------------------------------------------------------- */
#define RL4CO_ACO_SAMPLE 1
#define RL4CO_ACO_UPDATE 2

typedef struct rl4co_aco_tsp_args {
  int32_t B;                /* instances (= workgroups), >= 1                               */
  int32_t N;                /* nodes, 2 .. 1024                                             */
  int32_t n_ants;           /* >= 1; n_ants * B <= 2^31 - 1                                 */
  int32_t iterations;       /* >= 1; 1 unless both phases are set                           */
  int32_t phases;           /* RL4CO_ACO_SAMPLE | RL4CO_ACO_UPDATE                          */
  int32_t has_best;         /* 0: final_reward / final_actions hold nothing yet             */
  float alpha;
  float beta;
  float decay;
  float Q;
  float temperature;        /* > 0                                                          */
  int32_t reserved0;        /* 0                                                            */
  uint64_t philox_seed;     /* in-kernel noise when ln_noise == NULL                        */
  uint64_t philox_offset;
  const uint64_t* philox_seed_dev; /* optional device word XOR-ed into philox_seed          */
  const float* log_heuristic;   /* [B,N,N] (SAMPLE)                                         */
  float* pheromone;             /* [B,N,N] in / out                                         */
  const float* locs;            /* [B,N,2]; NULL allowed for one phase alone (no reward)    */
  const int64_t* start_nodes;   /* [iterations,rows] (SAMPLE)                               */
  const float* ln_noise;        /* [iterations,N-1,rows,N] or NULL                          */
  const int64_t* forced_actions;/* [rows,N] or NULL (SAMPLE, iterations == 1)               */
  float* logits_scratch;        /* [B,N,N]; required above rl4co_aco_tsp_lds_nodes()        */
  int64_t* actions;             /* [rows,N] last iteration's tours (UPDATE alone: input)    */
  float* reward;                /* [rows] last iteration's rewards (UPDATE alone: input)    */
  float* logps;                 /* [rows,N] or NULL                                         */
  float* all_logps;             /* [rows,N,N] or NULL                                       */
  int64_t* iter_actions;        /* [iterations,rows,N] or NULL                              */
  float* iter_reward;           /* [iterations,rows] or NULL                                */
  float* final_reward;          /* [B] in / out (UPDATE)                                    */
  int64_t* final_actions;       /* [B,N] in / out (UPDATE)                                  */
  float* final_reward_cache;    /* [iterations,B] or NULL                                   */
  int32_t* err;                 /* sticky error bits                                        */
} rl4co_aco_tsp_args;

int rl4co_aco_tsp(const rl4co_aco_tsp_args* args, void* stream);
/* Largest N at which rl4co_aco_tsp keeps the logits and the pheromone in LDS (the kernel's LDS budget, aco_tsp.hip header). */
int rl4co_aco_tsp_lds_nodes(void);

/* --------------------------------------------------------------------------
 * The backward of rl4co_aco_tsp's SAMPLE phase with alpha = beta = 1 and a pheromone of ones (DeepACO's training path,
 * models/zoo/deepaco/policy.py:138-163): the gradient of the ants' log-likelihoods with respect to the heatmap, fp32, one
 * launch (aco_tsp_grad.hip). Rows are ant-major as above. For the ant of row r = j * B + b with tour a_0 .. a_{N-1} and
 * step t = 1 .. N - 1: i = a_{t-1}, F = the nodes not among a_0 .. a_{t-1}, p = softmax(heatmap[b, i, F] / temperature) in
 * rl4co_aco_tsp's own order of operations (p_n = exp of the log-prob the forward reports),
 * g = grad_ll[r] + grad_steps[r, t], and for n in F
 *   grad_heatmap[b, i, n] += g * ((n == a_t) - p_n) / temperature.
 * Every word of grad_heatmap is written (0 where nothing contributes: the diagonal, the rows of refused instances). Each
 * word is a sum over the ants in ascending order: two launches, and any row_split, give identical bits. A step whose feasible
 * logits are all -inf contributes nothing; a -inf logit among finite ones gets gradient 0.
 * Grid B x row_split: workgroup s of an instance takes the heatmap rows i = s (mod row_split).
 * Per instance, before anything is read through an action: an action outside [0, N) sets RL4CO_EBIT_TOUR_INDEX, a row that
 * is not a permutation of 0 .. N - 1 sets RL4CO_EBIT_INVALID_TOUR; that instance's gradient is all zeros.
 * -------------------------------------------------------------------------- */
typedef struct rl4co_aco_tsp_grad_args {
  int32_t B;                /* instances, >= 1                                              */
  int32_t N;                /* nodes, 2 .. 1024                                             */
  int32_t n_ants;           /* >= 1; n_ants * B <= 2^31 - 1                                 */
  int32_t row_split;        /* workgroups per instance, 1 .. N                              */
  float temperature;        /* > 0; the forward's                                           */
  int32_t reserved0;        /* 0                                                            */
  const float* heatmap;     /* [B,N,N] the logits the forward sampled from (not divided)    */
  const int64_t* actions;   /* [rows,N] the ants' tours                                     */
  const float* grad_ll;     /* [rows] upstream gradient of each row's summed log-likelihood */
  const float* grad_steps;  /* [rows,N] upstream gradient of the per-step log-probs or NULL; column 0 is ignored */
  uint16_t* pos_scratch;    /* [B*row_split,n_ants,N]; required when n_ants * N > rl4co_aco_tsp_grad_lds_entries(); used
                               whenever it is not NULL                                      */
  float* grad_heatmap;      /* [B,N,N] out                                                  */
  int32_t* err;             /* sticky error bits                                            */
} rl4co_aco_tsp_grad_args;

int rl4co_aco_tsp_logp_grad(const rl4co_aco_tsp_grad_args* args, void* stream);
/* Largest n_ants * N whose inverse-permutation table rl4co_aco_tsp_logp_grad keeps in LDS (aco_tsp_grad.hip header). */
int rl4co_aco_tsp_grad_lds_entries(void);

/* --------------------------------------------------------------------------
 * The backward of the SAMPLE phases of rl4co_aco_cvrp and rl4co_aco_prize with alpha = beta = 1 and a pheromone of ones
 * (DeepACO's training path on the depot graphs): the gradient of the ants' log-likelihoods with respect to the heatmap,
 * fp32, one launch (aco_depot_grad.hip). N is the heatmap side with the depot as node 0, C = N - 1; rows are ant-major and
 * W wide as the forward writes them (CVRP W = max(C + 1, 2 C - 1); OP, PCTSP W = N), zero-filled after each row's length.
 * For the ant of row r = j * B + b and every step t below the row's length (step 0 included; with `multistart` column 0 is
 * a given customer and contributes nothing): i = the node the ant leaves (the depot for t = 0, else a_{t-1}), F = the
 * environment's feasible set at that step in the forward's own fp32 expressions, p = softmax(heatmap[b, i, F] /
 * temperature) in the forward's order of operations, g = grad_ll[r] + grad_steps[r, t], and for n in F
 *   grad_heatmap[b, i, n] += g * ((n == a_t) - p_n) / temperature.
 * Every word of grad_heatmap is written (0 where nothing contributes). Each word is a sum in (ant, step) order: two
 * launches, any row_split and either table tier give identical bits. A step whose feasible logits are all -inf contributes
 * nothing; a -inf logit among finite ones gets gradient 0.
 * Grid B x row_split: workgroup s of an instance takes the heatmap rows i = s (mod row_split).
 * Per instance, before any gradient is written, the rows are replayed once: an action outside [0, N) (or a multistart start
 * that is the depot) sets RL4CO_EBIT_TOUR_INDEX, a customer taken twice RL4CO_EBIT_INVALID_TOUR, a taken action that is
 * infeasible under the environment's rule or a row not done after W actions RL4CO_EBIT_INFEASIBLE; that instance's gradient
 * is all zeros, other instances are untouched.
 * -------------------------------------------------------------------------- */
typedef struct rl4co_aco_depot_grad_args {
  int32_t env;              /* RL4CO_ENV_CVRP, RL4CO_ENV_OP or RL4CO_ENV_PCTSP                */
  int32_t B;                /* instances, >= 1                                              */
  int32_t N;                /* nodes with the depot, 2 .. 1024                              */
  int32_t n_ants;           /* >= 1; n_ants * B <= 2^31 - 1                                 */
  int32_t row_split;        /* workgroups per instance, 1 .. N                              */
  int32_t multistart;       /* CVRP: 1 = column 0 is a given customer start; else 0         */
  float temperature;        /* > 0; the forward's                                           */
  int32_t reserved0;        /* 0                                                            */
  const float* heatmap;     /* [B,N,N] the logits the forward sampled from (not divided)    */
  const int64_t* actions;   /* [rows,W] the ants' rows                                      */
  const float* grad_ll;     /* [rows] upstream gradient of each row's summed log-likelihood */
  const float* grad_steps;  /* [rows,W] upstream gradient of the per-step log-probs or NULL */
  const float* locs;        /* [B,N,2] OP                                                   */
  const float* demand;      /* [B,C] CVRP                                                   */
  const float* vehicle_capacity; /* [B] CVRP                                                */
  const float* prize;       /* [B,N] PCTSP (the prize the environment steps with)           */
  const float* max_length;  /* [B,N] OP (the environment's per-node table)                  */
  void* scratch;            /* B * row_split * rl4co_aco_depot_grad_scratch_bytes(n_ants, N) bytes; required when
                               n_ants * N > rl4co_aco_depot_grad_lds_entries(); used whenever it is not NULL */
  float* grad_heatmap;      /* [B,N,N] out                                                  */
  int32_t* err;             /* sticky error bits                                            */
} rl4co_aco_depot_grad_args;

int rl4co_aco_depot_logp_grad(const rl4co_aco_depot_grad_args* args, void* stream);
/* Largest n_ants * N whose replay table rl4co_aco_depot_logp_grad keeps in LDS (aco_depot_grad.hip header). */
int rl4co_aco_depot_grad_lds_entries(void);
/* Bytes of `scratch` one workgroup takes for its table (16-byte multiple); -1 outside the served sizes. */
int64_t rl4co_aco_depot_grad_scratch_bytes(int n_ants, int N);

/* --------------------------------------------------------------------------
 * Ant System search on a heatmap for CVRP (the same reference class with CVRPEnv) as ONE launch, one workgroup per
 * instance (aco_cvrp.hip). N is the heatmap side with the depot as node 0, C = N - 1 the customers, rows = n_ants * B
 * ant-major as in rl4co_aco_tsp, and W = max(C + 1, 2 C - 1) the longest action row the reference can produce.
 *   SAMPLE  L as in rl4co_aco_tsp. An ant carries CVRPEnv's state (cvrp/env.py:66-136) in fp32: used = (used +
 *           demand[a - 1]) * (a != 0); customer c is infeasible when visited or demand[c - 1] + used >
 *           vehicle_capacity + 1e-5f; the depot is infeasible when the ant stands on it and some customer is feasible;
 *           the row is done when every customer has been visited and action 0 has been taken at least once. With
 *           start_nodes == NULL (multisample) every ant starts at the depot and samples its first action from row 0 of L;
 *           with start_nodes (multistart) column 0 of `actions` is the given customer with log-prob 0, stepped through the
 *           state. A step is rl4co_aco_tsp's over the feasible nodes; ln_noise is [iterations, W, rows, N] (step t reads
 *           [it][t][row]; t = 0 is unused in multistart mode), the Philox step counter is philox_offset + it * W + t.
 *           An ant stops at done: lengths[row] counts its actions, the rest of the row is 0 (log-probs 0). A row not done
 *           after W actions (a demand above the capacity) raises RL4CO_EBIT_INFEASIBLE and ends there.
 *           REWARD WIDTH: the reward is minus the closed length of [depot, actions[0 .. W-1]] at the fixed width W,
 *           bit-equal to rl4co_tour_length_f32 with prepend_depot on the W-wide zero-padded row. The reference trims a
 *           batch to its longest row before it sums, which changes only the association of the sum (trailing depot
 *           segments are exactly 0) and depends on the other instances; this kernel does not follow that.
 *   UPDATE  rl4co_aco_tsp's over the whole padded row of width T (SAMPLE: T = W): edges (a_t, a_t+1), t = 0 .. T - 2, for
 *           ants in ascending order, (0, 0) edges skipped (the reference zeroes delta[0][0] afterwards);
 *           final_iteration[b] = iteration_base + it where iteration `it` replaced the record of instance b.
 * phases, the one-phase-alone rule, the LDS tier (rl4co_aco_cvrp_lds_nodes(), logits_scratch above it) and the sticky bits
 * are rl4co_aco_tsp's; RL4CO_EBIT_INFEASIBLE also covers a forced node that is infeasible and the row that is not done
 * after W actions; RL4CO_EBIT_TOUR_INDEX covers a start node outside [1, N) and a forced / UPDATE-only action outside
 * [0, N): that instance is left untouched.
 * -------------------------------------------------------------------------- */
typedef struct rl4co_aco_cvrp_args {
  int32_t B;                /* instances (= workgroups), >= 1                               */
  int32_t N;                /* nodes with the depot, 2 .. 1024                              */
  int32_t n_ants;           /* >= 1; n_ants * B <= 2^31 - 1                                 */
  int32_t iterations;       /* >= 1; 1 unless both phases are set                           */
  int32_t phases;           /* RL4CO_ACO_SAMPLE | RL4CO_ACO_UPDATE                          */
  int32_t has_best;         /* 0: final_reward / final_actions hold nothing yet             */
  int32_t T;                /* width of actions / final_actions: W with SAMPLE, else >= 2   */
  int32_t iteration_base;   /* added to the iteration index written to final_iteration      */
  float alpha;
  float beta;
  float decay;
  float Q;
  float temperature;        /* > 0                                                          */
  int32_t reserved0;        /* 0                                                            */
  uint64_t philox_seed;     /* in-kernel noise when ln_noise == NULL                        */
  uint64_t philox_offset;
  const uint64_t* philox_seed_dev; /* optional device word XOR-ed into philox_seed          */
  const float* log_heuristic;   /* [B,N,N] (SAMPLE)                                         */
  float* pheromone;             /* [B,N,N] in / out                                         */
  const float* locs;            /* [B,N,2], depot first; NULL allowed for one phase alone   */
  const float* demand;          /* [B,N-1] (SAMPLE)                                         */
  const float* vehicle_capacity;/* [B] (SAMPLE)                                             */
  const int64_t* start_nodes;   /* [iterations,rows] customers (multistart) or NULL         */
  const float* ln_noise;        /* [iterations,W,rows,N] or NULL                            */
  const int64_t* forced_actions;/* [rows,W] or NULL (SAMPLE, iterations == 1)               */
  float* logits_scratch;        /* [B,N,N]; required above rl4co_aco_cvrp_lds_nodes()       */
  int64_t* actions;             /* [rows,T] last iteration's rows (UPDATE alone: input)     */
  int32_t* lengths;             /* [rows] actions up to and including done (SAMPLE)         */
  float* reward;                /* [rows] last iteration's rewards (UPDATE alone: input)    */
  float* logps;                 /* [rows,W] or NULL                                         */
  float* all_logps;             /* [rows,W,N] or NULL                                       */
  int64_t* iter_actions;        /* [iterations,rows,W] or NULL                              */
  int32_t* iter_lengths;        /* [iterations,rows] or NULL                                */
  float* iter_reward;           /* [iterations,rows] or NULL                                */
  float* final_reward;          /* [B] in / out (UPDATE)                                    */
  int64_t* final_actions;       /* [B,T] in / out (UPDATE)                                  */
  int32_t* final_iteration;     /* [B] or NULL: written where the record is replaced        */
  float* final_reward_cache;    /* [iterations,B] or NULL                                   */
  int32_t* err;                 /* sticky error bits                                        */
} rl4co_aco_cvrp_args;

int rl4co_aco_cvrp(const rl4co_aco_cvrp_args* args, void* stream);
/* Largest N at which rl4co_aco_cvrp keeps the logits and the pheromone in LDS (the kernel's LDS budget, aco_cvrp.hip header). */
int rl4co_aco_cvrp_lds_nodes(void);

/* --------------------------------------------------------------------------
 * Ant System search on a heatmap for the prize problems, OP and PCTSP (the same reference class with OPEnv / PCTSPEnv), as
 * ONE launch (aco_prize.hip). env is RL4CO_ENV_OP or RL4CO_ENV_PCTSP (SPCTSP is PCTSP with the stochastic prize passed as
 * `prize`). N is the heatmap side with the depot as node 0, rows = n_ants * B ant-major as in rl4co_aco_tsp, and a row is
 * W = N wide: at most N - 1 customers, then the depot. One workgroup serves instances b, b + n_workgroups, ...
 * (n_workgroups == 0: one workgroup per instance); the results do not depend on n_workgroups.
 *   SAMPLE  L as in rl4co_aco_tsp. Every ant starts at the depot with nothing visited and samples its first action from row
 *           0 of L. A distance is d(i, j) = sqrtf(fmaf(dy, dy, dx * dx)), dx = x_j - x_i, dy = y_j - y_i.
 *           OP (op/env.py:67-154): state cur, visited (the depot included), tour_length, the step index; customer j is
 *           infeasible when visited, when the depot has been visited, or when tour_length + d(cur, j) > max_length[j]
 *           (`max_length` is the environment's per-node table: the budget minus the node's distance to the depot minus
 *           1e-6); the depot is always feasible; a step adds d(cur, a) to tour_length; done = (a == 0 and t > 0), so a row
 *           may take the depot at step 0 and again at step 1.
 *           PCTSP (pctsp/env.py:62-144): state cur, visited, cur_total_prize, the step index; customer j is infeasible
 *           when visited or when the depot has been visited; the depot is infeasible while cur_total_prize < 1 and an
 *           unvisited customer remains; a step adds prize[a]; done = (t > 0 and a == 0).
 *           A step is rl4co_aco_tsp's over the feasible nodes; ln_noise is [iterations, W, rows, N] (step t reads
 *           [it][t][row]), the Philox step counter is philox_offset + it * W + t. An ant stops at done: lengths[row]
 *           counts its actions, the rest of the row is 0 (log-probs 0).
 *   REWARD  at the fixed width W, every sum in rl4co_tour_length_f32's order (lds_tour_reward.h: 8 lanes, 4 accumulators,
 *           the 4-level cascade) over the W-wide zero-filled row. OP: the sum of prize[a_t], t = 0 .. W - 1. PCTSP:
 *           S - (len + P) with S the sum of penalty[a_t] over the row, len the closed length of [depot, a_0 .. a_{W-1}]
 *           (rl4co_tour_length_f32 with prepend_depot) and P the sum of penalty[1 .. N - 1].
 *   UPDATE  rl4co_aco_cvrp's ((0, 0) edges skipped, final_iteration, rows of any width T >= 2 with UPDATE alone).
 * phases, the one-phase-alone rule, the LDS tier (rl4co_aco_prize_lds_nodes(env), logits_scratch above it) and the sticky
 * bits are rl4co_aco_cvrp's; RL4CO_EBIT_TOUR_INDEX covers a forced / UPDATE-only action outside [0, N): that instance is
 * left untouched.
 * -------------------------------------------------------------------------- */
typedef struct rl4co_aco_prize_args {
  int32_t B;                /* instances, >= 1                                              */
  int32_t N;                /* nodes with the depot, 2 .. 1024                              */
  int32_t n_ants;           /* >= 1; n_ants * B <= 2^31 - 1                                 */
  int32_t iterations;       /* >= 1; 1 unless both phases are set                           */
  int32_t phases;           /* RL4CO_ACO_SAMPLE | RL4CO_ACO_UPDATE                          */
  int32_t has_best;         /* 0: final_reward / final_actions hold nothing yet             */
  int32_t T;                /* width of actions / final_actions: W = N with SAMPLE, else >= 2 */
  int32_t iteration_base;   /* added to the iteration index written to final_iteration      */
  int32_t env;              /* RL4CO_ENV_OP or RL4CO_ENV_PCTSP                              */
  int32_t n_workgroups;     /* 0: B; else 1 .. B workgroups striding over the instances     */
  float alpha;
  float beta;
  float decay;
  float Q;
  float temperature;        /* > 0                                                          */
  int32_t reserved0;        /* 0                                                            */
  uint64_t philox_seed;     /* in-kernel noise when ln_noise == NULL                        */
  uint64_t philox_offset;
  const uint64_t* philox_seed_dev; /* optional device word XOR-ed into philox_seed          */
  const float* log_heuristic;   /* [B,N,N] (SAMPLE)                                         */
  float* pheromone;             /* [B,N,N] in / out                                         */
  const float* locs;            /* [B,N,2], depot first (SAMPLE)                            */
  const float* prize;           /* [B,N], 0 at the depot (SAMPLE)                           */
  const float* penalty;         /* [B,N], 0 at the depot (SAMPLE, PCTSP)                    */
  const float* max_length;      /* [B,N] per-node entry limits (SAMPLE, OP)                 */
  const float* ln_noise;        /* [iterations,W,rows,N] or NULL                            */
  const int64_t* forced_actions;/* [rows,W] or NULL (SAMPLE, iterations == 1)               */
  float* logits_scratch;        /* [B,N,N]; required above rl4co_aco_prize_lds_nodes(env)   */
  int64_t* actions;             /* [rows,T] last iteration's rows (UPDATE alone: input)     */
  int32_t* lengths;             /* [rows] actions up to and including done (SAMPLE)         */
  float* reward;                /* [rows] last iteration's rewards (UPDATE alone: input)    */
  float* logps;                 /* [rows,W] or NULL                                         */
  float* all_logps;             /* [rows,W,N] or NULL                                       */
  int64_t* iter_actions;        /* [iterations,rows,W] or NULL                              */
  int32_t* iter_lengths;        /* [iterations,rows] or NULL                                */
  float* iter_reward;           /* [iterations,rows] or NULL                                */
  float* final_reward;          /* [B] in / out (UPDATE)                                    */
  int64_t* final_actions;       /* [B,T] in / out (UPDATE)                                  */
  int32_t* final_iteration;     /* [B] or NULL: written where the record is replaced        */
  float* final_reward_cache;    /* [iterations,B] or NULL                                   */
  int32_t* err;                 /* sticky error bits                                        */
} rl4co_aco_prize_args;

int rl4co_aco_prize(const rl4co_aco_prize_args* args, void* stream);
/* Largest N at which rl4co_aco_prize keeps the logits and the pheromone in LDS for `env` (aco_prize.hip header); -1 for an
 * environment it does not serve. */
int rl4co_aco_prize_lds_nodes(int env);

/* --------------------------------------------------------------------------
 * Greedy and top-k / top-p (nucleus) decoding of a heatmap (utils/decoding.py:109-188 under NonAutoregressiveDecoder; the
 * reference's NARGNNPolicy validates and tests with multistart_greedy and decodes its large graphs with top_k): the three
 * searches and the two gradients above with one options struct behind their own, unchanged argument struct. With every
 * option off (a zero-initialised struct) an *_opts entry point IS the entry point without the suffix: the same kernel
 * instantiation, the same bits; rl4co_aco_tsp(args, stream) is rl4co_aco_tsp_opts(args, &zeros, stream), and so on.
 *   top_k   0 < top_k < the step's number of feasible nodes: the feasible logits below the top_k-th largest are removed
 *           (ties at that value stay; a feasible -inf counts, so the threshold can be -inf and nothing is below it).
 *   top_p   0 < top_p < 1, after top_k and over its survivors: in (logit, node) ascending order, nodes are removed while
 *           their cumulative mass is <= (1 - top_p) Z; masses are exp(z - zmax) in the step's own order of sums. The
 *           largest logit is never removed.
 *           Everything after the filter (the log-softmax statistics, the log-probs, the argmax, all_logps) runs on the
 *           kept set: a removed node has log-prob -inf, and a forced action outside the kept set gets -inf and raises
 *           RL4CO_EBIT_NEG_INF_LOGP ("Logprobs should not be -inf").
 *   greedy  1: the chosen node is the argmax of the log-probs over the kept set, the lowest node on equal values; no noise
 *           is read and no Philox word is drawn (ln_noise must be NULL). The log-prob is reported as in sampling. The
 *           gradients ignore it.
 * The gradients recompute each step's kept set from the row's logits and the step's feasible set in the forward's own
 * text and run g * ((n == a_t) - p_n) / temperature over the kept nodes only: a removed node gets 0. Ascending-ant sums,
 * no float atomics, identical bits for any row_split and the per-instance refusals hold as without the filter.
 * -------------------------------------------------------------------------- */
typedef struct rl4co_heatmap_decode_opts {
  int32_t greedy;           /* 0 sample, 1 argmax of the log-probs (searches; ignored by the gradients) */
  int32_t top_k;            /* >= 0; 0 or >= the feasible nodes: off                          */
  float top_p;              /* 0 .. 1; 0 and 1: off                                           */
  int32_t reserved0;        /* 0                                                              */
} rl4co_heatmap_decode_opts;

int rl4co_aco_tsp_opts(const rl4co_aco_tsp_args* args, const rl4co_heatmap_decode_opts* opts, void* stream);
int rl4co_aco_cvrp_opts(const rl4co_aco_cvrp_args* args, const rl4co_heatmap_decode_opts* opts, void* stream);
int rl4co_aco_prize_opts(const rl4co_aco_prize_args* args, const rl4co_heatmap_decode_opts* opts, void* stream);
int rl4co_aco_tsp_logp_grad_opts(const rl4co_aco_tsp_grad_args* args, const rl4co_heatmap_decode_opts* opts, void* stream);
int rl4co_aco_depot_logp_grad_opts(const rl4co_aco_depot_grad_args* args, const rl4co_heatmap_decode_opts* opts,
                                   void* stream);

/* --------------------------------------------------------------------------
 * Neural-guided local search for TSP (DeepACO's NLS: AntSystem.local_search with use_nls, antsystem.py:173-230) as ONE
 * launch, one workgroup per tour row (tsp_nls.hip). Row r uses instance r % n_instances (the ant-major rows of
 * rl4co_aco_tsp); neither `locs` nor `perturb_distances` is tiled per ant. Per row, with two_opt the search of
 * rl4co_tsp_two_opt (the same text, every rule above: association, lowest (i, j) on ties, -1e-6 in double):
 *   cur  = two_opt(real, cur, ls_max_iterations)
 *   best = cur (written to out_actions[row]); best_r = reward(cur)
 *   n_perturbations times:
 *     cur = two_opt(perturb, cur, perturb_max_iterations)
 *     cur = two_opt(real,    cur, ls_max_iterations)
 *     r   = reward(cur);  if r > best_r (fp32, NaN never wins): out_actions[row] = cur, best_r = r
 *     (cur carries on whether or not it won)
 *   out_reward[row] = best_r
 * `real` is d[a][b] = sqrtf(fmaf(dy, dy, dx * dx)) from `locs` with d[a][a] = 1e9; `perturb` is perturb_distances (given
 * WITHOUT the diagonal, may be asymmetric) with 1e9 added on its diagonal. reward is minus the closed tour length from
 * `locs`, bit-equal to rl4co_tour_length_f32's. `scans` holds the scans of each of the 1 + 2 * n_perturbations searches,
 * counted as rl4co_tsp_two_opt's `iterations`; `accepted` the rounds that replaced the best tour.
 * Up to rl4co_tsp_nls_lds_nodes() nodes one matrix slot in LDS is restaged at each phase switch; above, up to 1024, the real
 * phases compute distances from coordinates in LDS and the perturbation phases read global memory.
 * A tour with an index outside [0, N) sets RL4CO_EBIT_TOUR_INDEX and is copied through unchanged with reward NaN, zero
 * scans and zero accepted. out_actions == actions (in place) is allowed.
 * -------------------------------------------------------------------------- */
typedef struct rl4co_tsp_nls_args {
  int32_t R;                      /* tour rows (= workgroups), >= 1, R % n_instances == 0    */
  int32_t n_instances;            /* I >= 1; row r uses instance r % I                       */
  int32_t N;                      /* nodes, 2 .. 1024                                        */
  int32_t T;                      /* tour length, 1 .. 1024                                  */
  int32_t ls_max_iterations;      /* >= 0: scans of a search over the real distances         */
  int32_t perturb_max_iterations; /* >= 0: scans of a search over perturb_distances          */
  int32_t n_perturbations;        /* >= 0 rounds                                             */
  int32_t reserved0;              /* 0                                                       */
  const float* locs;              /* [I,N,2]                                                 */
  const float* perturb_distances; /* [I,N,N], without the 1e9 diagonal                       */
  const int64_t* actions;         /* [R,T]                                                   */
  int64_t* out_actions;           /* [R,T] the best tour of each row                         */
  float* out_reward;              /* [R] its reward                                          */
  int32_t* scans;                 /* [R, 1 + 2 * n_perturbations] or NULL                    */
  int32_t* accepted;              /* [R] or NULL                                             */
  int32_t* err;                   /* sticky error bits                                       */
} rl4co_tsp_nls_args;

int rl4co_tsp_nls(const rl4co_tsp_nls_args* args, void* stream);
/* Largest N whose distance matrix rl4co_tsp_nls keeps in LDS (the kernel's LDS budget, tsp_nls.hip header). */
int rl4co_tsp_nls_lds_nodes(void);

/* --------------------------------------------------------------------------
 * DeepACO's heatmap encoder for TSP (NARGNNEncoder in inference: models/zoo/nargnn/encoder.py, the anisotropic edge-gated
 * GNN of models/nn/graph/gnn.py and the EdgeHeatmapGenerator MLP) as ONE launch in fp32, one workgroup per instance with a
 * grid-stride loop over the instances (nargnn.hip). The TSP graph is regular: node u has exactly K out-edges (u, v) to
 * neighbors[b][u][0 .. K-1], so the edge state is a dense [N, K, D] array, D = 64, and node u pools over its own K rows.
 *   x = silu(init(locs));  w = silu(edge_embed(edge_cost))
 *   L times, both lines reading the layer's incoming x and w:
 *     x <- x + silu(bn_v(v_lin1(x)[u] + mean_k(sigmoid(w[u][k]) * v_lin2(x)[v])))
 *     w <- w + silu(bn_e(e_lin(w) + v_lin3(x)[u] + v_lin4(x)[v]))
 *   h = sigmoid(out(silu(lin_{H-1}(... silu(lin_1(w))))))
 *   heatmap[b][u][v] = log(h + small_value) at the K neighbours of u, fill_value everywhere else (diagonal included).
 * silu(y) = y / (1 + exp(-y)); the batch norms are eval-mode, folded by the host into a per-channel scale and shift
 * (y * scale + shift). The 64-long dot products run on v_mfma_f32_16x16x4_f32 (the hardware's summation order).
 * Three tiers by where the state lives (nargnn_shared.h header): up to rl4co_nargnn_lds_nodes(K) nodes the edge state and the
 * two gathered node planes stay in LDS; above, the edge state lives in `scratch`; above 300 nodes every plane does.
 * `scratch` holds n_workgroups * rl4co_nargnn_scratch_bytes(N, K) bytes, 16-byte aligned.
 * A neighbour index outside [0, N) sets RL4CO_EBIT_TOUR_INDEX; that instance's outputs are left untouched.
 * -------------------------------------------------------------------------- */
typedef struct rl4co_nargnn_args {
  int32_t B;                /* instances, >= 1                                              */
  int32_t N;                /* nodes, 2 .. 1024                                             */
  int32_t K;                /* out-edges per node, 1 .. min(N - 1, 256)                     */
  int32_t D;                /* embedding width: 64                                          */
  int32_t L;                /* GNN layers, >= 0                                             */
  int32_t H;                /* heatmap MLP layers with the output layer, >= 1               */
  int32_t n_workgroups;     /* grid, 1 .. B                                                 */
  int32_t reserved0;        /* 0                                                            */
  float small_value;        /* added to h before the log                                    */
  float fill_value;         /* log(small_value) as the host computed it                     */
  const float* locs;        /* [B,N,2]                                                      */
  const int32_t* neighbors; /* [B,N,K]                                                      */
  const float* edge_cost;   /* [B,N,K]                                                      */
  const float* init_w;      /* [D,2]                                                        */
  const float* init_b;      /* [D]                                                          */
  const float* edge_w;      /* [D] (Linear(1, D))                                           */
  const float* edge_b;      /* [D]                                                          */
  const float* lin_w;       /* [L,5,D,D]: v_lin1 .. v_lin4, e_lin; NULL allowed when L == 0  */
  const float* lin_b;       /* [L,5,D]                                                      */
  const float* bn;          /* [L,2,2,D]: (v_bn, e_bn) x (scale, shift)                     */
  const float* mlp_w;       /* [H-1,D,D]; NULL allowed when H == 1                          */
  const float* mlp_b;       /* [H-1,D] or NULL (linear_bias = False)                        */
  const float* out_w;       /* [D]                                                          */
  const float* out_b;       /* [1] or NULL                                                  */
  float* scratch;           /* n_workgroups * rl4co_nargnn_scratch_bytes(N, K) bytes        */
  int64_t scratch_bytes;
  float* heatmap;           /* [B,N,N] out                                                  */
  float* node_embed;        /* [B,N,D] out: init(locs), before the activation               */
  int32_t* err;             /* sticky error bits                                            */
} rl4co_nargnn_args;

int rl4co_nargnn_heatmap(const rl4co_nargnn_args* args, void* stream);
/* Largest N at which rl4co_nargnn_heatmap keeps the edge state of K out-edges per node in LDS (nargnn_shared.h header). */
int rl4co_nargnn_lds_nodes(int K);
/* Bytes of `scratch` one workgroup needs at this shape (0 < result; the tier is the kernel's own choice). */
int64_t rl4co_nargnn_scratch_bytes(int N, int K);

/* --------------------------------------------------------------------------
 * The same encoder for the depot graphs of CVRP, OP and PCTSP (NARGNNEncoder(env_name=...) in inference with
 * VRP / OP / PCTSPInitEmbedding and CVRPEdgeEmbedding, env_embeddings/edge.py:119-176) as ONE launch in fp32
 * (nargnn_depot.hip). Node 0 is the depot, nodes 1 .. C = N - 1 the customers. Customer u has K + 1 out-edges: to
 * neighbors[b][u-1][0 .. K-1] (customers, values in 1 .. N-1) and to the depot; the depot has C out-edges, one to every
 * customer: C (K + 2) edges. The layer equations are rl4co_nargnn_args', the mean pooled by SOURCE node: over K + 1
 * rows for a customer, over C rows for the depot (eight partial sums).
 *   x[0] = silu(depot(locs[0]));  x[u] = silu(init(locs[u], feats[u-1]));  w = silu(edge_embed(cost))
 *   heatmap[b][u][v_k], heatmap[b][u][0] and heatmap[b][0][i] = log(h + small_value); fill_value everywhere else
 *   (the diagonal and heatmap[b][0][0] included).
 * feats: CVRP demand; OP prize[:, 1:]; PCTSP (expected_prize, penalty[:, 1:]). depot_cost[b][u-1] is the one distance of
 * (u -> 0) and (0 -> u). The layer, MLP and output parameters are packed exactly as in rl4co_nargnn_args.
 * Tiers as above with C (K + 2) edge rows: up to rl4co_nargnn_depot_lds_nodes(K) nodes the edge state and the two
 * gathered node planes stay in LDS; above, the edge state lives in `scratch`; above 300 nodes every plane does.
 * `scratch` holds n_workgroups * rl4co_nargnn_depot_scratch_bytes(N, K) bytes, 16-byte aligned.
 * A neighbour index outside [1, N) (0, the depot, included: it would repeat the depot edge) sets
 * RL4CO_EBIT_TOUR_INDEX; that instance's outputs are left untouched.
 * -------------------------------------------------------------------------- */
typedef struct rl4co_nargnn_depot_args {
  int32_t B;                /* instances, >= 1                                              */
  int32_t N;                /* nodes with the depot, 3 .. 1024                              */
  int32_t K;                /* customer neighbours per customer, 1 .. min(N - 2, 256)       */
  int32_t F;                /* customer features behind the coordinates: 1 or 2             */
  int32_t D;                /* embedding width: 64                                          */
  int32_t L;                /* GNN layers, >= 0                                             */
  int32_t H;                /* heatmap MLP layers with the output layer, >= 1               */
  int32_t n_workgroups;     /* grid, 1 .. B                                                 */
  float small_value;        /* added to h before the log                                    */
  float fill_value;         /* log(small_value) as the host computed it                     */
  const float* locs;        /* [B,N,2]                                                      */
  const float* feats;       /* [B,N-1,F]                                                    */
  const int32_t* neighbors; /* [B,N-1,K], values in 1 .. N-1                                */
  const float* edge_cost;   /* [B,N-1,K]                                                    */
  const float* depot_cost;  /* [B,N-1]                                                      */
  const float* init_w;      /* [D,2+F] (customers)                                          */
  const float* init_b;      /* [D]                                                          */
  const float* depot_w;     /* [D,2]                                                        */
  const float* depot_b;     /* [D]                                                          */
  const float* edge_w;      /* [D] (Linear(1, D))                                           */
  const float* edge_b;      /* [D]                                                          */
  const float* lin_w;       /* [L,5,D,D]: v_lin1 .. v_lin4, e_lin; NULL allowed when L == 0  */
  const float* lin_b;       /* [L,5,D]                                                      */
  const float* bn;          /* [L,2,2,D]: (v_bn, e_bn) x (scale, shift)                     */
  const float* mlp_w;       /* [H-1,D,D]; NULL allowed when H == 1                          */
  const float* mlp_b;       /* [H-1,D] or NULL (linear_bias = False)                        */
  const float* out_w;       /* [D]                                                          */
  const float* out_b;       /* [1] or NULL                                                  */
  float* scratch;           /* n_workgroups * rl4co_nargnn_depot_scratch_bytes(N, K) bytes  */
  int64_t scratch_bytes;
  float* heatmap;           /* [B,N,N] out                                                  */
  float* node_embed;        /* [B,N,D] out: the init embeddings, before the activation      */
  int32_t* err;             /* sticky error bits                                            */
} rl4co_nargnn_depot_args;

int rl4co_nargnn_depot_heatmap(const rl4co_nargnn_depot_args* args, void* stream);
/* Largest N at which rl4co_nargnn_depot_heatmap keeps the (N - 1)(K + 2) edge rows in LDS (nargnn_shared.h header). */
int rl4co_nargnn_depot_lds_nodes(int K);
/* Bytes of `scratch` one workgroup needs at this shape (0 outside the supported range). */
int64_t rl4co_nargnn_depot_scratch_bytes(int N, int K);

/* --------------------------------------------------------------------------
 * The GNN stack of the TSP heatmap encoder in TRAIN mode and its backward (gnn.py:45-61 over the regular graph, batch
 * norms on BATCH statistics), fp32, nargnn_train.hip. Rows: n_v = B N node rows, n_e = B N K edge rows, all dense
 * [rows, D], D = 64; edge row e belongs to node i = e / K and points at node j = (i / N) N + neighbors[e].
 *   per layer, s = sigmoid(w0):
 *     pre_v[i] = v_lin1(x0)[i] + (1 / K) sum_k s[i,k] * v_lin2(x0)[j];   pre_e[e] = e_lin(w0)[e] + v_lin3(x0)[i] + v_lin4(x0)[j]
 *     per channel over ALL rows: mu, biased var, r = 1 / sqrt(var + eps); x = x0 + silu(gamma (pre_v - mu) r + beta), w alike
 * rl4co_nargnn_train_forward writes x_out, w_out, stats[l] = (mu_v, r_v, var_v, mu_e, r_e, var_e) and the saves in
 * `workspace`; rl4co_nargnn_train_backward, given the SAME workspace, inputs and parameters and the gradients of x_out and
 * w_out, writes the gradients of x_in, w_in and of every parameter. Every batch-wide reduction crosses a launch boundary
 * (per-workgroup partials, a finalize launch that combines them in a fixed order); there is no grid barrier and no
 * floating-point atomic: every output is bit-identical run to run. The variance is combined from per-workgroup
 * (count, mean, M2) by Chan's formula. The scatter to target nodes runs over the incoming-edge CSR: csr_ptr[j] ..
 * csr_ptr[j + 1] are the positions in csr_src of the edge rows e (ascending) that point at global node j.
 * A neighbour index outside [0, N) or a CSR that is not exactly that of `neighbors` sets RL4CO_EBIT_TOUR_INDEX, decided by
 * the first launch of either call before anything is read through them; the call's outputs are then left unwritten.
 * workspace floats, nv = 64 B N, ne = 64 B N K, P_v = min(ceil(B N / 64), 1024), P_e = min(ceil(B N K / 64), 1024):
 *   64 + max(L - 1, 0) (nv + ne) + L (2 nv + ne) + 5 nv + 2 ne + 192 (P_v + P_e) + 4160 (4 P_v + P_e) + 512
 * (the layers' x0 and w0 behind the first, pre_v, x2 and pre_e per layer; the node planes, the running gradients and gu_e;
 * the statistics partials; the weight-gradient partials; the backward's means).
 * -------------------------------------------------------------------------- */
typedef struct rl4co_nargnn_train_args {
  int32_t B;                  /* instances, >= 1                                              */
  int32_t N;                  /* nodes, 2 .. 1024; B N >= 2                                   */
  int32_t K;                  /* out-edges per node, 1 .. min(N - 1, 64)                      */
  int32_t D;                  /* embedding width: 64                                          */
  int32_t L;                  /* GNN layers, >= 1                                             */
  int32_t reserved0;          /* 0                                                            */
  float eps;                  /* the batch norms' eps                                         */
  int32_t reserved1;          /* 0                                                            */
  const int32_t* neighbors;   /* [B,N,K]                                                      */
  const int32_t* csr_ptr;     /* [B N + 1]                                                    */
  const int32_t* csr_src;     /* [B N K]                                                      */
  const float* x_in;          /* [B N, D]                                                     */
  const float* w_in;          /* [B N K, D]                                                   */
  const float* lin_w;         /* [L,5,D,D]: v_lin1 .. v_lin4, e_lin                           */
  const float* lin_b;         /* [L,5,D]                                                      */
  const float* bn_w;          /* [L,2,D]: gamma of (v_bn, e_bn)                               */
  const float* bn_b;          /* [L,2,D]: beta                                                */
  float* workspace;           /* rl4co_nargnn_train_workspace_bytes(B, N, K, L) bytes         */
  int64_t workspace_bytes;
  float* x_out;               /* [B N, D]       forward out                                   */
  float* w_out;               /* [B N K, D]     forward out                                   */
  float* stats;               /* [L,6,D]        forward out, backward in                      */
  const float* grad_x_out;    /* [B N, D]       backward in                                   */
  const float* grad_w_out;    /* [B N K, D]     backward in                                   */
  float* grad_x_in;           /* [B N, D]       backward out                                  */
  float* grad_w_in;           /* [B N K, D]     backward out                                  */
  float* grad_lin_w;          /* [L,5,D,D]      backward out                                  */
  float* grad_lin_b;          /* [L,5,D]        backward out                                  */
  float* grad_bn_w;           /* [L,2,D]        backward out                                  */
  float* grad_bn_b;           /* [L,2,D]        backward out                                  */
  int32_t* err;               /* sticky error bits                                            */
} rl4co_nargnn_train_args;

int rl4co_nargnn_train_forward(const rl4co_nargnn_train_args* args, void* stream);
int rl4co_nargnn_train_backward(const rl4co_nargnn_train_args* args, void* stream);
/* Bytes of `workspace` at this shape by the formula above (0 outside the supported range). */
int64_t rl4co_nargnn_train_workspace_bytes(int B, int N, int K, int L);

/* --------------------------------------------------------------------------
 * The same stack, train mode and backward, on the DEPOT graph of CVRP, OP and PCTSP (CVRPEdgeEmbedding: every customer's K
 * nearest customers plus the depot, the depot to every customer), fp32, nargnn_train.hip: the kernels of
 * rl4co_nargnn_train_* instantiated for a second graph. Node 0 of an instance is the depot, C = N - 1 are customers.
 * Rows: n_v = B N node rows, n_e = B E edge rows, E = C (K + 2), per instance in the reference's own order:
 *   [0, C K)             the kNN rows by source: row (i - 1) K + k is i -> neighbors[i - 1, k], a customer in 1 .. N - 1
 *   [C K, C K + C)       row C K + (i - 1) is i -> 0
 *   [C K + C, C (K + 2)) row C K + C + (i - 1) is 0 -> i
 * Source and target of a row are closed forms of (row, neighbors); no edge list is stored. deg(i), the out-degree, is
 * K + 1 for a customer (its K rows and its i -> 0 row) and C for the depot.
 *   per layer, s = sigmoid(w0), e: i -> j:
 *     pre_v[i] = v_lin1(x0)[i] + (1 / deg(i)) sum_{e out of i} s[e] * v_lin2(x0)[j];
 *     pre_e[e] = e_lin(w0)[e] + v_lin3(x0)[i] + v_lin4(x0)[j]
 *     per channel over ALL rows: mu, biased var, r = 1 / sqrt(var + eps); x = x0 + silu(gamma (pre_v - mu) r + beta), w alike
 * Forward, backward, statistics, determinism and the workspace are rl4co_nargnn_train_*'s, with E in place of N K:
 *   nv = 64 B N, ne = 64 B E, P_v = min(ceil(B N / 64), 1024), P_e = min(ceil(B E / 64), 1024), the same formula.
 * The depot's sums (its mean, its gradient sums: C terms) are eight interleaved partial sums, term t into partial t mod 8,
 * combined ((0 + 1) + (2 + 3)) + ((4 + 5) + (6 + 7)); every other node's sums run in row order.
 * The CSR runs over all n_e rows: csr_ptr[j] .. csr_ptr[j + 1] are the positions in csr_src of the edge rows (ascending)
 * whose target is global node j; the depot's in-degree is C, a customer's at least 1. A neighbour index outside [1, N)
 * (the depot is nobody's kNN neighbour) or a CSR that is not exactly that of the rows' closed-form targets sets
 * RL4CO_EBIT_TOUR_INDEX in the first launch of either call; the whole call is then refused (batch statistics tie the
 * instances together) and its outputs are left unwritten.
 * Served: B >= 1, 3 <= N <= 1024, 1 <= K <= min(N - 2, 64), L >= 1, B C (K + 2) <= 2^24.
 * -------------------------------------------------------------------------- */
typedef struct rl4co_nargnn_depot_train_args {
  int32_t B;                  /* instances, >= 1                                              */
  int32_t N;                  /* nodes with the depot, 3 .. 1024                              */
  int32_t K;                  /* kNN rows per customer, 1 .. min(N - 2, 64)                   */
  int32_t D;                  /* embedding width: 64                                          */
  int32_t L;                  /* GNN layers, >= 1                                             */
  int32_t reserved0;          /* 0                                                            */
  float eps;                  /* the batch norms' eps                                         */
  int32_t reserved1;          /* 0                                                            */
  const int32_t* neighbors;   /* [B,N-1,K], values in 1 .. N - 1                              */
  const int32_t* csr_ptr;     /* [B N + 1]                                                    */
  const int32_t* csr_src;     /* [B E]                                                        */
  const float* x_in;          /* [B N, D]                                                     */
  const float* w_in;          /* [B E, D]                                                     */
  const float* lin_w;         /* [L,5,D,D]: v_lin1 .. v_lin4, e_lin                           */
  const float* lin_b;         /* [L,5,D]                                                      */
  const float* bn_w;          /* [L,2,D]: gamma of (v_bn, e_bn)                               */
  const float* bn_b;          /* [L,2,D]: beta                                                */
  float* workspace;           /* rl4co_nargnn_depot_train_workspace_bytes(B, N, K, L) bytes   */
  int64_t workspace_bytes;
  float* x_out;               /* [B N, D]       forward out                                   */
  float* w_out;               /* [B E, D]       forward out                                   */
  float* stats;               /* [L,6,D]        forward out, backward in                      */
  const float* grad_x_out;    /* [B N, D]       backward in                                   */
  const float* grad_w_out;    /* [B E, D]       backward in                                   */
  float* grad_x_in;           /* [B N, D]       backward out                                  */
  float* grad_w_in;           /* [B E, D]       backward out                                  */
  float* grad_lin_w;          /* [L,5,D,D]      backward out                                  */
  float* grad_lin_b;          /* [L,5,D]        backward out                                  */
  float* grad_bn_w;           /* [L,2,D]        backward out                                  */
  float* grad_bn_b;           /* [L,2,D]        backward out                                  */
  int32_t* err;               /* sticky error bits                                            */
} rl4co_nargnn_depot_train_args;

int rl4co_nargnn_depot_train_forward(const rl4co_nargnn_depot_train_args* args, void* stream);
int rl4co_nargnn_depot_train_backward(const rl4co_nargnn_depot_train_args* args, void* stream);
/* Bytes of `workspace` at this shape (0 outside the served range). */
int64_t rl4co_nargnn_depot_train_workspace_bytes(int B, int N, int K, int L);

/* --------------------------------------------------------------------------
 * GFACS's log-partition head (the reference's models/zoo/gfacs/encoder.py:45-47, 62: Z_net = Linear(64, 64), SiLU,
 * Linear(64, Z) over the GNN stack's edge state, then a mean), forward and backward, fp32, nargnn_logz.hip. `w` is the
 * stack's output, flat and batch-major: rows = B E rows of 64 floats, instance 0's E rows first (E = N K for TSP,
 * (N - 1)(K + 2) for the depot graphs).
 *   score[r] = W2 silu(W1 w[r] + b1) + b2;   logZ[b] = (1 / E) sum of score[r] over b's group:
 *     RL4CO_LOGZ_POOL_REFERENCE  the rows r with r % B == b: gfacs/encoder.py:62 as written, reshape(-1, B, Z).mean(0),
 *                                which strides over the instances
 *     RL4CO_LOGZ_POOL_INSTANCE   instance b's own rows b E .. b E + E - 1
 * The hidden [rows, 64] is never written: the forward keeps it in the MFMA accumulators, the backward recomputes it.
 * rl4co_nargnn_logz_backward, given the same inputs and grad_logZ, writes the gradients of w and of the four parameters.
 * Every sum has a fixed order that depends on (B, E, pooling) alone (the pooled mean: 256 interleaved float64 sums per
 * group, halved 128, 64, ...; the parameter gradients: one partial per workgroup, combined in ascending order in float64);
 * no floating-point atomic, no grid barrier: every output is bit-identical run to run, and with B = 1 the two pooling
 * rules give the same bits.
 * Served: Z in {1, 2}, B >= 1, E >= 1, rows = B E <= 2^24. workspace floats: 2 rows + 4290 min(ceil(rows / 64), 1024).
 * -------------------------------------------------------------------------- */
#define RL4CO_LOGZ_POOL_REFERENCE 0
#define RL4CO_LOGZ_POOL_INSTANCE 1

typedef struct rl4co_nargnn_logz_args {
  int32_t B;                  /* instances, >= 1                                              */
  int32_t E;                  /* edge rows per instance, >= 1                                 */
  int32_t Z;                  /* outputs of the head (gfacs/encoder.py: z_out_dim), 1 or 2    */
  int32_t pooling;            /* RL4CO_LOGZ_POOL_*                                            */
  int64_t rows;               /* B E                                                          */
  const float* w;             /* [rows, 64]                                                   */
  const float* W1;            /* [64, 64]: Z_net.0.weight                                     */
  const float* b1;            /* [64]:     Z_net.0.bias                                       */
  const float* W2;            /* [Z, 64]:  Z_net.2.weight                                     */
  const float* b2;            /* [Z]:      Z_net.2.bias                                       */
  float* workspace;           /* rl4co_nargnn_logz_workspace_bytes(rows) bytes                */
  int64_t workspace_bytes;
  float* logZ;                /* [B, Z]         forward out                                   */
  const float* grad_logZ;     /* [B, Z]         backward in                                   */
  float* grad_w;              /* [rows, 64]     backward out                                  */
  float* grad_W1;             /* [64, 64]       backward out                                  */
  float* grad_b1;             /* [64]           backward out                                  */
  float* grad_W2;             /* [Z, 64]        backward out                                  */
  float* grad_b2;             /* [Z]            backward out                                  */
} rl4co_nargnn_logz_args;

/* gfacs/encoder.py:62: logZ = Z_net(edge_attr).reshape(-1, len(td), z_out_dim).mean(0) */
int rl4co_nargnn_logz_forward(const rl4co_nargnn_logz_args* args, void* stream);
/* the backward of gfacs/encoder.py:62 through Z_net to edge_attr and Z_net's parameters */
int rl4co_nargnn_logz_backward(const rl4co_nargnn_logz_args* args, void* stream);
/* Bytes of `workspace` for `rows` rows of gfacs/encoder.py's edge_attr (0 outside the served range). */
int64_t rl4co_nargnn_logz_workspace_bytes(int64_t rows);

/* --------------------------------------------------------------------------
 * a11-a13  fused encoder + decoder-cache fold on the matrix cores (inference rollouts).
 *
 * Replaces, per instance and in one launch: TSPInitEmbedding / VRPInitEmbedding
 * (models/nn/env_embeddings/init.py:55-68,115-136), GraphAttentionNetwork with L x
 * [x + MHA(x) -> Norm -> x + MLP(x) -> Norm] (models/nn/graph/attnnet.py:16-106,
 * nn/attention.py:110-134, nn/ops.py:30-54, nn/mlp.py:52-61; 8 heads, d = 128, FFN 512) and
 * AttentionModelDecoder._precompute_cache (zoo/am/decoder.py:201-228) in the folded form of
 * rl4co_am_decode_args. 16-bit MFMA inputs (act_dtype: bf16 or fp16), fp32 accumulation, 16-bit
 * residual stream (the reference's mixed-precision regimes, utils/trainer.py:57). Normalisation: norm = 0 is
 * batch norm in EVAL mode, passed as a per-channel (scale, shift) pair folded from the
 * running statistics; norm = 1 is instance norm (POMO), scale/shift = gamma/beta; norm = 2 is the
 * reference's "layer" normalisation (nn/ops.py:48-51: ONE mean and ONE unbiased variance over all N x 128
 * values of an instance, eps 1e-5, no affine) — scale is ignored, the 16-bit kernel reads the bias of the
 * GEMM in front of the norm (bo / b2) from the shift slot and adds it before the statistics (the fp32
 * kernel adds bo / b2 itself).
 * Train-mode batch statistics couple instances and stay on the torch path (which also
 * provides autograd). N <= rl4co_am_encoder_max_nodes().
 *
 * Weight matrices are nn.Linear weights [out,in] re-packed once per weight update into MFMA
 * fragment order: [out/32 tiles][in/16 ksteps][64 lanes][8] elements of act_dtype with lane = 32*hi + row,
 * element s = W[32*tile + row][16*kstep + 8*hi + s]   (rl4co_amd/encoder.py: pack_weight).
 * -------------------------------------------------------------------------- */
typedef struct rl4co_am_encoder_args {
  int32_t env;         /* RL4CO_ENV_TSP | RL4CO_ENV_CVRP (every depot env with a 3- or 4-feature customer embedding) | RL4CO_ENV_PDP */
  int32_t B;           /* instances                                                */
  int32_t N;           /* nodes incl. depot                                        */
  int32_t num_layers;  /* 3 (AM) / 6 (POMO)                                        */
  int32_t norm;        /* 0 = per-channel affine (batch norm, eval), 1 = instance, 2 = layer (nn/ops.py:48-51: one mean / one
                          unbiased variance per instance, no affine) — every entry point serves all three, the token-tile
                          ones through split half-layer kernels + a norm-apply kernel. What n*_scale / n*_shift hold:
                            0: scale = weight / sqrt(running_var + eps), shift = bias - running_mean * scale
                               (16-bit kernels: + the preceding GEMM's bias * scale; fp32 kernels add bo / b2 themselves)
                            1: gamma, beta (statistics per instance and channel over the nodes)
                            2: 16-bit kernels: scale unused, shift = the bias of the GEMM in front of the norm (out_proj /
                               the MLP's second linear: it does not cancel under a whole-instance mean and is added before
                               the statistics); fp32 kernels: unused (they add bo / b2 themselves) */
  int32_t cache_dtype; /* dtype of the three kvl planes written: RL4CO_DT_F32 or act_dtype */
  int32_t act_dtype;   /* 16-bit element type of the MFMA operands, the packed weights and the LDS residual stream:
                          RL4CO_DT_BF16 (autocast bfloat16) or RL4CO_DT_F16 (autocast float16, the reference's
                          default "16-mixed", utils/trainer.py:57: v_mfma_f32_32x32x16_f16, softmax always
                          max-subtracted — fp16 lacks the range of the bounded-score shortcut) */
  int32_t ctx_dtype;   /* (r06; was reserved0 = 0) element type of ctx_first / ctx_cur: RL4CO_DT_F32 (0, the default) or —
                          rl4co_am_encoder only, 16-bit planes — act_dtype: the tables written as dense 16-bit [B,N,128] rows
                          for rl4co_am_decode_args.ctx_dtype; every other entry point requires 0 */
  const float* locs;   /* [B,N,2] (CVRP: depot first, cvrp/env.py:108)             */
  const float* demand; /* [B,N-1] CVRP demand / OP prize / PCTSP expected prize     */
  const float* feature4; /* [B,N-1] PCTSP penalty / CVRPTW tw start (w_init is then [128,4] / [128,6]) or NULL */
  const float* feature5; /* [B,N-1] CVRPTW tw end, or NULL                          */
  const float* feature6; /* [B,N-1] CVRPTW service time, or NULL (feature4..6 are set together) */
  const float* w_init; /* [128,2] TSP / [128,3] CVRP customers / [128,4] PCTSP / [128,6] CVRPTW */
  const float* b_init; /* [128]                                                    */
  const float* w_depot; /* [128,2] depot environments                              */
  const float* b_depot; /* [128]                                                   */
  const float* w_extra; /* [128,2] RL4CO_ENV_PDP: the delivery embedding; w_init is then the pickup embedding */
  const float* b_extra; /* [128]     [128,4] over (x, y, x', y' of the paired delivery), init.py:335-360      */
  const void* wqkv_packed; /* [L] x packed [384,128]                               */
  const float* bqkv;       /* [L,384]                                              */
  const void* wo_packed;   /* [L] x packed [128,128]                               */
  const float* bo;         /* [L,128]                                              */
  const float* n1_scale;   /* [L,128]                                              */
  const float* n1_shift;   /* [L,128]                                              */
  const void* w1_packed;   /* [L] x packed [512,128]                               */
  const float* b1;         /* [L,512]                                              */
  const void* w2_packed;   /* [L] x packed [128,512]                               */
  const float* b2;         /* [L,128]                                              */
  const float* n2_scale;   /* [L,128]                                              */
  const float* n2_shift;   /* [L,128]                                              */
  const void* wfold_packed; /* 5 (TSP) / 4 (CVRP) x packed [128,128]: Wk, Wv, W_out^T Wl, W_ctx blocks */
  const float* w_fixed;     /* [128,128] project_fixed_context or NULL              */
  void* kvl;                /* planes 0..2 of the folded cache                      */
  int64_t kvl_plane_stride; /* elements between planes                              */
  int64_t kvl_batch_stride; /* elements between instances                           */
  void* ctx_first;          /* [B,N,128] TSP; fp32 unless ctx_dtype says otherwise   */
  void* ctx_cur;            /* [B,N,128]                                            */
  float* q_bias;            /* [B,128] or NULL                                      */
  float* hidden;            /* [B,N,128] final node embeddings, or NULL             */
} rl4co_am_encoder_args;

int rl4co_am_encoder(const rl4co_am_encoder_args* args, void* stream);
int rl4co_am_encoder_max_nodes(void);

/* a12 (training): the INPUT gradient of SkipConnection(MLP 128 -> 512 -> 128, ReLU) in one launch
 *   rl4co/models/nn/mlp.py:52-61 under rl4co/models/nn/ops.py:9-15 (autograd's backward of x + lin2(relu(lin1(x))))
 *   dh[M,512] = (dy . W2) * [h > 0]  (written once: rl4co_wgrad_* reads it for dW1 / db1)      dx[M,128] = dh . W1 + dy
 * dy [M,128], h [M,512] (the forward's hidden activations), dh, dx: 16-bit elements of `dtype` (RL4CO_DT_BF16 / _F16), fp32
 * accumulation on the matrix cores; w2t_packed = W2^T ([512,128]) and w1t_packed = W1^T ([128,512]) in the encoder's
 * fragment order (rl4co_am_encoder_args: "[out/32 tiles][in/16 ksteps][64 lanes][8]"). The 512-wide gradient goes
 * through LDS in four chunks: 1.05 GB of traffic per layer at M = 409 600 where two GEMM launches moved 1.58. */
int rl4co_mlp_input_grad(const void* dy, const void* h, int64_t M, const void* w2t_packed, const void* w1t_packed, int dtype,
                         void* dh, void* dx, void* stream);

/* The TRAINING forward of an instance-norm encoder stack (POMO: zoo/pomo/model.py:59-63; nn/graph/attnnet.py:16-106) in ONE
 * launch — the fused kernel's layer body fed with the init embedding, one workgroup per instance, N <= 128 — writing, per
 * layer, every tensor the backward kernels (rl4co_linear_* input gradients, rl4co_wgrad_*, rl4co_attn_bwd_*,
 * rl4co_skip_inorm_bwd_*) read: the per-op forward it replaces took seven launches and 27 [B N,128]-sized passes per
 * layer. Of `args` only B, N, num_layers, norm (must be 1), act_dtype, the packed weights (W_q UNSCALED: the scores are
 * scaled in the kernel, the saved q is the q the products used), bqkv, b1 and n*_scale / n*_shift (gamma, beta) are read. */
typedef struct rl4co_am_train_save {
  const void* x0; /* [B,N,128] act_dtype: the encoder's input (init embedding)                     */
  void* out;      /* [L,B,N,128] layer outputs (out[l-1] is layer l's input; out[L-1] the result)   */
  void* qkv;      /* [L,B,N,384] q | k | v                                                          */
  void* att;      /* [L,B,N,128] attention output before out_proj                                   */
  void* y1;       /* [L,B,N,128] x + attention branch (pre-norm; the branch's bias cancels in the norm) */
  void* x1;       /* [L,B,N,128] norm1 output                                                       */
  void* h;        /* [L,B,N,512] relu(x1 W1^T + b1)                                                 */
  void* y2;       /* [L,B,N,128] x1 + MLP branch (pre-norm)                                         */
  float* lse;     /* [L,B,8,N] log-sum-exp of the scaled scores, log2 domain (rl4co_attn_fwd's)     */
  float* stats;   /* [L,4,B,128] mean1, rstd1, mean2, rstd2                                         */
} rl4co_am_train_save;
int rl4co_am_encoder_train_fwd(const rl4co_am_encoder_args* args, const rl4co_am_train_save* save, void* stream);

/* The 16-bit encoder + cache fold for graphs of ANY size (csrc/am_encoder.hip: token-tile kernels; BASELINE configs[4],
 * CVRP-500): the fused kernel's layer algebra, GEMM routine and packed weights over tiles of 128 nodes — init embedding,
 * per layer [Q / K / V projection (+ per-head score bounds), rl4co_attn_flash_pre_*, ONE kernel for out-proj + norm + MLP +
 * norm], fold, graph context. Same argument struct and packing as rl4co_am_encoder; norm 0 (batch norm, eval) runs
 * the three-launch layer, norm 1 / 2 (instance / layer: statistics over ALL tiles of an instance) two half-layer kernels
 * that stop before their norm, write the pre-norm sums and per-tile (mean, centred sum of squares), and a norm-apply
 * kernel combining the tiles' pairs (Chan's update) — the workspace then also holds those sums and statistics. B <= 65535.
 * `workspace`: at least rl4co_am_encoder_tokens16_workspace(B, N) bytes of device memory, 16-byte aligned. */
int rl4co_am_encoder_tokens16(const rl4co_am_encoder_args* args, void* workspace, int64_t workspace_bytes, void* stream);
int64_t rl4co_am_encoder_tokens16_workspace(int B, int N);

/* The same fused encoder + cache fold in EXACT fp32 (csrc/am_encoder_f32.hip, v_mfma_f32_16x16x4_f32: f32 operands,
 * f32 accumulate, a k-ordered fmaf chain) — the encoder of the bit-identical configuration (no autocast), replacing the
 * same reference functions as rl4co_am_encoder with arithmetic in ATen's own order where that is knowable: GEMM then
 * + bias, x + branch, norm as x * alpha + beta, softmax as exp(s - max) / sum. Same argument struct, read this way:
 *   act_dtype   RL4CO_DT_F32; cache_dtype any of F32 / BF16 / F16 (planes rounded once on the way out)
 *   w*_packed   fp32, [out/16 tiles][in/16 chunks][64 lanes][4]: lane = 16 g + c, element s = W[16 tile + c][16 chunk + 4 g + s]
 *               (rl4co_amd/encoder.py: pack_weight_f32); the query rows of Wqkv and bqkv carry 1 / sqrt(16) (exact)
 *   bo, b2      ADDED by the kernel (the 16-bit kernel has them folded into the norm's shift)
 *   n*_scale / n*_shift   norm = 0: alpha = weight / sqrt(running_var + eps), beta = bias - running_mean * alpha;
 *               norm = 1: gamma, beta (alpha / beta built per instance from two-pass statistics)
 *   wfold_packed  3 + (ctx_first != NULL) + (ctx_cur != NULL) blocks of [128,128] in that order; with both context
 *               tables NULL the three blocks are the raw rows of project_node_embeddings (the reference's own
 *               association of the decoder, cache.py fold=False) and `hidden` carries the node embeddings. */
int rl4co_am_encoder_f32(const rl4co_am_encoder_args* args, void* stream);

/* The exact-fp32 encoder + cache fold for graphs of ANY size (csrc/am_tokens_f32.hip; BASELINE configs[4], CVRP-500): the
 * same arithmetic as rl4co_am_encoder_f32 (same GEMM routine and summation order) as launches over tiles of 128 nodes —
 * init embedding, per layer [Q/K/V projection, attention with keys / values streamed and an online softmax, out-proj +
 * norm + MLP + norm], fold, graph context. Same argument struct and packing as rl4co_am_encoder_f32; norm 0 .. 2 as for
 * rl4co_am_encoder_tokens16 (instance / layer norm: half-layer kernels + norm-apply over the tiles' combined statistics).
 * B <= 65535. `workspace`: at least rl4co_am_encoder_tokens_f32_workspace(B, N) bytes of device memory, 16-byte aligned,
 * contents irrelevant on entry (the [B N, 128] fp32 activation buffers, the per-head transposed values, the per-tile
 * statistics). */
int rl4co_am_encoder_tokens_f32(const rl4co_am_encoder_args* args, void* workspace, int64_t workspace_bytes, void* stream);
int64_t rl4co_am_encoder_tokens_f32_workspace(int B, int N);

/* The init embeddings alone: out[B,N,128] in the activations' type (act_dtype BF16 / F16: ..._init_embeds16; F32:
 * ..._init_embeds_f32) from the same argument struct — only env, B, N, act_dtype, the feature pointers and the init
 * embedding's weights are read. Replaces `init_embeds` of AttentionModelPolicy.forward(return_init_embeds=True)
 * (rl4co/models/zoo/am/encoder.py:84-103 returns them next to the final embeddings; env_embeddings/init.py). It is the
 * token path's first launch, i.e. the routine the fused kernels run internally. */
int rl4co_am_encoder_init_embeds16(const rl4co_am_encoder_args* args, void* out, void* stream);
int rl4co_am_encoder_init_embeds_f32(const rl4co_am_encoder_args* args, float* out, void* stream);

/* fp32 side of the cache fold from the final node embeddings of ANY encoder (zoo/am/decoder.py:201-228, cache.py):
 * out[i][B,N,128] = h . W_i^T for nblocks <= 5 blocks of [128,128] packed as for rl4co_am_encoder_f32 (the context
 * tables), and q_bias[B,128] = w_fixed . mean_j h[b,j] (w_fixed plain [128,128] fp32; both NULL: skipped). h: [B,N,128]
 * rows of h_dtype (RL4CO_DT_F32 / _BF16 / _F16, widened on load); fp32 MFMA, fp32 outputs. */
int rl4co_am_fold_tables_f32(const void* h, int h_dtype, int B, int N, const float* w_packed, int nblocks, float* const* out,
                             const float* w_fixed, float* q_bias, void* stream);

/* --------------------------------------------------------------------------
 * N1  teacher-forced log-likelihood, backward pass.
 *
 * Replaces the autograd graph the reference builds through its T-step decode loop
 * (rl/reinforce/reinforce.py:99-102 differentiates out["log_likelihood"];
 * models/common/constructive/base.py:226-263; decode_type="evaluate",
 * utils/decoding.py:448-461): given the actions of B trajectories and the upstream
 * gradient g[B,T] of their per-step log-probs, recompute every step from the reset state and
 * return dL/d(folded cache) for L = sum g * log p. Outputs are fp32; d_ctx_first, d_q_step0
 * and d_w_cap are accumulated atomically and must be zero-initialised by the caller, the
 * others are written. One workgroup per instance, its B / B_inst trajectories (s-major rows)
 * replayed in turn. N <= rl4co_am_teacher_max_nodes(). Every RL4CO_ENV_* on both variants (RL4CO_TEACHER_MMA: bf16
 * planes, 16-step blocks on the matrix cores; RL4CO_TEACHER_REPLAY: fp32 arithmetic, step by step).
 * -------------------------------------------------------------------------- */
#define RL4CO_TEACHER_AUTO 0   /* MMA when the planes are bf16 and T fits its step tables, else REPLAY */
#define RL4CO_TEACHER_REPLAY 1 /* am_teacher.hip: fp32 step-by-step replay, planes in registers        */
#define RL4CO_TEACHER_MMA 2    /* am_teacher_mma.hip: 16-step blocks on v_mfma_f32_16x16x16_bf16       */
typedef struct rl4co_am_teacher_args {
  int32_t env;
  int32_t B;            /* trajectories                                             */
  int32_t B_inst;       /* instances                                                */
  int32_t N;
  int32_t T;            /* columns of actions / grad_logp / logp_out                */
  int32_t t0;           /* 1: column 0 is the imposed multistart node (log-prob 0)  */
  int32_t mask_inner;
  int32_t mask_logits;
  float tanh_clipping;
  float temperature;
  int32_t cache_dtype;  /* dtype of the three planes                                */
  int32_t variant;      /* RL4CO_TEACHER_AUTO / _REPLAY / _MMA                      */
  const void* glimpse_key;
  const void* glimpse_val;
  const void* logit_key;
  int64_t kvl_row_stride;
  int64_t kvl_batch_stride;
  const void* ctx_first;         /* element type ctx_dtype (fp32 unless set), strides below */
  const void* ctx_cur;
  const float* q_bias;
  const float* q_step0;
  const float* w_cap;
  const int64_t* actions;        /* [B,T]                                           */
  const float* demand;           /* [B_inst,N-1] CVRP                               */
  const float* vehicle_capacity; /* [B_inst] CVRP                                   */
  const float* locs;             /* [B_inst,N,2] OP, CVRPTW                         */
  const float* max_length;       /* [B_inst,N] OP entry-limit table                 */
  const float* time_windows;     /* [B_inst,N,2] CVRPTW (start, end), fp32          */
  const float* durations;        /* [B_inst,N] CVRPTW service times                 */
  const float* w_time;           /* [128] CVRPTW: W_ctx[:, 129]                     */
  const float* grad_logp;        /* [B,T]                                           */
  float* d_kvl;                  /* [3,B_inst,N,128]                                */
  float* d_ctx_first;            /* [B_inst,N,128] TSP, zero-initialised            */
  float* d_ctx_cur;              /* [B_inst,N,128]                                  */
  float* d_q_bias;               /* [B_inst,128] or NULL                            */
  float* d_q_step0;              /* [128] TSP, zero-initialised                     */
  float* d_w_cap;                /* [128] CVRP, zero-initialised                    */
  float* d_w_time;               /* [128] CVRPTW, zero-initialised                  */
  float* logp_out;               /* [B,T] forward values, or NULL                   */
  int32_t* err;
  /* MMA variant: the three plane gradients as bf16 rows with the caller's strides instead of fp32 d_kvl (which may
   * then be NULL) — element [p][b][n][c] at d_planes_bf16 + p * plane_stride + b * batch_stride + n * row_stride + c.
   * Lets the caller place them next to each other as the columns of ONE [B_inst * N, 5 * 128] gradient matrix, the
   * operand of the fold GEMMs' backward (rl4co_linear / rl4co_wgrad), without an fp32 round trip. */
  void* d_planes_bf16;
  int64_t d_planes_row_stride;
  int64_t d_planes_batch_stride;
  int64_t d_planes_plane_stride;
  /* (r06, MMA variant) context tables in the planes' element type, as in rl4co_am_decode_args: ctx_dtype (0 = fp32),
   * strides in elements (0 = dense). d_ctx_in_planes = 1 (needs d_planes_bf16): the context-table gradients leave the
   * kernel converted to the planes' type as planes 3 (ctx_first, TSP) and 4 (ctx_cur; plane 3 in the depot environments)
   * of the same strided gradient matrix — d_ctx_first / d_ctx_cur remain the kernel's fp32 accumulation scratch
   * (d_ctx_first zero-initialised by the caller) and hold nothing the caller needs afterwards. */
  int32_t ctx_dtype;
  int32_t d_ctx_in_planes;
  int64_t ctx_row_stride;
  int64_t ctx_batch_stride;
} rl4co_am_teacher_args;

int rl4co_am_teacher_backward(const rl4co_am_teacher_args* args, void* stream);
int rl4co_am_teacher_max_nodes(void);
/* The variant rl4co_am_teacher_backward would run for these arguments (1 or 2), -1 if invalid. */
int rl4co_am_teacher_variant(const rl4co_am_teacher_args* args);

/* --------------------------------------------------------------------------
 * Element type of the 16-bit training-encoder / attention entry points (r06: ONE entry point per operation; until r05
 * every one of them existed twice, rl4co_<op>_bf16 and rl4co_<op>_f16). `dtype` = RL4CO_DT_BF16 (torch.autocast(bfloat16))
 * or RL4CO_DT_F16 (torch.autocast(float16): the reference's DEFAULT precision, Lightning's "16-mixed",
 * rl4co/utils/trainer.py:57); any other value is RL4CO_ERR_ARG. Every `const void*` / `void*` activation, weight or
 * gradient operand holds elements of that type, fp32 operands stay fp32; conversions to half round to nearest even and
 * overflow to infinity (what GradScaler's inf check expects). One source per kernel, compiled for both element types
 * (csrc/elem16.h); csrc/entry16.hip dispatches. The comments below say "bf16" where they mean "the 16-bit type".
 * -------------------------------------------------------------------------- */

/* --------------------------------------------------------------------------
 * a11 (training)  init embedding  env_embeddings/init.py:55-68,115-136
 * out[m,:] = W[128,F] . feats[m,:F] + b  (F <= 6: x, y (, demand, ...)); fp32 in, bf16 out [M,128].
 * -------------------------------------------------------------------------- */
int rl4co_init_embed(int dtype, const float* feats, const float* w, const float* b, int64_t M, int F, void* out, void* stream);
/* backward of the above w.r.t. W and b: partial[g, c, 0..F-1] = sum over the rows of block g of dout[m,c] * feats[m,f],
 * partial[g, c, F] = sum of dout[m,c]; dout bf16 [M,128], partial fp32 [blocks,128,F+1] (summed over g by the caller in a
 * fixed order: deterministic). Returns the number of blocks the launch uses through *blocks_out when partial == NULL. */
int rl4co_init_embed_wgrad(int dtype, const void* dout, const float* feats, int64_t M, int F, float* partial, int* blocks_out,
                                void* stream);

/* --------------------------------------------------------------------------
 * a12 (training)  SkipConnection + Normalization("instance")
 *   rl4co/models/nn/ops.py:9-15,30-54 ; nn/graph/attnnet.py:16-54 ; zoo/pomo/model.py:59-63
 * forward : y = x + s ; out = (y - mean_n y) * rsqrt(var_n y + eps) * gamma + beta, statistics per
 *           instance and channel over the N nodes (biased variance). bf16 activations [B,N,128],
 *           fp32 arithmetic; y, mean[B,128], rstd[B,128] are kept for the backward pass.
 * backward: dy (the gradient of BOTH skip inputs) from dout; dgamma / dbeta [B,128]: the per-instance
 *           contributions (every element written; the caller sums over B). N <= rl4co_skip_inorm_max_nodes().
 * -------------------------------------------------------------------------- */
int rl4co_skip_inorm_fwd(int dtype, const void* x, const void* s, const float* gamma, const float* beta, float eps,
                              int B, int N, void* y, void* out, float* mean, float* rstd, void* stream);
int rl4co_skip_inorm_bwd(int dtype, const void* dout, const void* y, const float* gamma, const float* mean,
                              const float* rstd, int B, int N, void* dy, float* dgamma, float* dbeta,
                              void* stream);
int rl4co_skip_inorm_max_nodes(void);
/* rl4co_skip_inorm_fwd / _bwd and rl4co_skip_lnorm_fwd / _bwd serve N <= rl4co_skip_inorm_wide_max_nodes() (r06): beyond
 * rl4co_skip_inorm_max_nodes() the instance's rows are re-read per pass instead of waiting in registers; same arithmetic,
 * same accumulation order. */
int rl4co_skip_inorm_wide_max_nodes(void);

/* --------------------------------------------------------------------------
 * a12 (training)  SkipConnection + Normalization("layer")
 *   rl4co/models/nn/ops.py:9-15,48-51
 * forward : y = x + s ; out = (y - mean y) / sqrt(var y + eps) with ONE mean and ONE unbiased variance (divisor M - 1)
 *           over all M = N x 128 values of the instance, no affine. 16-bit activations [B,N,128], fp32 arithmetic;
 *           y and stats[B,2] = (mean, 1 / sqrt(var + eps)) are kept for the backward pass.
 * backward: dy (the gradient of BOTH skip inputs) = r (dout - sum(dout) / M - xh sum(dout xh) / (M - 1)), xh = (y - mean) r.
 *           N <= rl4co_skip_inorm_max_nodes().
 * -------------------------------------------------------------------------- */
int rl4co_skip_lnorm_fwd(int dtype, const void* x, const void* s, float eps, int B, int N, void* y, void* out, float* stats,
                              void* stream);
int rl4co_skip_lnorm_bwd(int dtype, const void* dout, const void* y, const float* stats, int B, int N, void* dy, void* stream);

/* --------------------------------------------------------------------------
 * a12 (training)  SkipConnection + Normalization("batch") — the AttentionModel default
 *   rl4co/models/nn/ops.py:9-15,30-54 ; zoo/am/policy.py:50-122
 * BatchNorm1d over the M = B x nodes rows of bf16 [M,128] activations, batch statistics:
 *   stats : y = x + s (s may be NULL: y is not written, statistics of x);
 *           sums[0][c] += sum_m y, sums[1][c] += sum_m y^2      (fp32 [2,128], zero-initialised)
 *   apply : out = (y - mean) * rstd * gamma + beta               (mean / rstd from the host)
 *   bwd   : sums[0][c] += sum dout, sums[1][c] += sum dout * xh  (zero-initialised), then
 *           dy = rstd gamma (dout - sums[0]/M - xh sums[1]/M); sums[1] = dgamma, sums[0] = dbeta.
 * -------------------------------------------------------------------------- */
int rl4co_skip_bnorm_stats(int dtype, const void* x, const void* s, int64_t M, void* y, float* sums, void* stream);
int rl4co_bnorm_apply(int dtype, const void* y, const float* mean, const float* rstd, const float* gamma, const float* beta,
                           int64_t M, void* out, void* stream);
/* out = bn_eval(x + skip) in one pass (SkipConnection + Normalization("batch") in eval mode, nn/ops.py:9-54): the
 * token-parallel inference encoder for graphs beyond rl4co_am_encoder_max_nodes(); x, skip, out bf16 [M,128]. */
int rl4co_skip_bnorm_eval(int dtype, const void* x, const void* skip, const float* mean, const float* rstd, const float* gamma,
                               const float* beta, int64_t M, void* out, void* stream);
int rl4co_bnorm_bwd(int dtype, const void* dout, const void* y, const float* mean, const float* rstd, const float* gamma,
                         int64_t M, float* sums, void* dy, void* stream);

/* --------------------------------------------------------------------------
 * a12 (training)  nn.Linear over the token rows: Wqkv, out_proj, MLP
 *   rl4co/models/nn/attention.py:64-134 ; nn/mlp.py:52-61
 * out[M,N] = epilogue(A[M,K] . W[N,K]^T + bias[N]); bf16 A, W, out, fp32 bias and accumulate.
 * epilogue: relu != 0 -> max(.,0); mask != NULL -> (mask[m,n] > 0 ? . : 0) (ReLU backward, bf16 mask);
 * residual != NULL -> . + residual[m,n] (bf16 [M,N]: the skip connection's gradient joins the branch's input
 * gradient here, nn/ops.py:9-15 backward, instead of in one more pass over both). mask and residual exclude each other.
 * With W = weight^T (contiguous) it is the input gradient dX = dY . weight.
 * N and K multiples of 128; bias, mask and residual may be NULL.
 * -------------------------------------------------------------------------- */
int rl4co_linear(int dtype, const void* a, const void* w, const float* bias, const void* mask, const void* residual, int64_t M,
                      int N, int K, int relu, void* out, void* stream);
/* Weight gradient of the same layers: partial[c][N,K] = dY[rows of chunk c]^T . X[rows of chunk c]
 * (bf16 dY [M,N], X [M,K]; fp32 partial [chunks,N,K], every element written); dW = sum over c.
 * partial_bias [chunks,N] (or NULL) receives the column sums of dY per chunk: db = sum over c.
 * The rows are split into `chunks` equal ranges (a multiple of 32 rows each).
 * chunk_stride: elements between consecutive chunks of BOTH partial arrays; 0 = packed (N*K and N). With
 * partial_bias = partial + N*K and chunk_stride = N*K + N one reduction over the chunk axis yields dW and db. */
int rl4co_wgrad(int dtype, const void* dy, const void* x, int64_t M, int N, int K, int chunks, float* partial,
                     float* partial_bias, int64_t chunk_stride, void* stream);

/* --------------------------------------------------------------------------
 * a12 (training)  encoder self-attention on the packed projection output
 *   rl4co/models/nn/attention.py:110-134 (rearrange to heads + scaled_dot_product_attention)
 * qkv [B,N,384] bf16 = per node (q | k | v), each 8 heads x 16 dims. forward: out [B,N,128] bf16
 * (heads concatenated) and lse [B,8,N] fp32 (log2-domain log-sum-exp of the scaled scores);
 * backward: dqkv [B,N,384] bf16 from dout [B,N,128] and the forward's own out (the softmax
 * backward's row term sum_keys P dP is taken as sum_d dout out). rl4co_attn_bwd: N <= rl4co_attn_max_nodes() (one
 * workgroup holds an instance's keys); rl4co_attn_fwd: N <= rl4co_attn_wide_max_nodes() (beyond rl4co_attn_max_nodes()
 * the keys stream through LDS with an online softmax, r06).
 * rl4co_attn_bwd_wide (r06): the backward for any N <= rl4co_attn_wide_max_nodes(): one workgroup per (instance, half of
 * the heads, chunk of 128 keys); d k / d v of a chunk are complete in its workgroup, the chunks' shares of d q go through
 * `dq_partial` — a caller-provided fp32 workspace [ceil(N / 128), B, N, 128] — and are summed in chunk order.
 * -------------------------------------------------------------------------- */
int rl4co_attn_fwd(int dtype, const void* qkv, int B, int N, void* out, float* lse, void* stream);
int rl4co_attn_bwd(int dtype, const void* qkv, const void* out, const void* dout, const float* lse, int B, int N,
                        void* dqkv, void* stream);
int rl4co_attn_bwd_wide(int dtype, const void* qkv, const void* out, const void* dout, const float* lse, int B, int N,
                        void* dqkv, float* dq_partial, void* stream);
int rl4co_attn_max_nodes(void);
int rl4co_attn_wide_max_nodes(void);

/* --------------------------------------------------------------------------
 * (r06) The decoder's masked glimpse attention over ALL steps of given trajectories at once, forward and backward —
 * the inner multi-head attention of PointerAttention (rl4co/models/nn/attention.py:255-296 with the action mask,
 * models/zoo/am/decoder.py:150-190) as the dense re-evaluation of known actions uses it (`evaluate` decoding with
 * autograd: utils/decoding.py:448-461; rl/ppo/ppo.py:128-170): T step queries per trajectory against the N node keys of
 * its instance. 16-bit operands (dtype argument), fp32 softmax; heads = softmax_keys(q k^T / 4, masked) v per head.
 *   q    [B, T] rows of 128 (8 heads x 16), `q_stride` elements apart
 *   kv   [B_inst, N] rows of k 128 | v 128, `kv_stride` elements apart; trajectory b reads instance b % B_inst
 *   mask [B, T, mask_words] words of 32 keys, bit j = node j feasible at that step (rl4co_env_replay's mask_bits);
 *        mask_words % 4 == 0; NULL = every key. Every query needs at least one feasible key.
 *   forward : out [B, T, 128], lse [B, 8, T] (log2 domain)
 *   backward: dq [B, T, 128]; dkv [B_inst, N, dk 128 | dv 128] summed over steps and starts; `dq_partial` = fp32
 *             workspace [rl4co_cross_attn_chunks(N), B, T, 128]
 * -------------------------------------------------------------------------- */
typedef struct rl4co_cross_attn_args {
  int32_t B, B_inst, T, N;
  const void* q;
  int64_t q_stride;
  const void* kv;
  int64_t kv_stride;
  const uint32_t* mask;
  int32_t mask_words;
  int32_t reserved0;
  void* out;
  float* lse;
  const void* dout; /* backward only from here */
  void* dq;
  void* dkv;
  float* dq_partial;
} rl4co_cross_attn_args;
int rl4co_cross_attn_fwd(int dtype, const rl4co_cross_attn_args* args, void* stream);
int rl4co_cross_attn_bwd(int dtype, const rl4co_cross_attn_args* args, void* stream);
int rl4co_cross_attn_chunks(int N);

/* --------------------------------------------------------------------------
 * (r06) log p(a_t | s_t) of GIVEN actions from the pointer's raw logits (glimpse . logit_key, before the 1 / sqrt(128)),
 * every step of every trajectory as one row — the tail of the dense re-evaluation:
 *   u = raw / sqrt(128); z = tanh_clipping * tanh(u) (0: z = u); z = -inf where infeasible; z /= temperature;
 *   logp = log_softmax(z)[action]        rl4co/models/nn/attention.py:291-293, utils/decoding.py:169-188, :381
 * raw [rows, N] fp32; mask_bits [rows, mask_words] (bit j = node j feasible; NULL = all, i.e. mask_logits = False);
 * actions [rows]; forward -> logp [rows], lse [rows]; backward: d_raw [rows, N] from grad_logp [rows] and the saved lse.
 * err: RL4CO_EBIT_NAN_LOGIT / RL4CO_EBIT_INFEASIBLE (an action out of range), may be NULL.
 * -------------------------------------------------------------------------- */
int rl4co_logit_logp_fwd(const float* raw, const uint32_t* mask_bits, int mask_words, const int64_t* actions, int64_t rows, int N,
                         float tanh_clipping, float temperature, float* logp, float* lse, int32_t* err, void* stream);
int rl4co_logit_logp_bwd(const float* raw, const uint32_t* mask_bits, int mask_words, const int64_t* actions, const float* lse,
                         const float* grad_logp, int64_t rows, int N, float tanh_clipping, float temperature, float* d_raw,
                         void* stream);

/* --------------------------------------------------------------------------
 * a12 (inference, large graphs)  MultiHeadAttention.forward   rl4co/models/nn/attention.py:110-134
 * out[b, i, 16 h ..] = softmax_j(q_h[i] . k_h[j] / 4) v_h[j] on the packed projection output qkv [B,N,384]
 * (q | k | v, 8 heads x 16), bf16 -> out [B,N,128] bf16, any N: keys / values stream through LDS in blocks of
 * 64 nodes with a running (max, sum, output) per query — the N x N score matrix is never materialised
 * (csrc/am_attn_flash.hip). Serves the encoder beyond rl4co_am_encoder_max_nodes() (BASELINE configs[4]).
 * -------------------------------------------------------------------------- */
int rl4co_attn_flash(int dtype, const void* qkv, int B, int N, void* out, void* stream);
/* The same with q already in the exp2 domain (1/4 log2 e folded into the packed W_q: rl4co_am_encoder_tokens16) and,
 * bound != NULL, per (instance, head) the maxima over the nodes of |q_h|^2 and |k_h|^2 ([B,8,2] fp32): heads whose
 * product stays below 48^2 take the max-free softmax path (bf16 only; every |score| is then below 48 by Cauchy-Schwarz). */
int rl4co_attn_flash_pre(int dtype, const void* qkv, const float* bound, int B, int N, void* out, void* stream);

/* --------------------------------------------------------------------------
 * a19  select_start_nodes        rl4co/utils/ops.py:128-161
 * out[s*B + b] = s % num_loc (+1 for depot environments), s-major.
 * -------------------------------------------------------------------------- */
int rl4co_select_start_nodes(int64_t* out, int B, int num_starts, int num_loc, int has_depot,
                             void* stream);

/* --------------------------------------------------------------------------
 * N3  state augmentation                      rl4co/data/transforms.py:16-87, 105-151
 * Both kernels read the B instances ONCE and write the aug-major layout [A*B, N, 2] (row a*B + b) that the
 * multistart rollout consumes — what batchify (utils/ops.py:10-30) followed by the transform produces in the reference.
 *
 * dihedral8: the 8 symmetries of the unit square in the reference's order (transforms.py:27-37):
 *   (x,y) (1-x,y) (x,1-y) (1-x,1-y) (y,x) (1-y,x) (y,1-x) (1-y,1-x); xy [B,N,2] f32 -> out [8*B,N,2]. Bit-exact.
 * symmetric: rotation by phi_r about (offset, offset) and an axis swap where phi_r > 2 pi (transforms.py:49-69), one
 *   angle per OUTPUT row r. The caller passes cos(phi), sin(phi) [A*B] f32 and the swap flags [A*B] u8 (the angles are
 *   host-side RNG state: transforms.py:81 draws them from torch's global generator); the kernel does the fp32
 *   arithmetic in the reference's order, x' = cos*x - sin*y, y' = sin*x + cos*y (no fused multiply-add).
 * -------------------------------------------------------------------------- */
int rl4co_augment_dihedral8_f32(const float* xy, int B, int N, float* out, void* stream);
int rl4co_augment_symmetric_f32(const float* xy, const float* cos_phi, const float* sin_phi, const uint8_t* swap_axes,
                                int B, int A, int N, float offset, float* out, void* stream);

/* --------------------------------------------------------------------------
 * N3  POMO evaluation epilogue                rl4co/models/zoo/pomo/model.py:112-140
 *                                             (unbatchify / gather_by_index: rl4co/utils/ops.py:33-66)
 * reward [S*A*B] f32 and actions [S*A*B, T] i64 of a multistart rollout over an augmented batch, rows ordered
 * (s * A + a) * B + b. One launch computes
 *   max_reward[b,a]      = max_s reward            best_start[b,a] = its first arg-max (torch.max's tie rule)
 *   max_aug_reward[b]    = max_a max_reward[b,a]   best_aug[b]     = its first arg-max
 *   best_ms_actions[b,a] = actions of (best_start[b,a], a, b)          [B,A,T]
 *   best_aug_actions[b]  = actions of (best_start[b,a*], a* = best_aug[b], b)   [B,T]
 * Any output pointer may be NULL; actions may be NULL when no action output is asked for. A = 1 and / or S = 1 are
 * the degenerate cases of the same reduction.
 * -------------------------------------------------------------------------- */
int rl4co_pomo_best(const float* reward, const int64_t* actions, int A, int S, int B, int T, float* max_reward,
                    int64_t* best_start, float* max_aug_reward, int64_t* best_aug, int64_t* best_ms_actions,
                    int64_t* best_aug_actions, void* stream);

/* --------------------------------------------------------------------------
 * N2 / a10  instance generation on the device
 *        rl4co/envs/common/utils.py:34-62 (get_sampler -> Uniform), tsp/generator.py:49-58,
 *        cvrp/generator.py:114-140
 * out[i] = low + (high - low) * u_i, u_i = k_i / 2^24 from Philox4x32-10 keyed by `seed` (counter = element block,
 * stream_id) — U(low, high) like the reference's sampler, drawn straight into HBM in one launch (the reference draws on
 * the host and uploads). mode 1 = CVRP demands: (trunc(v) + 1) / capacity, i.e. `(U(min-1, max-1).int() + 1) / cap`.
 * A different generator than torch's: the CPU stream of the reference is reproduced by the host mirror
 * (envs.*Generator(device="cpu")), not by this kernel; this one is pinned to oracle_uniform_f32 bit for bit.
 * -------------------------------------------------------------------------- */
int rl4co_uniform_f32(float* out, int64_t n, float low, float high, uint64_t seed, uint32_t stream_id, int mode,
                      float capacity, void* stream);

/* --------------------------------------------------------------------------
 * Micro-benchmark helper: HBM read stream (float4 grid-stride sum), used by
 * bench.py to report the achievable-copy ceiling next to the 8 TB/s spec.
 * -------------------------------------------------------------------------- */
int rl4co_hbm_read_probe(const void* src, int64_t bytes, float* sink, void* stream);

/* --------------------------------------------------------------------------
 * Deterministic-math probe: y[i] = f(x[i]) on the device, f = 0 exp / 1 log / 2 tanh of
 * csrc/rl4co_math.h (the fp32 polynomials behind torch.tanh / log_softmax / exp in
 * utils/decoding.py:169-188). tests/test_math.py checks device == host bit for bit and
 * both against float64 libm.
 * -------------------------------------------------------------------------- */
int rl4co_math_probe_f32(int fn, const float* x, int64_t n, float* y, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RL4CO_AMD_H */

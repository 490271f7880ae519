/* scg_cbf_nn.h — the CBF-QP safety filter with a learned correction of the Lie derivative (safety_filters/cbf/cbf_nn.py of the
 * reference) as HIP.  The C ABI of libscg_cbfnn_<spechash>_<H>_<act>.so (safe_control_gym_amd/_cbf_nn.py builds it from
 * safe_control_gym_amd/csrc/scg_cbf_nn.hip).  The library also exports everything of scg_hip.h and of scg_cbf.h.  Float32 CartPole
 * only; any other build exports the entry points and refuses with SCG_ERR_INVALID, as scg_cbf.h's do.
 *
 * With (a_nn, b_nn) = mlp(X) the reference's barrier row (cbf_nn.py:104-124) is
 *      -slope h(X) - LfV(X, u) - (a_nn u + b_nn) <= s
 * and with LfV = a + b u this is scg_cbf.h's problem with
 *      k' = slope h + a + b_nn          b' = b + a_nn
 * so its minimiser is the same closed form (soft and hard), with the same u0 clip and the same `feasible` rule.  The residual network
 * is MLP(4 -> 256 -> 256 -> 2), relu on both hidden layers, no output activation; its input is the state (the first four observation
 * entries); output 0 is a_nn, output 1 is b_nn.  The forward pass is csrc/scg_mlp_rows.h's (exact float32 on the matrix cores, layer 2
 * in registers): the arithmetic per row does not depend on where the row sits in a launch, and ONE device function serves both entry
 * points, so a filter row of scg_rollout_cbf_nn equals scg_cbf_nn_certify of the same state, action and weights bit for bit.
 */
#ifndef SCG_CBF_NN_H
#define SCG_CBF_NN_H

#include <stdint.h>

#include "scg_cbf.h"
#include "scg_learn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SCG_CBF_NN_HIDDEN 256

/* The residual network: a flat float32 parameter vector on the device and the word offsets of its six tensors (PyTorch layouts:
 * W1 [256][4], b1 [256], W2 [256][256], b2 [256], W3 [2][256], b3 [2]).  Read at every launch: nothing of it is cached. */
typedef struct scg_cbf_residual {
    const float* d_params;
    scg_mlp_layout mlp;
    int32_t hidden;             /* must be SCG_CBF_NN_HIDDEN */
} scg_cbf_residual;

/* Certify n (state, action) rows; n is independent of the env count, n = 0 is a no-op.  Workgroups of 512 threads serve 8 column tiles
 * of 32 rows each.
 *   env          the handle (its device is used; no env state is read or written)
 *   d_state      float32 [n][4], 16-byte aligned
 *   d_action     float32 [n]      uncertified PHYSICAL action
 *   d_certified  float32 [n]      u*
 *   d_slack      float32 [n]      s* (may be NULL)
 *   d_feasible   uint8   [n]      1 = feasible
 *   d_ab         float32 [n][2]   (a_nn, b_nn) of every row (may be NULL) */
int scg_cbf_nn_certify(scg_env* env, const scg_cbf_params* params, const scg_cbf_residual* residual, const float* d_state,
                       const float* d_action, float* d_certified, float* d_slack, uint8_t* d_feasible, float* d_ab, int n, void* stream);

/* How the action of a control step is formed and what the env step receives. */
typedef struct scg_cbf_nn_mode {
    int32_t deterministic;      /* 1: the actor's mean; 0: mean + exp(logstd) N(0,1) from Philox channel 5 (scg_rollout_policy's draw) */
    int32_t uniform;            /* 1: the uncertified action is action_space.sample() = act_low + (act_high - act_low) U[0, 1) from
                                   Philox channel 4 (scg_rollout_random's word); the actor is not read, out.logp receives 0 */
    float act_low, act_high;    /* the env's action space (read when uniform) */
    float blend;                /* < 0: apply u* where feasible, else the policy's own action (evaluation, scg_rollout_cbf's rule);
                                   0 <= blend <= 1: applied = (1 - blend) a + blend u*_env regardless of feasibility (cbf_nn.py:349),
                                   a the controller's unclipped action, u*_env = u* / act_scale when the action space is normalised */
} scg_cbf_nn_mode;

/* K control steps with PPO's Gaussian actor, the residual network AND the filter in the loop, as ONE launch.
 *   actor          per-tensor pointers (scg_actor_ptrs) of the compiled shape; ignored when mode.uniform
 *   out            as for scg_rollout_policy; out.act / out.logp keep the POLICY's action and its log-probability
 *   d_filter_rows  float32 [k][N][4] = (u0, u*, s*, feasible as 0.0 / 1.0), 16-byte aligned
 *   d_applied      float32 [k][N]    the action given to the env step
 *   d_ab           float32 [k][N][2] (a_nn, b_nn)
 * Results do not depend on the launch geometry. */
int scg_rollout_cbf_nn(scg_env* env, const scg_actor_ptrs* actor, const scg_cbf_params* params, const scg_cbf_residual* residual,
                       const scg_cbf_nn_mode* mode, int k_steps, const scg_policy_rollout* out, float* d_filter_rows, float* d_applied,
                       float* d_ab, void* stream);

/* Compiled shape: the actor's hidden width and activation, the residual's hidden width (256), observation and action dims (all 0 when
 * the library is not a float32 CartPole one: the entry points then return SCG_ERR_INVALID). */
int scg_cbf_nn_shape(int32_t* hidden, int32_t* activation, int32_t* residual_hidden, int32_t* obs_dim, int32_t* act_dim);

/* Dynamic LDS bytes of the rollout kernel with `tiles` (1 | 8) column tiles per workgroup: the row-split image plus the actor image;
 * 0 when not served. */
int scg_cbf_nn_lds(int tiles, int32_t* lds_bytes);

#ifdef __cplusplus
}
#endif

#endif /* SCG_CBF_NN_H */

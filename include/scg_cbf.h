/* scg_cbf.h — the CBF-QP safety filter (safety_filters/cbf/cbf.py of the reference) as HIP: a batched certify, and the policy
 * rollout with the filter between the actor and the env step, as ONE launch.  The C ABI of libscg_cbfroll_<spechash>_<H>_<act>.so
 * (safe_control_gym_amd/_cbf.py builds it from safe_control_gym_amd/csrc/scg_cbf.hip).  The library also exports everything of
 * scg_hip.h.  CartPole only, as the reference.
 *
 * The reference's QP has two unknowns (the input u and one slack s), one barrier row that is affine in u, and box bounds on u; its
 * minimiser is unique and has a closed form.  With X = (x, x_dot, theta, theta_dot), limits L_i, the prior model's f(X, F):
 *   h      = 1 - sum (X_i / L_i)^2              grad h_i = -2 X_i / L_i^2
 *   a      = grad h . f(X, 0)                   b = grad h . (f(X, 1) - f(X, 0))        (LfV(X, u) = a + b u)
 *   k      = slope h + a                        u0 = clip(u, lo, hi)                    r(u) = -k - b u
 *   soft:  u* = u0 if r(u0) <= 0, else clip((u0 - 2 w b k) / (1 + 2 w b^2), lo, hi);  s* = max(0, r(u*));  feasible = s* <= tolerance
 *   hard:  u* = u0 if r(u0) <= 0, else -k / b when that lies in [lo, hi] on the side of u0 the row allows (feasible), else u0 with
 *          feasible = 0;  s* = 0
 * Plain float32, IEEE division, sinf / cosf of the device library; ONE device function serves both entry points, so a row of
 * scg_rollout_cbf equals scg_cbf_certify of the same state and action bit for bit.
 */
#ifndef SCG_CBF_H
#define SCG_CBF_H

#include <stdint.h>

#include "scg_actor_rollout.h"
#include "scg_adversarial.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The filter's settings, by value: nothing of it is compiled in, one library serves every filter config of its task. */
typedef struct scg_cbf_params {
    float L[4];                 /* state limits min(|upper_i|, |lower_i|) of the single state constraint */
    float m, M, l, g;           /* prior model: pole mass, cart mass, effective pole length, gravity */
    float slope;                /* the barrier's linear class-K function */
    float slack_weight;         /* w */
    float slack_tolerance;
    float lo, hi;               /* physical_action_bounds */
    int32_t soft;               /* soft_constrained */
} scg_cbf_params;

/* Certify n (state, action) rows, one thread per row; n is independent of the env count.
 *   env          the handle (its device is used; no env state is read or written)
 *   d_state      float32 [n][4]
 *   d_action     float32 [n]   uncertified PHYSICAL action (clipped to [lo, hi] first, as certify_action does)
 *   d_certified  float32 [n]   u*
 *   d_slack      float32 [n]   s* (may be NULL)
 *   d_feasible   uint8   [n]   1 = feasible */
int scg_cbf_certify(scg_env* env, const scg_cbf_params* params, const float* d_state, const float* d_action, float* d_certified,
                    float* d_slack, uint8_t* d_feasible, int n, void* stream);

/* K control steps with the actor AND the filter in the loop: scg_rollout_policy's kernel with, between the action and the env step,
 *   u_phys = act_scale a (normalized_rl_action_space) or a;  (u0, u*, s*, feasible) = certify(obs[0:4], u_phys);
 *   applied = u* / act_scale (or u*) where feasible, else the policy's own action a      (base_experiment.py:183-184)
 *   actor          per-tensor pointers (scg_actor_ptrs: W1, b1, W2, b2, W3, b3, logstd)
 *   deterministic  1: a = the actor's mean; 0: mean + exp(logstd) N(0,1) from Philox channel 5, exactly scg_rollout_policy's draw
 *   out            as for scg_rollout_policy; out.act / out.logp keep the POLICY's action and its log-probability
 *   d_filter_rows  float32 [k][N][4] = (u0, u*, s*, feasible as 0.0 / 1.0), 16-byte aligned
 *   d_applied      float32 [k][N]    the (normalised) action given to the env step */
int scg_rollout_cbf(scg_env* env, const scg_actor_ptrs* actor, const scg_cbf_params* params, int deterministic, int k_steps,
                    const scg_policy_rollout* out, float* d_filter_rows, float* d_applied, void* stream);

/* The same with the deterministic SAC / DDPG actor of scg_actor_rollout.h in front of the filter (scg_rollout_actor's kernel with the
 * certify step between the head and the env step): scg_rollout_cbf's row layout and applied-action rule; out.act keeps the actor's
 * action, out.logp is not written.  Served by libscg_cbfroll_<spechash>_<H>_<act>_<sac|ddpg>.so (float32 CartPole); every other
 * library returns SCG_ERR_INVALID, as does an actor whose hidden / activation / kind differ from the compiled ones. */
int scg_rollout_cbf_actor(scg_env* env, const scg_actor* actor, const scg_cbf_params* params, int k_steps, const scg_policy_rollout* out,
                          float* d_filter_rows, float* d_applied, void* stream);

/* Compiled shape: actor hidden width and activation, observation and action dims (all 0 when the library's task is not CartPole:
 * both entry points then return SCG_ERR_INVALID). */
int scg_cbf_shape(int32_t* hidden, int32_t* activation, int32_t* obs_dim, int32_t* act_dim);

#ifdef __cplusplus
}
#endif

#endif /* SCG_CBF_H */

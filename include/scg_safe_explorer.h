/* scg_safe_explorer.h — the Safe-Explorer PPO collector (actor, safety layer, projection, sampling, env step) as ONE launch: the
 * C ABI of libscg_saferoll_<spechash>_<H>_<act>_<Hc>.so (safe_control_gym_amd/_safe_explorer.py builds it from
 * safe_control_gym_amd/csrc/scg_safe_explorer.hip).  The library also exports everything of scg_hip.h.
 *
 * Per control step and env (safe_explorer.SafeExplorerPPO._collect_body / evaluate, step for step):
 *   actor       obs -> H -> H -> A mean (tanh / relu / leaky_relu, the library's shape) on the matrix cores, as scg_rollout_policy;
 *   safety      the C constraint models g_i = W2_i relu(W1_i obs + b1_i) + b2_i (one hidden layer of Hc, safety_layer.SafetyLayer),
 *               C = the spec's state-constraint rows, on the matrix cores (exact float32);
 *   projection  numer_i = g_i.a + c_i + slack_i, denom_i = g_i.g_i + 1e-8, mult_i = relu(numer_i / denom_i) (IEEE division),
 *               i* = the FIRST maximum (torch.max), a_safe = a - mult_i* g_i*;
 *   action      a_safe + exp(logstd) N(0,1) from Philox channel 5 exactly as scg_rollout_policy draws it (or a_safe), and its
 *               log-probability under Normal(a_safe, exp(logstd));
 *   env step    as scg_step, auto-reset included;
 *   next c      the state-constraint rows (EnvOps::constraints(..., only_state)) of the post-step state, or of the fresh state
 *               where the env was reset: what SafeExplorerPPO._next_c feeds the next policy step.
 *
 * Packed safety layer (float32, one contiguous 16-byte aligned device buffer; _safe_explorer.pack_safety_layer writes it).
 * Hp = Hc rounded up to a multiple of 32, NT = Hp / 32, Q = 4 * ceil(obs_dim / 8), row(q, h) = (q & 3) + 8 (q >> 2) + 4 h.
 * Constraint i occupies the block [i * STRIDE, (i + 1) * STRIDE), STRIDE = NT*Q*64 + Hp*(1 + A) + 4 words:
 *   W1f [NT][Q][64]   word (t, q, lane) = W1_i[32 t + (lane & 31)][row(q, lane >> 5)]   (the MFMA A operand of lane `lane`)
 *   b1  [Hp]
 *   W2  [A][Hp]       nn.Linear layout
 *   b2  [4]           A values, zero padded
 * Every padded entry (hidden unit >= Hc, input row >= obs_dim) is zero: relu(0) times a zero column adds nothing.
 *
 * Placement: the launcher keeps the packed layer in LDS next to the actor image when both (and, for 16-byte observation rows,
 * the obs transpose scratch) fit in 160 KiB, and otherwise reads it from memory (shared by every wave: L2-resident).  Both
 * placements run the same MFMA sequence: results are bit-identical.  SCG_SAFE_WEIGHTS=lds|global forces one (measurement); a
 * forced LDS placement that does not fit returns SCG_ERR_INVALID and never launches.  Results do not depend on SCG_ROLLOUT_EPW /
 * SCG_ROLLOUT_WPW, and no output column depends on another env's input.
 */
#ifndef SCG_SAFE_EXPLORER_H
#define SCG_SAFE_EXPLORER_H

#include <stdint.h>

#include "scg_adversarial.h"

#ifdef __cplusplus
extern "C" {
#endif

/* K control steps of Safe-Explorer PPO's collector (or, deterministic = 1, its evaluation loop) in one launch.
 *   actor       the policy's actor, per-tensor pointers (scg_actor_ptrs: W1, b1, W2, b2, W3, b3, logstd)
 *   d_safety    the packed safety layer (layout above; scg_safe_explorer_shape reports its size in words)
 *   d_slack     float32 [C] per-constraint slack
 *   out         as for scg_rollout_policy (obs [k + 1][N][obs_dim], act, logp, reward, done, flags, terminal obs, episode totals)
 *   d_c_rows    float32 [k][N][C]: row t = the constraint values step t's policy saw (row 0 = the carry passed in)
 *   d_c_carry   float32 [N][C], in/out: the constraint values of the current state; on return those after the last step */
int scg_rollout_safe(scg_env* env, const scg_actor_ptrs* actor, const float* d_safety, const float* d_slack, int deterministic,
                     int k_steps, const scg_policy_rollout* out, float* d_c_rows, float* d_c_carry, void* stream);

/* Compiled shape: constraints C, safety hidden width Hc, actor hidden width and activation, action and observation dims, and the
 * packed layer's size in float words. */
int scg_safe_explorer_shape(int32_t* n_constraints, int32_t* hidden_c, int32_t* hidden, int32_t* activation, int32_t* act_dim,
                            int32_t* obs_dim, int32_t* packed_words);

/* What the launcher does when asked for `wpw` waves per workgroup (SCG_SAFE_WEIGHTS honoured): LDS bytes per workgroup, the waves
 * per workgroup it runs (0: no placement fits) and whether the safety layer sits in LDS (1) or is read from memory (0). */
int scg_safe_explorer_lds(int wpw, int32_t* lds_bytes, int32_t* wpw_used, int32_t* weights_in_lds);

#ifdef __cplusplus
}
#endif

#endif /* SCG_SAFE_EXPLORER_H */

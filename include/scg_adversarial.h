/* scg_adversarial.h — the robust-adversarial collector (RARL / RAP) as ONE launch: the C ABI of
 * libscg_advroll_<spechash>_<H>_<act>_<n>.so (safe_control_gym_amd/_adversarial.py builds it from
 * safe_control_gym_amd/csrc/scg_adversarial.hip).  The library also exports everything of scg_hip.h, scg_rollout_policy
 * included, so one handle serves the training collection and protagonist-only evaluation.
 *
 * Per control step and env (rarl.py:349-428, rap.py:349-470 — both policies act on every step):
 *   protagonist  exactly scg_rollout_policy's step: actor MLP, action = mean + exp(logstd) N(0,1) from Philox channel 5
 *                (or the mean), its log-probability;
 *   adversary    the same obs -> H -> H -> adv_dim MLP (same hidden width and activation: the reference builds both
 *                PPOAgents from one config) on the same observation; action = mean + exp(logstd) N(0,1) from Philox
 *                CHANNEL 6 (rng_tag(6, 0, 0), one 4-word draw per env and step, Box-Muller as on channel 5), or the mean;
 *                with a population (RAP, n <= 4) env e uses adversary d_adv_index[e];
 *   control      set_adversary_control (benchmark_env.py:216-228) on the raw adversary action: clamp to [-1, 1], times the
 *                float32 adversary_disturbance_scale, plus the float32 adversary_disturbance_offset — two rounded
 *                operations, no fused multiply-add, so that the result equals the step-by-step path bit for bit — into
 *                the env's adversary channel (action or dynamics), then the same control step as scg_step.
 * Channels 0-5 keep their layout (scg_rng.h, SCG_RNG_LAYOUT_VERSION 2): channel 6 is new and only this kernel draws it.
 *
 * Stored: everything scg_rollout_policy stores (protagonist rows, terminal observations, episode statistics) plus the RAW
 * sampled adversary action (before the clamp) and its log-probability.  Results do not depend on the launch geometry
 * (SCG_ROLLOUT_EPW / SCG_ROLLOUT_WPW as for scg_rollout_policy) nor, with a population, on which other adversaries share a
 * wave: every MFMA output column depends only on its own input column.
 *
 * LDS: per workgroup one protagonist and n adversary weight images plus, for 16-byte observation rows, the obs transpose
 * scratch (waves x 64 x obs_dim floats).  Over 160 KiB the launcher drops to 4 waves per workgroup, then stores the obs rows
 * one by one without the scratch; a shape that still does not fit returns SCG_ERR_INVALID with a message and never launches.
 */
#ifndef SCG_ADVERSARIAL_H
#define SCG_ADVERSARIAL_H

#include <stdint.h>

#include "scg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One adversary's actor, as per-tensor pointers in nn.Linear layout: W1 [H][obs_dim], b1 [H], W2 [H][H], b2 [H],
 * W3 [adv_dim][H], b3 [adv_dim], logstd [adv_dim].  (A population's members need not share a flat parameter vector.) */
typedef struct {
    const float *W1, *b1, *W2, *b2, *W3, *b3, *logstd;
} scg_actor_ptrs;

/* K control steps with the protagonist and the adversary (or adversaries) in the loop.
 *   protagonist        as for scg_rollout_policy (flat vector + offsets; hidden / activation must equal the library's)
 *   adversaries        [n_adversaries] actors; n_adversaries must equal the library's compiled population size
 *   d_adv_index        int32 [N] adversary of each env (values clamped to [0, n)), or NULL when n_adversaries == 1
 *   deterministic_adversary  1: adversary action = its mean
 *   out                the protagonist's rows, as for scg_rollout_policy
 *   d_adv_act          float32 [k][N][adv_dim] raw sampled adversary actions
 *   d_adv_logp         float32 [k][N] their log-probabilities
 * Captured in a HIP graph the call issues no host-side setup (the kernel attributes are set on the first call per device). */
int scg_rollout_adversarial(scg_env* env, const scg_policy* protagonist, const scg_actor_ptrs* adversaries, int n_adversaries,
                            const int32_t* d_adv_index, int deterministic_adversary, int k_steps, const scg_policy_rollout* out,
                            void* d_adv_act, void* d_adv_logp, void* stream);

/* Compiled shape of this library: population size, hidden width, activation, adversary dim; LDS bytes and waves per workgroup
 * the launcher uses when asked for `wpw` (0 if the shape does not fit). */
int scg_adversarial_shape(int32_t* n_adversaries, int32_t* hidden, int32_t* activation, int32_t* adv_dim);
int scg_adversarial_lds(int wpw, int32_t* lds_bytes, int32_t* wpw_used);

#ifdef __cplusplus
}
#endif

#endif /* SCG_ADVERSARIAL_H */

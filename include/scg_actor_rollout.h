/* scg_actor_rollout.h — the fused policy-in-the-loop rollout for the two off-policy actors (SAC, DDPG): K control steps of every env in
 * ONE launch with the DETERMINISTIC actor inside the env kernel, as scg_rollout_policy (scg_hip.h) does for PPO's Gaussian actor.
 *
 *   SCG_ACTOR_SAC   (sac_utils.py:185-222)   h1 = act(W1 x + b1);  h2 = W2 h1 + b2 (no activation: upstream's MLP applies none after its
 *                                            last layer);  u = W3 h2 + b3 with W3 / b3 the first act_dim rows of the stacked
 *                                            [2 act_dim][H] head (mean rows first, scg_sac.h)
 *   SCG_ACTOR_DDPG  (ddpg_utils.py:127-175)  h1 = act(W1 x + b1);  h2 = act(W2 h1 + b2);  u = W3 h2 + b3
 *   both                                     a = low + 0.5 (tanhf(u) + 1)(high - low)      (a column with low == high gives low exactly)
 *
 * The C ABI of libscg_spec_<hash>_pol<H>_<act>_<sac|ddpg>.so (safe_control_gym_amd/csrc/scg_actor_rollout.hip, built with
 * -DSCG_POLICY_H= -DSCG_POLICY_ACT= -DSCG_POLICY_KIND=, float32), which also exports everything of scg_hip.h.  The CBF libraries
 * (scg_cbf.h) export it too; one built without a kind returns SCG_ERR_INVALID (scg_last_error says why) and launches nothing.  The
 * simulator's own libraries (libscg_hip.so, libscg_spec_<hash>[_pol<H>_<act>].so) are unchanged and do not carry the symbols.
 * Sampled actions (SAC) and exploration noise (DDPG) are not part of it: scg_sac_sample / scg_ddpg_noisy_act keep those, and SAC's
 * sampled TRAINING collection is an entry point of its own in the same libraries (scg_rollout_sac_collect, scg_actor_collect.h).
 *
 * Hidden widths: 32 / 64 / 96 / 128 in the libraries above, and 256 in libscg_spec_<hash>_wide256_<act>_<sac|ddpg>.so
 * (safe_control_gym_amd/csrc/scg_actor_rollout_wide.hip, built with -DSCG_ACTOR_WIDE_H=256 -DSCG_ACTOR_WIDE_ACT= -DSCG_ACTOR_WIDE_KIND= and
 * without -DSCG_POLICY_H=) and libscg_cbfroll_<hash>_256_<act>_<sac|ddpg>.so (csrc/scg_cbf_wide.hip): the same entry points, structs and
 * argument checks, scg_actor_rollout_shape reports 256.  There the second layer's weights live in registers, split by output rows over
 * the 8 waves of a workgroup (csrc/scg_mlp_rows.h); a workgroup serves 1 or 8 tiles of 32 envs (chosen by num_envs,
 * SCG_ROLLOUT_WIDE_TILES=1|8 overrides it for measurements; results do not depend on it; SCG_ROLLOUT_EPW / SCG_ROLLOUT_WPW are not
 * read).  A 256 library exports scg_rollout_policy like every library and refuses there: PPO's rollout has no width 256.
 */
#ifndef SCG_ACTOR_ROLLOUT_H
#define SCG_ACTOR_ROLLOUT_H

#include <stdint.h>

#include "scg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { SCG_ACTOR_SAC = 1, SCG_ACTOR_DDPG = 2 };

typedef struct {
    const float* d_params;            /* flat float32 vector */
    int32_t W1, b1, W2, b2, W3, b3;   /* offsets (floats), nn.Linear layout; SAC: W3 / b3 = the stacked head (mean rows first); DDPG: the output layer */
    int32_t hidden, activation, kind; /* must equal the library's compiled shape (activation: 0 tanh | 1 relu | 2 leaky_relu) */
    float act_low[4], act_high[4];    /* action-space bounds, the first act_dim entries are read */
} scg_actor;

/* K control steps with the actor in the loop.  `out` as for scg_rollout_policy: d_obs [k + 1][N][obs_dim], d_act [k][N][act_dim] (the
 * rescaled action given to the env step), d_reward / d_done / d_flags [k][N], d_terminal_obs, d_ep_stats, d_episode_acc and
 * max_episodes with the same meaning; d_logp is NOT written and may be NULL.  Results do not depend on the launch geometry
 * (SCG_ROLLOUT_EPW / SCG_ROLLOUT_WPW, as for scg_rollout_policy).  Capturable in a HIP graph after the first call on the device. */
int scg_rollout_actor(scg_env* env, const scg_actor* actor, int k_steps, const scg_policy_rollout* out, void* stream);

/* Compiled actor shape (all zero when the library carries no actor rollout). */
int scg_actor_rollout_shape(int32_t* hidden, int32_t* activation, int32_t* kind);

#ifdef __cplusplus
}
#endif

#endif /* SCG_ACTOR_ROLLOUT_H */

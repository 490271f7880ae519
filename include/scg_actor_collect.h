/* scg_actor_collect.h — SAC's TRAINING collection as one launch: K control steps of every env with the SAMPLED actor (or the warm-up's
 * uniform action) inside the env kernel, each transition written straight into the replay ring (SACBuffer.push with the time-limit
 * fix-up of sac.py:287-305, i.e. scg_sac_push's semantics, include/scg_sac.h).  What SAC.train_step's loop (sac.py:273-305) enqueues
 * between two updates, in place of K x (scg_sac_sample, scg_step, scg_sac_push).
 *
 * Per step t and env i, in order:
 *   action, c->uniform == 1   a_j = low_j + (high_j - low_j) u01(w_j), w the Philox block of env-stream channel 4, item 0, block 0 at the
 *                             env's (global id, episode, step in episode) BEFORE the step
 *   action, c->uniform == 0   the actor forward of scg_rollout_actor (include/scg_actor_rollout.h) with ALL 2 act_dim rows of the stacked
 *                             head (mean rows first, then log_std rows);  u = mu + exp(clamp(log_std, -20, 2)) eps;
 *                             a = low + 0.5 (tanhf(u) + 1)(high - low);  eps = the Box-Muller draws of env-stream channel 5, item 0,
 *                             block 0 at the same address (what scg_rollout_policy draws its action noise from)
 *                             (either mode: a column with low == high gives low exactly)
 *   env step                  unchanged, with auto-reset, episode statistics and the episode accumulator as in scg_rollout_actor
 *   ring row                  (pos0 + t N + i) mod capacity, pos0 = *d_pos at entry  <-  (obs_t, a, reward, next observation = the TERMINAL
 *                             observation where the episode was truncated by the time limit (done and flags bit 0) else obs_{t+1},
 *                             mask = 1 where truncated else 1 - done)
 * After the K steps d_cur_obs [N][obs_dim] holds the observation after the last step, and a second, one-thread launch advances *d_pos,
 * *d_size_f and *d_size_i32 by K N (the size saturates at capacity).  Every counter is a device scalar: the call is capturable in a HIP
 * graph after the first call on the device.  The draws are addressed by the env's own counters, which scg_get_counters reads and
 * scg_set_counters restores: a checkpoint needs nothing else to continue the noise.
 *
 * Exported by the libraries that export scg_rollout_actor; served by libscg_spec_<hash>_pol<H>_<act>_sac.so (H = 32 / 64 / 96 / 128,
 * float32; safe_control_gym_amd/csrc/scg_actor_collect.h).  Every other one — built without a kind, with kind ddpg (its exploration
 * noise is ONE process continued across the envs in env order: a dependency across the batch inside every step), at hidden width 256,
 * or a CBF library — returns SCG_ERR_INVALID.  So do k_steps < 1, k_steps N > capacity, an actor whose shape is not the compiled
 * one, a NULL required pointer, a trace group given in part, row arrays that are not 16-byte aligned, and a ring whose observation
 * array exceeds 4 GiB (rows are addressed with 32-bit byte offsets).  scg_last_error says why; nothing is launched.
 * Results do not depend on the launch geometry (SCG_ROLLOUT_EPW / SCG_ROLLOUT_WPW, as for scg_rollout_policy).
 */
#ifndef SCG_ACTOR_COLLECT_H
#define SCG_ACTOR_COLLECT_H

#include <stdint.h>

#include "scg_actor_rollout.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    /* ---- the replay ring: scg_sac_ring's fields (include/scg_sac.h) without the noise counter; arrays of `capacity` rows */
    float* d_ring_obs;              /* [capacity][obs_dim] */
    float* d_ring_act;              /* [capacity][act_dim] */
    float* d_ring_rew;              /* [capacity] */
    float* d_ring_next_obs;         /* [capacity][obs_dim] */
    float* d_ring_mask;             /* [capacity] */
    int32_t capacity;
    int64_t* d_pos;                 /* write position, read at entry and advanced by K N */
    float* d_size_f;                /* rows valid, as float (nullable) */
    int32_t* d_size_i32;            /* rows valid (nullable; what scg_sac_args.d_ring_size reads) */
    /* ---- the collector's persistent current-observation batch: written, never read (the env holds its own state) */
    float* d_cur_obs;               /* [N][obs_dim] */
    int32_t uniform;                /* 1: the warm-up's uniform actions (the actor's parameters are not read), 0: samples of the policy */
    /* ---- episode statistics, as in scg_policy_rollout (each nullable) */
    float* d_ep_stats;              /* [N][4] running episodes: read at entry, written at exit */
    float* d_episode_acc;           /* [N][8] finished episodes' sums: read at entry, written at exit */
    int32_t max_episodes;           /* <= 0: no limit */
    /* ---- trace of the launch (tests): ALL of them or none, meanings as in scg_policy_rollout */
    float* d_obs;                   /* [k + 1][N][obs_dim] */
    float* d_act;                   /* [k][N][act_dim] */
    float* d_reward;                /* [k][N] */
    uint8_t* d_done;                /* [k][N] */
    uint8_t* d_flags;               /* [k][N] */
    float* d_terminal_obs;          /* [k][N][obs_dim], rows written where done */
} scg_sac_collect;

int scg_rollout_sac_collect(scg_env* env, const scg_actor* actor, int k_steps, const scg_sac_collect* c, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SCG_ACTOR_COLLECT_H */

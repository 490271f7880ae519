/* scg_ddpg.h — C ABI of libscg_ddpg_<obs>_<hidden>_<act_dim>_<activation>.so: ONE gradient step of the reference's
 * DDPGAgent.update (safe_control_gym/controllers/ddpg/ddpg_utils.py:16-121) on MI355X, fused, and the DDPG collector's
 * device-side pieces (the deterministic actor plus the reference's exploration noise, the replay-ring push).
 *
 * What one scg_ddpg_update call enqueues (8 kernels; no host synchronisation, exact float32, matrix products on
 * v_mfma_f32_32x32x2_f32, no atomics, every reduction in a fixed order: the step is bitwise reproducible):
 *   actor fwd  batch rows ~ U[0, *d_ring_size) of the replay ring; a = actor(obs), its activation tiles kept
 *   q d/da     q(obs, a) and d q / d a                                                 (compute_policy_loss)
 *   actor grad policy_loss = -mean q(obs, actor(obs)) back through the actor
 *   reduce     sum of the partials + Adam (actor), Polyak averaging of the actor's target copy
 *   actor fwd  a' = actor(next_obs) with the UPDATED, online actor (upstream quirk: not the target actor)
 *   q fwd      target critic at (next_obs, a'); beside it the online critic at (obs, act)
 *   q grad     critic_loss = mean((q - y)^2), y = rew + gamma mask q_targ(next_obs, a')    (compute_q_loss)
 *   reduce     sum + Adam (critic), Polyak averaging of the critic's target copy, step counters and loss statistics
 * soft_update runs over ALL parameters (the target actor is never read, but it is averaged, as upstream does).
 * Networks (ddpg_utils.py:126-175 over neural_networks.py:18-54): actor obs -> H (act) -> H (act) -> act_dim, then tanh and
 * the rescaling to [low, high]; q: (obs, act) -> H (act) -> H (act) -> 1.
 *
 * Conventions as in scg_learn.h / scg_sac.h: plain C types, d_* = caller-owned DEVICE pointers, kernels go to the caller's
 * hipStream_t, 0 = ok / negative = error + scg_ddpg_last_error().  Parameters, gradients and Adam moments are FLAT float32
 * vectors [actor | q] in torch's nn.Linear layout ([out][in] row-major) at the offsets of the two layouts.
 */
#ifndef SCG_DDPG_H
#define SCG_DDPG_H

#include <stddef.h>
#include <stdint.h>

#include "scg_learn.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    /* ---- parameters: flat vector of n_params floats, [actor | q] */
    float* d_params;
    float* d_target;                /* target copy (ac_targ), same order */
    float* d_grad;                  /* [n_params] gradients of the current step */
    float* d_m; float* d_v;         /* [n_params] Adam moments */
    float* d_steps;                 /* [2] Adam step counts: actor, critic */
    scg_mlp_layout actor, q;        /* offsets inside d_params */
    int32_t n_actor;                /* actor parameters are [0, n_actor), the critic's [n_actor, n_params) */
    int32_t n_params;
    /* ---- replay ring: row-major device arrays of `capacity` rows */
    const float* d_obs;             /* [capacity][obs_dim] */
    const float* d_act;             /* [capacity][act_dim] */
    const float* d_rew;             /* [capacity] */
    const float* d_next_obs;        /* [capacity][obs_dim] */
    const float* d_mask;            /* [capacity] */
    const int32_t* d_ring_size;     /* device scalar: rows currently valid (sampling happens on the device) */
    /* ---- hyper-parameters (ddpg.yaml) */
    int32_t batch;                  /* train_batch_size, a multiple of 32 */
    float gamma, tau;
    float actor_lr, critic_lr;
    float act_low[4], act_high[4];
    /* ---- randomness: Philox4x32-10 keyed by `seed`, counter = (*d_counter, row, 0); d_counter is advanced by the call */
    uint64_t seed;
    uint32_t* d_counter;            /* device scalar */
    /* ---- tests / replay: when non-NULL, the ring rows of the minibatch */
    const int32_t* d_idx_in;        /* [batch] */
    /* ---- scratch + outputs */
    void* d_workspace;              /* scg_ddpg_workspace_bytes(batch) bytes */
    float* d_stats;                 /* [2] policy_loss, critic_loss of this step */
    float* d_stats_acc;             /* [2] nullable: running sums over calls */
} scg_ddpg_args;

void scg_ddpg_shape(int32_t* obs_dim, int32_t* hidden, int32_t* act_dim, int32_t* activation);
size_t scg_ddpg_workspace_bytes(int batch);
/* One-time kernel attributes (dynamic LDS > 64 KB); call before capturing into a HIP graph (not a stream operation). */
int scg_ddpg_prepare(void);
int scg_ddpg_update(const scg_ddpg_args* args, void* stream);
/* n_steps whole gradient steps, bit-identical to n_steps scg_ddpg_update calls, in 7 n_steps + 1 launches: step k's target-action
 * launch also draws step k + 1's minibatch rows and evaluates the actor at them (the critic's step in between touches neither the
 * actor nor the ring).  Capturable in a HIP graph. */
int scg_ddpg_update_n(const scg_ddpg_args* args, int n_steps, void* stream);

/* ---- exploration noise (math_and_models/random_processes.py + schedule.py), ONE process of size act_dim shared by the env batch:
 * DDPG.train_step samples it once per env, in env order, on every vector step (ddpg.py:283-286).
 *   OU:        x_k = x_{k-1} + theta (0 - x_{k-1}) dt + std_k sqrt(dt) eps_k    (carry x_{-1} = *d_x_prev)
 *   Gaussian:  x_k = std_k eps_k
 *   std_k = LinearSchedule(start, end, steps) after c_k = *d_calls + k calls: start + c_k inc, bounded by end
 * The recurrence is evaluated in float64 (the reference's NumPy dtype).  Every value is a device scalar, so a vector step is
 * capturable: scg_ddpg_noisy_act leaves the batch's last x in d_x_next and the number of sample() calls it made in *d_pending;
 * scg_ddpg_push's bookkeeping launch (or scg_ddpg_noise_commit) moves them into *d_x_prev / *d_calls. */
enum { SCG_DDPG_NOISE_NONE = 0, SCG_DDPG_NOISE_OU = 1, SCG_DDPG_NOISE_GAUSSIAN = 2 };
typedef struct {
    int32_t kind;
    double theta, dt;               /* OU: 0.15, 1e-2 */
    double std_start, std_end, std_inc;     /* LinearSchedule: inc = (end - start) / steps (0: constant) */
    double* d_x_prev;               /* [4] the process's carry (OU) */
    double* d_x_next;               /* [4] staging: x of the last env of the latest noisy launch */
    int64_t* d_calls;               /* sample() calls so far (the schedule's position) */
    int32_t* d_pending;             /* calls made by the latest noisy launch, not yet committed */
} scg_ddpg_noise;

/* One launch per vector step: d_act_out[m][act_dim] = f32(actor(obs) + noise) — the deterministic actor (ac.act) on the m current
 * observations plus the process continued across the m envs in env order.  eps ~ N(0, 1) from Philox4x32-10 keyed by `seed`, counter
 * (*d_counter, env, 3), or the caller's d_eps_in[m][act_dim] (tests).  uniform != 0: the warm-up's action_space.sample(), a ~ U[low, high)
 * (no noise call: the process does not advance).  noise NULL or kind NONE: the deterministic actor alone.
 * The scan: envs are split into chunks of 256, one per workgroup; a workgroup derives its carry-in from the draws of the envs in front of
 * its chunk (terms whose weight (1 - theta dt)^k has fallen below 2^-50 are left out — far below the float32 output's resolution). */
int scg_ddpg_noisy_act(const float* d_params, const scg_mlp_layout* actor, const float* act_low, const float* act_high, const float* d_obs,
                       int m, uint64_t seed, const uint32_t* d_counter, int uniform, const scg_ddpg_noise* noise, const float* d_eps_in,
                       float* d_act_out, void* stream);
/* The deterministic actor on a batch: low + 0.5 (tanh(actor(obs)) + 1)(high - low). */
int scg_ddpg_act(const float* d_params, const scg_mlp_layout* actor, const float* act_low, const float* act_high, const float* d_obs,
                 int m, float* d_act_out, void* stream);
/* *d_x_prev <- *d_x_next (OU), *d_calls += *d_pending, *d_pending <- 0: one one-thread launch. */
int scg_ddpg_noise_commit(const scg_ddpg_noise* noise, void* stream);

/* One vectorised env step into the replay ring: the semantics of scg_sac_push (time-limit fix-up: a truncated transition stores the
 * TERMINAL observation with mask 1), then the bookkeeping launch advances *d_pos / *d_size_* / *d_counter and commits the noise (noise
 * nullable).  Exported here rather than borrowed from the SAC library: the noise commit rides in that bookkeeping launch, so a DDPG
 * vector step stays at the SAC collector's launch count and the collector needs one library only. */
typedef struct {
    float* d_obs; float* d_act; float* d_rew; float* d_next_obs; float* d_mask;
    int32_t capacity;
    int64_t* d_pos;
    float* d_size_f;                /* nullable */
    int32_t* d_size_i32;            /* nullable */
    uint32_t* d_counter;            /* nullable: the noise's Philox counter word, incremented */
} scg_ddpg_ring;
int scg_ddpg_push(const scg_ddpg_ring* ring, const scg_ddpg_noise* noise, float* d_cur_obs, const float* d_act, const float* d_reward,
                  const float* d_next_obs, const float* d_terminal_obs, const uint8_t* d_done, const uint8_t* d_flags, int n, void* stream);

const char* scg_ddpg_last_error(void);
const char* scg_ddpg_source_hash_tag(void);

#ifdef __cplusplus
}
#endif
#endif /* SCG_DDPG_H */

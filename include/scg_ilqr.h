/* scg_ilqr.h — the LQR / iLQR baseline controllers (controllers/lqr/{lqr,ilqr}.py of the reference) as HIP: the closed-loop rollout
 * with an affine time-varying state feedback in the loop, and iLQR's backward pass, each ONE launch for N envs (one thread = one env).
 * The C ABI of libscg_ilqr_<spechash>.so (safe_control_gym_amd/_ilqr.py builds it from safe_control_gym_amd/csrc/scg_ilqr.hip).  The
 * library also exports everything of scg_hip.h.  Element type T below is the env's dtype (float32 or float64).
 *
 * The env must observe its state (obs_dim = state_dim: cost = quadratic) and take PHYSICAL actions (normalized_rl_action_space off).
 */
#ifndef SCG_ILQR_H
#define SCG_ILQR_H

#include <stdint.h>

#include "scg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* scg_rollout_feedback: per env i and step t < k_steps, with s = min(t, schedule_len - 1):
 *     u = K[s] obs + ff[s];  x[t] = obs, u[t] = u;  env step;  cost -= reward;  stop at the first done (n_steps = t + 1)
 * A stopped env takes no further step and writes nothing more: rows t >= n_steps of every [k]-stacked output keep their contents.
 *   per_env = 0   d_gains T [schedule_len][nu][nx],    d_ff T [schedule_len][nu]      one schedule for every env
 *   per_env = 1   d_gains T [schedule_len][nu][nx][N], d_ff T [schedule_len][nu][N]   (what scg_ilqr_backward writes)
 * Outputs (all SoA, env index last):
 *   d_x T [k_steps][nx][N], d_u T [k_steps][nu][N], d_final_obs T [nx][N] (the observation after the last step taken: the terminal
 *   observation), d_stats T [4][N] = (cost = -sum reward, steps taken, constraint violations, sum of the per-step mse),
 *   d_n_steps int32 [N], d_final_flags uint8 [N] (the last step's SCG_FLAG_* bits, out-of-bounds included);
 *   optional (NULL to skip) d_reward T [k_steps][N], d_done / d_flags uint8 [k_steps][N]. */
typedef struct scg_feedback_rollout {
    const void* d_gains;
    const void* d_ff;
    int32_t schedule_len;
    int32_t per_env;
    void* d_x;
    void* d_u;
    void* d_final_obs;
    void* d_stats;
    int32_t* d_n_steps;
    uint8_t* d_final_flags;
    void* d_reward;
    uint8_t* d_done;
    uint8_t* d_flags;
} scg_feedback_rollout;

int scg_rollout_feedback(scg_env* env, int k_steps, const scg_feedback_rollout* io, void* stream);

/* scg_ilqr_backward: iLQR.update_policy (ilqr.py:185-278) for every env whose mask byte is non-zero (d_mask NULL: all).  With the
 * quadratic cost l = (x - Xr)' Q (x - Xr) / 2 + (u - Ur)' R (u - Ur) / 2 (Q, R diagonal, Ur = u_eq) and the PRIOR model f (inertial
 * parameters `par`, in the order of scg_get_params), starting from Sv = Q (x[n] - Xr_last), Sm = Q at n = n_steps[i], for k = n-1 .. 0:
 *     A_c, B_c = central differences of f at (x[k], u[k]) with step eps;  Ad = I + A_c dt, Bd = B_c dt
 *     g = R (u - Ur) + Bd' Sv;  G = Bd' Sm Ad;  H = R + Bd' Sm Bd
 *     sum(H) not finite: unstable[i] = 1, this step's gains stay as they are, the recursion goes on unchanged
 *     else H = (H + H') / 2, eigenvalues below 0 clipped to 0, + lamb[i], inverted through the eigenvectors (closed form, nu <= 2)
 *          duff = -Hinv g;  K = -Hinv G;  gains[k] = K;  ff[k] = u[k] + duff - K x[k]
 *          Sm = Q + Ad' Sm Ad + K' H K + K' G + G' K;  Sv = Q (x - Xr) + Ad' Sv + K' H duff + K' g + G' duff
 * Xr = the env's goal row (stabilisation) or row k of its reference (tracking; the last row for the terminal term).
 *   d_x T [k_steps + 1][nx][N] (row n_steps[i] holds env i's final observation), d_u T [k_steps][nu][N], d_n_steps int32 [N] (1..k_steps),
 *   d_lamb T [N]; d_gains T [k_steps][nu][nx][N] and d_ff T [k_steps][nu][N] are updated in place; d_unstable uint8 [N] is SET to 1
 *   where H was not finite and otherwise left alone.
 * Serves CartPole, Quadrotor 1D and 2D; Quadrotor 3D returns SCG_ERR_INVALID (nu = 4 needs another eigen-solve and register budget):
 * scg_ilqr_backward_wide (scg_ilqr_wide.h) serves it. */
typedef struct scg_ilqr_model {
    double q[12];               /* diagonal of Q (nx used) */
    double r[4];                /* diagonal of R (nu used) */
    double u_eq[4];
    double par[4];              /* the prior model's inertial parameters */
    double arm;                 /* quadrotors: the prior model's moment arm L / sqrt(2) (the env's engine may integrate another one) */
    double dt;                  /* discretisation step (the control period) */
    double eps;                 /* central-difference step */
} scg_ilqr_model;

int scg_ilqr_backward(scg_env* env, const scg_ilqr_model* model, int k_steps, const void* d_x, const void* d_u, const int32_t* d_n_steps,
                      const void* d_lamb, const uint8_t* d_mask, void* d_gains, void* d_ff, uint8_t* d_unstable, void* stream);

/* Device-side snapshot / restore of every env's raw simulator state, so that an iLQR iteration restarts its envs without host work:
 * scg_ilqr_snapshot copies the env's raw state (T [ns][N], ns = the raw state arrays of scg_get_state) to d_state;
 * scg_ilqr_restart copies d_state back and zeroes every env's control-step counter.  Both are ordered on `stream`. */
int scg_ilqr_snapshot(scg_env* env, void* d_state, void* stream);
int scg_ilqr_restart(scg_env* env, const void* d_state, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SCG_ILQR_H */

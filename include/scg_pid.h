/* scg_pid.h — the PID baseline controller (controllers/pid/pid.py of the reference: the DSL cascade position / attitude PID of the
 * Crazyflie) inside the fused closed-loop rollout: ONE launch runs k_steps control steps of N envs, one thread = one env, with the
 * controller's nine values of state carried in registers from step to step.  Part of the C ABI of libscg_ilqr_<spechash>.so
 * (safe_control_gym_amd/csrc/scg_pid.h, included by scg_ilqr.hip): one library per task config serves lqr, ilqr and pid.
 * Element type T below is the env's dtype (float32 or float64).
 *
 * The env must observe its state (obs_dim = state_dim: cost = quadratic) and take PHYSICAL actions (normalized_rl_action_space off).
 * Quadrotor 2D and 3D are served; CartPole and Quadrotor 1D return SCG_ERR_INVALID.
 */
#ifndef SCG_PID_H
#define SCG_PID_H

#include <stdint.h>

#include "scg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The controller's constants (pid.py:63-76, 250), by value. */
typedef struct scg_pid_config {
    double kf;                  /* thrust coefficient */
    double gravity;             /* g x the PRIOR model's mass: the feed-forward force */
    double pwm2rpm_scale;
    double pwm2rpm_const;
    double min_pwm;
    double max_pwm;
    double dt;                  /* the control period */
} scg_pid_config;

/* scg_rollout_pid: per env i and step t < k_steps (pid.py:83-243), with c = the env's control-step counter before the step:
 *     pos, vel, rpy   from the observation: Quadrotor 2D (x, 0, z), (x_dot, 0, z_dot), (0, theta, 0); 3D obs[0,2,4], obs[1,3,5], obs[6,7,8]
 *     q = quaternion(rpy);  R = matrix(q);  cur_rpy = euler(q)     PyBullet's conversions, gimbal branches included: the law is the
 *                                                                  reference's for EVERY observation, |pitch| >= pi/2 included
 *     target          tracking: row min(c, last) of the env's reference, positions and velocities; stabilisation: the goal, zero velocity
 *     int_pos = clip(int_pos + pos_e dt, +-2), z then to +-0.15
 *     F = P_for pos_e + I_for int_pos + D_for vel_e + (0, 0, gravity)
 *     thrust = (sqrt(max(0, F . R[:,2]) / (4 kf)) - pwm2rpm_const) / pwm2rpm_scale
 *     Rt = (x, y, z) with z = F / |F|, y = z x (1, 0, 0) normalised, x = y x z                   (target yaw 0)
 *     rot_e = vee(Rt' R - R' Rt);  rate_e = -(cur_rpy - last_rpy) / dt;  last_rpy = cur_rpy
 *     int_rpy = clip(int_rpy - rot_e dt, +-1500), roll / pitch then to +-1
 *     tau = clip(-P_tor rot_e + D_tor rate_e + I_tor int_rpy, +-3200)
 *     pwm = clip(thrust + MIXER tau, [min_pwm, max_pwm]);  a = kf (pwm2rpm_scale pwm + pwm2rpm_const)^2
 *     u = a (3D) or (a0 + a3, a1 + a2) (2D);  x[t] = obs, u[t] = u;  env step (the env clips the action);  stop at the first done
 * The reference passes Rt through scipy's as_euler / from_euler; Rt is used as it is here (equal up to rounding).
 *
 *   d_gains      T [18] (per_env = 0) or T [18][N] (per_env = 1): P_for, I_for, D_for, P_tor, I_tor, D_tor, three values each.  ONE code
 *                path: element k lives at k * gs + gi with (gs, gi) = (N, i) per env and (1, 0) shared.
 *   d_pid_state  T [9][N]: int_pos, last_rpy, int_rpy.  Read at entry, written at exit (the state after the last step taken), so that a
 *                rollout continues across launches.  NULL: start from zeros, discard at exit.
 * Outputs as scg_rollout_feedback's (include/scg_ilqr.h): d_x T [k_steps][nx][N], d_u T [k_steps][nu][N], d_final_obs T [nx][N],
 * d_stats T [4][N], d_n_steps int32 [N], d_final_flags uint8 [N]; optional d_reward T [k_steps][N], d_done / d_flags uint8 [k_steps][N].
 * A stopped env takes no further step and writes nothing more. */
typedef struct scg_pid_rollout {
    const void* d_gains;
    int32_t per_env;
    int32_t reserved;
    void* d_pid_state;
    scg_pid_config config;
    void* d_x;
    void* d_u;
    void* d_final_obs;
    void* d_stats;
    int32_t* d_n_steps;
    uint8_t* d_final_flags;
    void* d_reward;
    uint8_t* d_done;
    uint8_t* d_flags;
} scg_pid_rollout;

int scg_rollout_pid(scg_env* env, int k_steps, const scg_pid_rollout* io, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* SCG_PID_H */

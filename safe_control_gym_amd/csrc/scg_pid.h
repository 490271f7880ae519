// scg_pid.h — the PID baseline controller (include/scg_pid.h) in the fused closed-loop rollout.  Included by scg_ilqr.hip after its own
// kernels: rollout_pid_kernel is rollout_feedback_kernel's loop (state in registers, the same EnvOps::step, the same outputs) with the
// cascade PID law in place of u = K x + ff, and the law's nine values of state (position integral, last rpy, attitude integral) carried
// in registers across the steps.  One thread = one env; no LDS, no cross-lane traffic.
#ifndef SCG_CSRC_PID_H
#define SCG_CSRC_PID_H

#include "../../include/scg_pid.h"

namespace scg {

template <typename T>
struct PidArgs {
    const T* gains; T* state;
    int32_t per_env, k_steps;
    T kf, gravity, scale, cnst, min_pwm, max_pwm, dt;
    T* x; T* u; T* final_obs; T* stats;
    int32_t* n_steps; uint8_t* final_flags;
    T* reward; uint8_t* done; uint8_t* flags;
};

// pid.py:153-243 for one env.  g = the 18 gains; ip / lr / ir = the controller state, updated in place; act = the four motor thrusts.
// The pose goes Euler -> quaternion -> (matrix, Euler) with PyBullet's conversions, as the reference's does, in library precision
// (the attitude loop's derivative term multiplies the angles' rounding by D_tor / dt ~ 1e6: the float reset path's 3e-7 rad shortcuts
// are not used here).
template <typename T>
__device__ __forceinline__ void pid_law(const T* pos, const T* vel, const T* ang, const T* tp, const T* tv, const T* g, const PidArgs<T>& A,
                                        T* ip, T* lr, T* ir, T* act) {
    T q[4], R[3][3], rpy[3];
    {
        T sr, cr, sp, cp, sy, cy;
        m_sincos((T)0.5 * ang[0], &sr, &cr);
        m_sincos((T)0.5 * ang[1], &sp, &cp);
        m_sincos((T)0.5 * ang[2], &sy, &cy);
        q[0] = sr * cp * cy - cr * sp * sy;
        q[1] = cr * sp * cy + sr * cp * sy;
        q[2] = cr * cp * sy - sr * sp * cy;
        q[3] = cr * cp * cy + sr * sp * sy;
    }
    quat_to_mat(q, R);
    {
        const T x = q[0], y = q[1], z = q[2], w = q[3];
        const T sarg = (T)-2 * (x * z - w * y);
        if (sarg <= (T)-0.99999) {
            rpy[0] = (T)0; rpy[1] = -Const<T>::HALF_PI; rpy[2] = (T)2 * m_atan2(x, -y);
        } else if (sarg >= (T)0.99999) {
            rpy[0] = (T)0; rpy[1] = Const<T>::HALF_PI; rpy[2] = (T)2 * m_atan2(-x, y);
        } else {
            rpy[0] = m_atan2((T)2 * (y * z + w * x), w * w - x * x - y * y + z * z);
            rpy[1] = m_asin(sarg);
            rpy[2] = m_atan2((T)2 * (x * y + w * z), w * w + x * x - y * y - z * z);
        }
    }
    // ---- position loop
    T F[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const T pe = tp[k] - pos[k], ve = tv[k] - vel[k];
        T s = m_clamp(ip[k] + pe * A.dt, (T)-2, (T)2);
        if (k == 2) s = m_clamp(s, (T)-0.15, (T)0.15);
        ip[k] = s;
        F[k] = g[k] * pe + g[3 + k] * s + g[6 + k] * ve + (k == 2 ? A.gravity : (T)0);
    }
    const T along = F[0] * R[0][2] + F[1] * R[1][2] + F[2] * R[2][2];
    const T thrust = (m_sqrt(m_max(along, (T)0) / ((T)4 * A.kf)) - A.cnst) / A.scale;
    // ---- target rotation: z along F, y = z x (1, 0, 0) normalised, x = y x z
    const T fn = m_sqrt(F[0] * F[0] + F[1] * F[1] + F[2] * F[2]);
    const T zx = F[0] / fn, zy = F[1] / fn, zz = F[2] / fn;
    const T yn = m_sqrt(zz * zz + zy * zy);
    const T yy = zz / yn, yz = -zy / yn;                       // y = (0, yy, yz)
    const T xx = yy * zz - yz * zy, xy = yz * zx, xz = -yy * zx;
    // ---- attitude loop: rot_e = vee(Rt' R - R' Rt)
    T re[3];
    re[0] = (zx * R[0][1] + zy * R[1][1] + zz * R[2][1]) - (yy * R[1][2] + yz * R[2][2]);
    re[1] = (xx * R[0][2] + xy * R[1][2] + xz * R[2][2]) - (zx * R[0][0] + zy * R[1][0] + zz * R[2][0]);
    re[2] = (yy * R[1][0] + yz * R[2][0]) - (xx * R[0][1] + xy * R[1][1] + xz * R[2][1]);
    T tau[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const T rate_e = -(rpy[k] - lr[k]) / A.dt;
        lr[k] = rpy[k];
        T s = m_clamp(ir[k] - re[k] * A.dt, (T)-1500, (T)1500);
        if (k < 2) s = m_clamp(s, (T)-1, (T)1);
        ir[k] = s;
        tau[k] = m_clamp(-g[9 + k] * re[k] + g[15 + k] * rate_e + g[12 + k] * s, (T)-3200, (T)3200);
    }
    // ---- the fixed mixer, PWM clip, PWM -> RPM -> thrust
    const T h0 = (T)0.5 * tau[0], h1 = (T)0.5 * tau[1];
    const T pwm[4] = {thrust + h0 - h1 - tau[2], thrust + h0 + h1 + tau[2], thrust - h0 + h1 - tau[2], thrust - h0 - h1 + tau[2]};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const T rpm = A.scale * m_clamp(pwm[j], A.min_pwm, A.max_pwm) + A.cnst;
        act[j] = A.kf * rpm * rpm;
    }
}

// The shared and the per-env gains go through ONE code path, with the feedback rollout's addressing: gain k lives at k * gs + gi with
// (gs, gi) = (N, i) per env and (1, 0) shared.
template <int SYS, typename T, bool DIST>
__global__ __launch_bounds__(64) void rollout_pid_kernel(const InstParams<T> I, const PidArgs<T> A) {
    static_assert(SYS == SCG_QUAD_2D || SYS == SCG_QUAD_3D, "the PID law serves Quadrotor 2D and 3D");
    using Ops = EnvOps<SYS, T, DIST, SCG_SEQ_ST_AUX>;
    using D = Dims<SYS>;
    constexpr int NX = D::NX, NU = D::NU;
    constexpr CfgParams<T> kcfg = scg_make_spec_cfg<T>();
    const PV<T> P{kcfg, I};
    const GoalTab<T> goal{nullptr, I.x_goal, false};
    const int i = I.env_first + blockIdx.x * blockDim.x + threadIdx.x;
    const size_t N = (size_t)I.num_envs;
    if (i >= I.env_end) return;
    typename Ops::E e;
    Ops::load_state(P, i, e);
    Ops::load_params(P, i, e);
    const RngKey key{I.key0, I.key1};
    const size_t gs = A.per_env ? N : 1, gi = A.per_env ? (size_t)i : 0;
    T g[18], ip[3], lr[3], ir[3];
#pragma unroll
    for (int k = 0; k < 18; ++k) g[k] = A.gains[(size_t)k * gs + gi];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        ip[k] = A.state ? A.state[(size_t)k * N + i] : (T)0;
        lr[k] = A.state ? A.state[(size_t)(3 + k) * N + i] : (T)0;
        ir[k] = A.state ? A.state[(size_t)(6 + k) * N + i] : (T)0;
    }
    const bool track = kcfg.task == SCG_TASK_TRAJ_TRACKING;
    const int last_row = kcfg.goal_rows - 1;
    T st[NX], row[2 * NX];
    Ops::state_vector(e, st);
    {
        const bool fresh = e.step == 0;
        const int32_t c0 = e.step - 1;
        Ops::obs_row(P, goal, st, e, key, fresh ? 1 : c0 + 2, fresh ? 0u : (uint32_t)(c0 + 1), fresh ? 0 : c0, i, nullptr, row);
    }
    T cost = (T)0, viol = (T)0, mse = (T)0;
    int n = 0;
    uint8_t fl = 0;
    for (int t = 0; t < A.k_steps; ++t) {
        const int32_t c0 = e.step;
        const T* gp = I.x_goal + (size_t)(track ? (c0 < last_row ? c0 : last_row) : 0) * NX;
        T pos[3], vel[3], ang[3], tp[3], tv[3], act[4], u[NU];
        if constexpr (SYS == SCG_QUAD_2D) {
            pos[0] = row[0]; pos[1] = (T)0; pos[2] = row[2];
            vel[0] = row[1]; vel[1] = (T)0; vel[2] = row[3];
            ang[0] = (T)0; ang[1] = row[4]; ang[2] = (T)0;
            tp[0] = gp[0]; tp[1] = (T)0; tp[2] = gp[2];
            tv[0] = track ? gp[1] : (T)0; tv[1] = (T)0; tv[2] = track ? gp[3] : (T)0;
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                pos[k] = row[2 * k]; vel[k] = row[2 * k + 1]; ang[k] = row[6 + k];
                tp[k] = gp[2 * k]; tv[k] = track ? gp[2 * k + 1] : (T)0;
            }
        }
        pid_law(pos, vel, ang, tp, tv, g, A, ip, lr, ir, act);
        if constexpr (SYS == SCG_QUAD_2D) {
            u[0] = act[0] + act[3]; u[1] = act[1] + act[2];
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) u[j] = act[j];
        }
        const size_t tn = (size_t)t * N + i;
#pragma unroll
        for (int k = 0; k < NX; ++k) A.x[((size_t)t * NX + k) * N + i] = row[k];
#pragma unroll
        for (int j = 0; j < NU; ++j) A.u[((size_t)t * NU + j) * N + i] = u[j];
        T noisy[NU];
        const typename Ops::StepResult r = Ops::step(P, goal, e, u, nullptr, key, i, st, noisy, seq_slot((T*)nullptr, 0), 0);
        Ops::obs_row(P, goal, st, e, key, c0 + 2, (uint32_t)(c0 + 1), c0, i, nullptr, row);
        cost -= r.reward;
        viol += (r.flags & FLAG_VIOLATION) ? (T)1 : (T)0;
        mse += r.mse;
        fl = r.flags;
        n = t + 1;
        if (A.reward) A.reward[tn] = r.reward;
        if (A.done) A.done[tn] = r.done ? 1 : 0;
        if (A.flags) A.flags[tn] = r.flags;
        if (r.done) break;
    }
#pragma unroll
    for (int k = 0; k < NX; ++k) A.final_obs[(size_t)k * N + i] = row[k];
    A.stats[i] = cost; A.stats[N + i] = (T)n; A.stats[2 * N + i] = viol; A.stats[3 * N + i] = mse;
    A.n_steps[i] = n;
    A.final_flags[i] = fl;
    if (A.state) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            A.state[(size_t)k * N + i] = ip[k];
            A.state[(size_t)(3 + k) * N + i] = lr[k];
            A.state[(size_t)(6 + k) * N + i] = ir[k];
        }
    }
    Ops::store(P, i, e, false);
}

}  // namespace scg

extern "C" int scg_rollout_pid(scg_env* env, int k_steps, const scg_pid_rollout* io, void* stream) {
    using namespace scg;
    using T = IlqrT;
    if (!env || !io) return fail(SCG_ERR_INVALID, "NULL argument to scg_rollout_pid");
    if (k_steps <= 0) return fail(SCG_ERR_INVALID, "k_steps must be positive");
    if (!io->d_gains || !io->d_x || !io->d_u || !io->d_final_obs || !io->d_stats || !io->d_n_steps || !io->d_final_flags)
        return fail(SCG_ERR_INVALID, "scg_rollout_pid needs d_gains, d_x, d_u, d_final_obs, d_stats, d_n_steps and d_final_flags");
    const scg_pid_config& c = io->config;
    if (!(c.kf > 0.0) || !(c.dt > 0.0) || !(c.pwm2rpm_scale != 0.0) || !(c.min_pwm <= c.max_pwm))
        return fail(SCG_ERR_INVALID, "scg_pid_config: kf and dt must be positive, pwm2rpm_scale non-zero, min_pwm <= max_pwm");
    if (!env->has_reset) return fail(SCG_ERR_STATE, "scg_reset (all envs) must be called before scg_rollout_pid");
    constexpr CfgParams<T> kcfg = scg_make_spec_cfg<T>();
    constexpr int S = SCG_SPEC_SYS;
    if constexpr (S != SCG_QUAD_2D && S != SCG_QUAD_3D) {
        (void)stream;
        return fail(SCG_ERR_INVALID, "scg_rollout_pid serves Quadrotor 2D and 3D (not CartPole, not Quadrotor 1D)");
    } else if constexpr (kcfg.nobs != Dims<S>::NX || kcfg.normalized_action) {
        (void)stream;
        return fail(SCG_ERR_INVALID, "scg_rollout_pid needs an env that observes its state (obs_dim = state_dim) and takes physical actions");
    } else {
        HIP_TRY(hipSetDevice(env->device));
        PidArgs<T> A;
        A.gains = (const T*)io->d_gains; A.state = (T*)io->d_pid_state;
        A.per_env = io->per_env ? 1 : 0; A.k_steps = k_steps;
        A.kf = (T)c.kf; A.gravity = (T)c.gravity; A.scale = (T)c.pwm2rpm_scale; A.cnst = (T)c.pwm2rpm_const;
        A.min_pwm = (T)c.min_pwm; A.max_pwm = (T)c.max_pwm; A.dt = (T)c.dt;
        A.x = (T*)io->d_x; A.u = (T*)io->d_u; A.final_obs = (T*)io->d_final_obs; A.stats = (T*)io->d_stats;
        A.n_steps = io->d_n_steps; A.final_flags = io->d_final_flags;
        A.reward = (T*)io->d_reward; A.done = io->d_done; A.flags = io->d_flags;
        const InstParams<T> I = inst_of<T>(env);
        const int grid = (env->cfg.num_envs + 63) / 64;
        rollout_pid_kernel<S, T, SCG_SPEC_DIST != 0><<<dim3(grid), dim3(64), 0, (hipStream_t)stream>>>(I, A);
        HIP_TRY(hipGetLastError());
        return SCG_OK;
    }
}

#endif  // SCG_CSRC_PID_H

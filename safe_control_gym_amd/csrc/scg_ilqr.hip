// scg_ilqr.hip — libscg_ilqr_<spechash>.so: the LQR / iLQR baseline controllers (include/scg_ilqr.h) next to everything
// libscg_spec_<hash>.so carries.  Two kernels, one thread = one environment, no MFMA (there is no dense contraction: every env is its
// own small problem):
//   rollout_feedback_kernel   step_sequence_kernel's structure (state in registers, the same EnvOps::step) with the action COMPUTED from
//                             an affine time-varying feedback instead of loaded; an env stops at its first done.
//   ilqr_backward_kernel      iLQR.update_policy: the Sm / Sv recursion in registers, the prior model's Jacobians by the central
//                             differences of prior_model_kernel (same EnvOps::sym_f), the Hessian's eigen-decomposition in closed form.
//
// Built only as   hipcc ... -DSCG_SPEC -include <spec header> scg_ilqr.hip   (safe_control_gym_amd/_ilqr.py); the simulator's
// translation unit is included whole, without any edit to it.  The PID baseline's rollout (scg_pid.h, include/scg_pid.h) is included at
// the end: one library per task config serves lqr, ilqr and pid.  So is the LDS-resident backward pass (scg_ilqr_wide.h,
// include/scg_ilqr_wide.h), which serves Quadrotor 3D as well.
#include "scg_kernels.hip"

#include "../../include/scg_ilqr.h"

#if !defined(SCG_SPEC)
#error "scg_ilqr.hip is built with -DSCG_SPEC -include <spec header>"
#endif

namespace scg {

#if SCG_SPEC_DTYPE == 1
using IlqrT = double;
#else
using IlqrT = float;
#endif

template <typename T>
struct FbArgs {
    const T* gains; const T* ff;
    int32_t schedule_len, per_env, k_steps;
    T* x; T* u; T* final_obs; T* stats;
    int32_t* n_steps; uint8_t* final_flags;
    T* reward; uint8_t* done; uint8_t* flags;
};

// The shared and the per-env schedule go through ONE code path: element (s, j, k) of the schedule lives at ((s * nu + j) * nx + k) * gs + gi
// with (gs, gi) = (N, i) per env and (1, 0) shared, so the two modes differ in addresses only and agree bit for bit.
template <int SYS, typename T, bool DIST>
__global__ __launch_bounds__(64) void rollout_feedback_kernel(const InstParams<T> I, const FbArgs<T> A) {
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
    const int last = A.schedule_len - 1;
    T Kc[NU][NX], fc[NU], Kn[NU][NX], fn[NU];
#pragma unroll
    for (int j = 0; j < NU; ++j) {
#pragma unroll
        for (int k = 0; k < NX; ++k) Kn[j][k] = A.gains[(size_t)(j * NX + k) * gs + gi];
        fn[j] = A.ff[(size_t)j * gs + gi];
    }
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
#pragma unroll
        for (int j = 0; j < NU; ++j) {
#pragma unroll
            for (int k = 0; k < NX; ++k) Kc[j][k] = Kn[j][k];
            fc[j] = fn[j];
        }
        if (t + 1 < A.k_steps && t < last) {                     // next step's gains: requested now, consumed one step later
            const size_t s = (size_t)(t + 1);
#pragma unroll
            for (int j = 0; j < NU; ++j) {
#pragma unroll
                for (int k = 0; k < NX; ++k) Kn[j][k] = A.gains[((s * NU + j) * NX + k) * gs + gi];
                fn[j] = A.ff[(s * NU + j) * gs + gi];
            }
        }
        T u[NU];
#pragma unroll
        for (int j = 0; j < NU; ++j) {
            T a = fc[j];
#pragma unroll
            for (int k = 0; k < NX; ++k) a += Kc[j][k] * row[k];
            u[j] = a;
        }
        const size_t tn = (size_t)t * N + i;
#pragma unroll
        for (int k = 0; k < NX; ++k) A.x[((size_t)t * NX + k) * N + i] = row[k];
#pragma unroll
        for (int j = 0; j < NU; ++j) A.u[((size_t)t * NU + j) * N + i] = u[j];
        const int32_t c0 = e.step;
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
    Ops::store(P, i, e, false);
}

template <typename T>
struct BwArgs {
    const T* x; const T* u; const int32_t* n_steps; const T* lamb; const uint8_t* mask;
    T* gains; T* ff; uint8_t* unstable;
    int32_t k_steps;
    T q[12], r[4], u_eq[4], par[4], arm, dt, eps;
};

// Symmetric 2 x 2 (a b; b d): eigenvalues l1 >= l2 and the unit eigenvector (vx, vy) of l1 (the other one is (-vy, vx)).
template <typename T>
__device__ __forceinline__ void sym2_eig(T a, T b, T d, T& l1, T& l2, T& vx, T& vy) {
    const T mean = (T)0.5 * (a + d), diff = (T)0.5 * (a - d);
    const T rad = m_sqrt(diff * diff + b * b);
    l1 = mean + rad; l2 = mean - rad;
    T px, py;
    if (diff >= (T)0) { px = diff + rad; py = b; } else { px = b; py = rad - diff; }      // the better conditioned of the two forms
    const T nrm = m_sqrt(px * px + py * py);
    if (nrm > (T)0) { vx = px / nrm; vy = py / nrm; } else { vx = (T)1; vy = (T)0; }
}

template <int SYS, typename T>
__global__ __launch_bounds__(64) void ilqr_backward_kernel(const InstParams<T> I, const BwArgs<T> B) {
    using Ops = EnvOps<SYS, T, false>;
    using D = Dims<SYS>;
    constexpr int NX = D::NX, NU = D::NU;
    static_assert(NU <= 2, "the closed-form eigen-decomposition serves one or two inputs");
    constexpr CfgParams<T> kcfg = scg_make_spec_cfg<T>();
    CfgParams<T> prior = kcfg;                                   // the prior model's constants: the task's, with the prior's moment arm
    prior.arm = B.arm;
    const PV<T> P{prior, I};
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const size_t N = (size_t)I.num_envs;
    if (i >= I.num_envs) return;
    if (B.mask && !B.mask[i]) return;
    typename Ops::E e;
#pragma unroll
    for (int k = 0; k < D::NP; ++k) e.par[k] = B.par[k];
    int n = B.n_steps[i];
    n = n < 0 ? 0 : (n > B.k_steps ? B.k_steps : n);
    const T lamb = B.lamb[i];
    const bool track = kcfg.task == SCG_TASK_TRAJ_TRACKING;
    const int last_row = kcfg.goal_rows - 1;
    const T dt = B.dt, eps = B.eps, inv2 = (T)0.5 / eps;
    T Sm[NX][NX], Sv[NX];
    {
        const int gr = track ? last_row : 0;
#pragma unroll
        for (int r = 0; r < NX; ++r) {
            Sv[r] = B.q[r] * (B.x[((size_t)n * NX + r) * N + i] - I.x_goal[gr * NX + r]);
#pragma unroll
            for (int c = 0; c < NX; ++c) Sm[r][c] = r == c ? B.q[r] : (T)0;
        }
    }
    bool bad = false;
    T x[NX], u[NU], xn[NX], un[NU];
    if (n > 0) {
#pragma unroll
        for (int r = 0; r < NX; ++r) xn[r] = B.x[((size_t)(n - 1) * NX + r) * N + i];
#pragma unroll
        for (int j = 0; j < NU; ++j) un[j] = B.u[((size_t)(n - 1) * NU + j) * N + i];
    }
    for (int k = n - 1; k >= 0; --k) {
#pragma unroll
        for (int r = 0; r < NX; ++r) x[r] = xn[r];
#pragma unroll
        for (int j = 0; j < NU; ++j) u[j] = un[j];
        if (k > 0) {                                             // the next operating point: requested now, consumed one step later
#pragma unroll
            for (int r = 0; r < NX; ++r) xn[r] = B.x[((size_t)(k - 1) * NX + r) * N + i];
#pragma unroll
            for (int j = 0; j < NU; ++j) un[j] = B.u[((size_t)(k - 1) * NU + j) * N + i];
        }
        // ---- linearised prior model about (x_k, u_k): prior_model_kernel's central differences, then the Euler discretisation
        T Ad[NX][NX], Bd[NX][NU];
#pragma unroll
        for (int c = 0; c < NX; ++c) {
            T xp[NX], xm[NX], fp[NX], fm[NX];
#pragma unroll
            for (int r = 0; r < NX; ++r) { xp[r] = x[r] + (r == c ? eps : (T)0); xm[r] = x[r] - (r == c ? eps : (T)0); }
            Ops::sym_f(P, e, xp, u, fp);
            Ops::sym_f(P, e, xm, u, fm);
#pragma unroll
            for (int r = 0; r < NX; ++r) Ad[r][c] = (r == c ? (T)1 : (T)0) + (fp[r] - fm[r]) * inv2 * dt;
        }
#pragma unroll
        for (int c = 0; c < NU; ++c) {
            T up[NU], um[NU], fp[NX], fm[NX];
#pragma unroll
            for (int j = 0; j < NU; ++j) { up[j] = u[j] + (j == c ? eps : (T)0); um[j] = u[j] - (j == c ? eps : (T)0); }
            Ops::sym_f(P, e, x, up, fp);
            Ops::sym_f(P, e, x, um, fm);
#pragma unroll
            for (int r = 0; r < NX; ++r) Bd[r][c] = (fp[r] - fm[r]) * inv2 * dt;
        }
        // ---- cost terms
        const int gr = track ? (k < last_row ? k : last_row) : 0;
        T Qv[NX], Rv[NU];
#pragma unroll
        for (int r = 0; r < NX; ++r) Qv[r] = B.q[r] * (x[r] - I.x_goal[gr * NX + r]);
#pragma unroll
        for (int j = 0; j < NU; ++j) Rv[j] = B.r[j] * (u[j] - B.u_eq[j]);
        // ---- g = Rv + Bd' Sv;  G = Bd' (Sm Ad);  H = R + Bd' (Sm Bd)
        T SA[NX][NX], SB[NX][NU];
#pragma unroll
        for (int r = 0; r < NX; ++r) {
#pragma unroll
            for (int c = 0; c < NX; ++c) {
                T a = (T)0;
#pragma unroll
                for (int m = 0; m < NX; ++m) a += Sm[r][m] * Ad[m][c];
                SA[r][c] = a;
            }
#pragma unroll
            for (int c = 0; c < NU; ++c) {
                T a = (T)0;
#pragma unroll
                for (int m = 0; m < NX; ++m) a += Sm[r][m] * Bd[m][c];
                SB[r][c] = a;
            }
        }
        T g[NU], G[NU][NX], H[NU][NU];
        T hsum = (T)0;
#pragma unroll
        for (int j = 0; j < NU; ++j) {
            T a = (T)0;
#pragma unroll
            for (int m = 0; m < NX; ++m) a += Bd[m][j] * Sv[m];
            g[j] = Rv[j] + a;
#pragma unroll
            for (int c = 0; c < NX; ++c) {
                T b = (T)0;
#pragma unroll
                for (int m = 0; m < NX; ++m) b += Bd[m][j] * SA[m][c];
                G[j][c] = b;
            }
#pragma unroll
            for (int c = 0; c < NU; ++c) {
                T b = (T)0;
#pragma unroll
                for (int m = 0; m < NX; ++m) b += Bd[m][j] * SB[m][c];
                H[j][c] = (j == c ? B.r[j] : (T)0) + b;
                hsum += H[j][c];
            }
        }
        if (!(hsum - hsum == (T)0)) { bad = true; continue; }     // inf or nan: the reference leaves this step's gains and the recursion alone
        // ---- H symmetrised, eigenvalues clipped at 0, + lamb, inverted through the eigenvectors
        T Hi[NU][NU];
        if constexpr (NU == 1) {
            Hi[0][0] = (T)1 / ((H[0][0] < (T)0 ? (T)0 : H[0][0]) + lamb);
        } else {
            const T off = (T)0.5 * (H[0][1] + H[1][0]);
            H[0][1] = H[1][0] = off;
            T l1, l2, vx, vy;
            sym2_eig(H[0][0], off, H[1][1], l1, l2, vx, vy);
            const T i1 = (T)1 / ((l1 < (T)0 ? (T)0 : l1) + lamb), i2 = (T)1 / ((l2 < (T)0 ? (T)0 : l2) + lamb);
            Hi[0][0] = vx * vx * i1 + vy * vy * i2;
            Hi[0][1] = Hi[1][0] = vx * vy * (i1 - i2);
            Hi[1][1] = vy * vy * i1 + vx * vx * i2;
        }
        T duff[NU], K[NU][NX];
#pragma unroll
        for (int j = 0; j < NU; ++j) {
            T a = (T)0;
#pragma unroll
            for (int m = 0; m < NU; ++m) a += Hi[j][m] * g[m];
            duff[j] = -a;
#pragma unroll
            for (int c = 0; c < NX; ++c) {
                T b = (T)0;
#pragma unroll
                for (int m = 0; m < NU; ++m) b += Hi[j][m] * G[m][c];
                K[j][c] = -b;
            }
        }
#pragma unroll
        for (int j = 0; j < NU; ++j) {
            T kx = (T)0;
#pragma unroll
            for (int c = 0; c < NX; ++c) {
                kx += K[j][c] * x[c];
                B.gains[(((size_t)k * NU + j) * NX + c) * N + i] = K[j][c];
            }
            B.ff[((size_t)k * NU + j) * N + i] = u[j] + duff[j] - kx;
        }
        // ---- Sm = Q + Ad' (Sm Ad) + K' (H K) + K' G + G' K;  Sv = Qv + Ad' Sv + K' (H duff) + K' g + G' duff
        T HK[NU][NX], Hd[NU];
#pragma unroll
        for (int j = 0; j < NU; ++j) {
            T a = (T)0;
#pragma unroll
            for (int m = 0; m < NU; ++m) a += H[j][m] * duff[m];
            Hd[j] = a;
#pragma unroll
            for (int c = 0; c < NX; ++c) {
                T b = (T)0;
#pragma unroll
                for (int m = 0; m < NU; ++m) b += H[j][m] * K[m][c];
                HK[j][c] = b;
            }
        }
        T Svn[NX];
#pragma unroll
        for (int r = 0; r < NX; ++r) {
            T a = (T)0, b = (T)0, c2 = (T)0, d2 = (T)0;
#pragma unroll
            for (int m = 0; m < NX; ++m) a += Ad[m][r] * Sv[m];
#pragma unroll
            for (int j = 0; j < NU; ++j) { b += K[j][r] * Hd[j]; c2 += K[j][r] * g[j]; d2 += G[j][r] * duff[j]; }
            Svn[r] = Qv[r] + a + b + c2 + d2;
        }
#pragma unroll
        for (int r = 0; r < NX; ++r) {
            T rowv[NX];
#pragma unroll
            for (int c = 0; c < NX; ++c) {
                T a = (T)0, b = (T)0, c2 = (T)0, d2 = (T)0;
#pragma unroll
                for (int m = 0; m < NX; ++m) a += Ad[m][r] * SA[m][c];
#pragma unroll
                for (int j = 0; j < NU; ++j) { b += K[j][r] * HK[j][c]; c2 += K[j][r] * G[j][c]; d2 += G[j][r] * K[j][c]; }
                rowv[c] = (r == c ? B.q[r] : (T)0) + a + b + c2 + d2;
            }
#pragma unroll
            for (int c = 0; c < NX; ++c) Sm[r][c] = rowv[c];
        }
#pragma unroll
        for (int r = 0; r < NX; ++r) Sv[r] = Svn[r];
    }
    if (bad) B.unstable[i] = 1;
}

}  // namespace scg

extern "C" int scg_rollout_feedback(scg_env* env, int k_steps, const scg_feedback_rollout* io, void* stream) {
    using namespace scg;
    using T = IlqrT;
    if (!env || !io) return fail(SCG_ERR_INVALID, "NULL argument to scg_rollout_feedback");
    if (k_steps <= 0) return fail(SCG_ERR_INVALID, "k_steps must be positive");
    if (io->schedule_len <= 0) return fail(SCG_ERR_INVALID, "schedule_len must be positive");
    if (!io->d_gains || !io->d_ff || !io->d_x || !io->d_u || !io->d_final_obs || !io->d_stats || !io->d_n_steps || !io->d_final_flags)
        return fail(SCG_ERR_INVALID, "scg_rollout_feedback needs d_gains, d_ff, d_x, d_u, d_final_obs, d_stats, d_n_steps and d_final_flags");
    if (!env->has_reset) return fail(SCG_ERR_STATE, "scg_reset (all envs) must be called before scg_rollout_feedback");
    constexpr CfgParams<T> kcfg = scg_make_spec_cfg<T>();
    constexpr int S = SCG_SPEC_SYS;
    if constexpr (kcfg.nobs != Dims<S>::NX || kcfg.normalized_action) {
        (void)stream;
        return fail(SCG_ERR_INVALID, "scg_rollout_feedback needs an env that observes its state (obs_dim = state_dim) and takes physical actions");
    } else {
        HIP_TRY(hipSetDevice(env->device));
        FbArgs<T> A;
        A.gains = (const T*)io->d_gains; A.ff = (const T*)io->d_ff;
        A.schedule_len = io->schedule_len; A.per_env = io->per_env ? 1 : 0; A.k_steps = k_steps;
        A.x = (T*)io->d_x; A.u = (T*)io->d_u; A.final_obs = (T*)io->d_final_obs; A.stats = (T*)io->d_stats;
        A.n_steps = io->d_n_steps; A.final_flags = io->d_final_flags;
        A.reward = (T*)io->d_reward; A.done = io->d_done; A.flags = io->d_flags;
        const InstParams<T> I = inst_of<T>(env);
        const int grid = (env->cfg.num_envs + 63) / 64;
        rollout_feedback_kernel<S, T, SCG_SPEC_DIST != 0><<<dim3(grid), dim3(64), 0, (hipStream_t)stream>>>(I, A);
        HIP_TRY(hipGetLastError());
        return SCG_OK;
    }
}

extern "C" int scg_ilqr_backward(scg_env* env, const scg_ilqr_model* model, int k_steps, const void* d_x, const void* d_u,
                                 const int32_t* d_n_steps, const void* d_lamb, const uint8_t* d_mask, void* d_gains, void* d_ff,
                                 uint8_t* d_unstable, void* stream) {
    using namespace scg;
    using T = IlqrT;
    if (!env || !model) return fail(SCG_ERR_INVALID, "NULL argument to scg_ilqr_backward");
    if (k_steps <= 0) return fail(SCG_ERR_INVALID, "k_steps must be positive");
    if (!d_x || !d_u || !d_n_steps || !d_lamb || !d_gains || !d_ff || !d_unstable)
        return fail(SCG_ERR_INVALID, "scg_ilqr_backward needs d_x, d_u, d_n_steps, d_lamb, d_gains, d_ff and d_unstable");
    if (!(model->dt > 0.0) || !(model->eps > 0.0)) return fail(SCG_ERR_INVALID, "scg_ilqr_model: dt and eps must be positive");
    constexpr int S = SCG_SPEC_SYS;
    if constexpr (S == SCG_QUAD_3D) {
        (void)d_mask; (void)stream;
        return fail(SCG_ERR_INVALID, "scg_ilqr_backward serves CartPole, Quadrotor 1D and Quadrotor 2D (not the 12-state, 4-input Quadrotor 3D)");
    } else {
        HIP_TRY(hipSetDevice(env->device));
        BwArgs<T> B;
        B.x = (const T*)d_x; B.u = (const T*)d_u; B.n_steps = d_n_steps; B.lamb = (const T*)d_lamb; B.mask = d_mask;
        B.gains = (T*)d_gains; B.ff = (T*)d_ff; B.unstable = d_unstable; B.k_steps = k_steps;
        for (int k = 0; k < 12; ++k) B.q[k] = (T)model->q[k];
        for (int k = 0; k < 4; ++k) { B.r[k] = (T)model->r[k]; B.u_eq[k] = (T)model->u_eq[k]; B.par[k] = (T)model->par[k]; }
        B.arm = (T)model->arm; B.dt = (T)model->dt; B.eps = (T)model->eps;
        const InstParams<T> I = inst_of<T>(env);
        const int grid = (env->cfg.num_envs + 63) / 64;
        ilqr_backward_kernel<S, T><<<dim3(grid), dim3(64), 0, (hipStream_t)stream>>>(I, B);
        HIP_TRY(hipGetLastError());
        return SCG_OK;
    }
}

extern "C" int scg_ilqr_snapshot(scg_env* env, void* d_state, void* stream) {
    if (!env || !d_state) return fail(SCG_ERR_INVALID, "NULL argument to scg_ilqr_snapshot");
    HIP_TRY(hipSetDevice(env->device));
    const size_t bytes = (size_t)env->ns * env->cfg.num_envs * sizeof(scg::IlqrT);
    HIP_TRY(hipMemcpyAsync(d_state, env->d_state, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return SCG_OK;
}

extern "C" int scg_ilqr_restart(scg_env* env, const void* d_state, void* stream) {
    if (!env || !d_state) return fail(SCG_ERR_INVALID, "NULL argument to scg_ilqr_restart");
    HIP_TRY(hipSetDevice(env->device));
    const size_t bytes = (size_t)env->ns * env->cfg.num_envs * sizeof(scg::IlqrT);
    HIP_TRY(hipMemcpyAsync(env->d_state, d_state, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    HIP_TRY(hipMemsetAsync(env->d_step, 0, (size_t)env->cfg.num_envs * 4, (hipStream_t)stream));
    return SCG_OK;
}

#include "scg_pid.h"
#include "scg_ilqr_wide.h"

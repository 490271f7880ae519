// scg_ilqr_wide.h — iLQR's backward pass with its matrices resident in LDS (include/scg_ilqr_wide.h).  Included by scg_ilqr.hip
// after its own kernels: ilqr_backward_wide_kernel is ilqr_backward_kernel's recursion, statement for statement and in the same order
// of summation, for systems whose NX x NX matrices do not fit the register file (Quadrotor 3D: Sm, SA = Sm Ad and Ad are 3 x 144
// words).  One thread = one env, no cross-lane traffic and no barrier: a lane only ever touches its own column of the LDS image
// [element][env of the block] (the env index is the fastest, so one wave access to one element is one contiguous, conflict-free row).
// Sm, SA, Ad (NX x NX) and G, K (NU x NX) live there; Bd, H, its inverse, the vectors and ONE central-difference column at a time
// stay in registers.  Loops whose indices only form LDS addresses run as loops, loops that index register arrays are unrolled.
#ifndef SCG_CSRC_ILQR_WIDE_H
#define SCG_CSRC_ILQR_WIDE_H

#include "../../include/scg_ilqr_wide.h"

namespace scg {

// Symmetric 4 x 4 H -> Hi = V diag(1 / (max(l, 0) + lamb)) V' by cyclic Jacobi (include/scg_ilqr_wide.h).  H = V diag(l) V', the
// eigenvectors in V's columns; every rotation keeps V orthonormal to rounding, whatever H's eigenvalues are.
template <typename T>
__device__ __forceinline__ void sym4_jacobi_inverse(const T (&H)[4][4], T lamb, T (&Hi)[4][4]) {
    T A[4][4], V[4][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int c = 0; c < 4; ++c) { A[j][c] = H[j][c]; V[j][c] = j == c ? (T)1 : (T)0; }
    }
#pragma unroll 1
    for (int sweep = 0; sweep < SCG_ILQR_JACOBI_SWEEPS; ++sweep) {
#pragma unroll
        for (int p = 0; p < 3; ++p) {
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                const T apq = A[p][q];
                if (apq != (T)0) {
                    const T theta = (A[q][q] - A[p][p]) / ((T)2 * apq);
                    const T ath = theta < (T)0 ? -theta : theta;
                    const T tt = (T)1 / (ath + m_sqrt(theta * theta + (T)1));
                    const T t = theta < (T)0 ? -tt : tt;
                    const T cs = (T)1 / m_sqrt(t * t + (T)1), sn = t * cs;
                    A[p][p] -= t * apq;
                    A[q][q] += t * apq;
                    A[p][q] = A[q][p] = (T)0;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        if (k != p && k != q) {
                            const T akp = A[k][p], akq = A[k][q];
                            A[k][p] = A[p][k] = cs * akp - sn * akq;
                            A[k][q] = A[q][k] = sn * akp + cs * akq;
                        }
                    }
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const T vkp = V[k][p], vkq = V[k][q];
                        V[k][p] = cs * vkp - sn * vkq;
                        V[k][q] = sn * vkp + cs * vkq;
                    }
                }
            }
        }
    }
    T W[4][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const T il = (T)1 / ((A[k][k] < (T)0 ? (T)0 : A[k][k]) + lamb);
#pragma unroll
        for (int j = 0; j < 4; ++j) W[j][k] = V[j][k] * il;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
        for (int m = j; m < 4; ++m) {
            T a = (T)0;
#pragma unroll
            for (int k = 0; k < 4; ++k) a += W[j][k] * V[m][k];
            Hi[j][m] = Hi[m][j] = a;
        }
    }
}

extern __shared__ __align__(16) unsigned char ilqr_wide_lds[];

// Between the iterations of an unrolled loop that reads a row or a column from LDS: the scheduler may not gather the loads of all
// iterations up front (144 live values), which is what spills.
#define ILQR_WIDE_FENCE() __builtin_amdgcn_sched_barrier(0)

// EPB = envs per block = threads per block.  LDS: T [3 NX NX + 2 NU NX][EPB]: Sm, then SA, then Ad, element (r, c) of each at row
// r NX + c, then G and K [NU][NX] each.  (G beside K in registers is 192 of the 256 architectural VGPRs in float64: it spilled.)
template <int SYS, typename T, int EPB>
__global__ __launch_bounds__(EPB) void ilqr_backward_wide_kernel(const InstParams<T> I, const BwArgs<T> B) {
    using Ops = EnvOps<SYS, T, false>;
    using D = Dims<SYS>;
    constexpr int NX = D::NX, NU = D::NU, NN = NX * NX;
    static_assert(NU <= 2 || NU == 4, "closed-form eigen-decomposition for one or two inputs, Jacobi for four");
    constexpr CfgParams<T> kcfg = scg_make_spec_cfg<T>();
    CfgParams<T> prior = kcfg;                                   // the prior model's constants: the task's, with the prior's moment arm
    prior.arm = B.arm;
    const PV<T> P{prior, I};
    const int i = blockIdx.x * EPB + threadIdx.x;
    const size_t N = (size_t)I.num_envs;
    if (i >= I.num_envs) return;
    if (B.mask && !B.mask[i]) return;
    T* const sm = reinterpret_cast<T*>(ilqr_wide_lds) + threadIdx.x;        // this env's column of the LDS image
    // One base register per matrix, each opaque to the compiler: folded into ONE base, the element offsets pass the 16 bits of a DS
    // instruction's immediate (64 KB) and every address becomes a register of its own, kept live and spilled.
    int o_sa = NN * EPB, o_ad = 2 * NN * EPB, o_gl = 3 * NN * EPB, o_kl = (3 * NN + NU * NX) * EPB;
    asm volatile("" : "+s"(o_sa), "+s"(o_ad), "+s"(o_gl), "+s"(o_kl));
    T* const sa = sm + o_sa;
    T* const ad = sm + o_ad;
    T* const gl = sm + o_gl;                                      // G [NU][NX]
    T* const kl = sm + o_kl;                                      // K [NU][NX]
    typename Ops::E e;
#pragma unroll
    for (int k = 0; k < D::NP; ++k) e.par[k] = B.par[k];
    int n = B.n_steps[i];
    n = n < 0 ? 0 : (n > B.k_steps ? B.k_steps : n);
    const T lamb = B.lamb[i];
    const bool track = kcfg.task == SCG_TASK_TRAJ_TRACKING;
    const int last_row = kcfg.goal_rows - 1;
    const T dt = B.dt, eps = B.eps, inv2 = (T)0.5 / eps;
    T Sv[NX];
    {
        const int gr = track ? last_row : 0;
#pragma unroll
        for (int r = 0; r < NX; ++r) {
            Sv[r] = B.q[r] * (B.x[((size_t)n * NX + r) * N + i] - I.x_goal[gr * NX + r]);
#pragma unroll
            for (int c = 0; c < NX; ++c) sm[(r * NX + c) * EPB] = r == c ? B.q[r] : (T)0;
        }
    }
    bool bad = false;
    T x[NX], u[NU];
    for (int k = n - 1; k >= 0; --k) {
        // (no request one step ahead as in ilqr_backward_kernel: a step here is thousands of cycles, and 16 more live values spill)
        {
            const T* const xk = B.x + (size_t)k * NX * N + i;
            const T* const uk = B.u + (size_t)k * NU * N + i;
#pragma unroll
            for (int r = 0; r < NX; ++r) x[r] = xk[(size_t)r * N];
#pragma unroll
            for (int j = 0; j < NU; ++j) u[j] = uk[(size_t)j * N];
        }
        // ---- Bd = B_c dt by central differences
        T Bd[NX][NU], H[NU][NU];
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
        // ---- Ad = I + A_c dt, one central-difference column at a time: stored, and consumed into SA[:, c] = Sm Ad[:, c] and
        //      G[:, c] = Bd' SA[:, c] at once
#pragma unroll 1
        for (int c = 0; c < NX; ++c) {
            T xp[NX], xm[NX], fp[NX], fm[NX], col[NX];
#pragma unroll
            for (int r = 0; r < NX; ++r) { xp[r] = x[r] + (r == c ? eps : (T)0); xm[r] = x[r] - (r == c ? eps : (T)0); }
            Ops::sym_f(P, e, xp, u, fp);
            Ops::sym_f(P, e, xm, u, fm);
#pragma unroll
            for (int r = 0; r < NX; ++r) {
                col[r] = (r == c ? (T)1 : (T)0) + (fp[r] - fm[r]) * inv2 * dt;
                ad[(r * NX + c) * EPB] = col[r];
            }
            T Gc[NU];
#pragma unroll
            for (int j = 0; j < NU; ++j) Gc[j] = (T)0;
#pragma unroll
            for (int r = 0; r < NX; ++r) {
                T a = (T)0;
#pragma unroll
                for (int m = 0; m < NX; ++m) a += sm[(r * NX + m) * EPB] * col[m];
                sa[(r * NX + c) * EPB] = a;
#pragma unroll
                for (int j = 0; j < NU; ++j) Gc[j] += Bd[r][j] * a;
                ILQR_WIDE_FENCE();
            }
#pragma unroll
            for (int j = 0; j < NU; ++j) gl[(j * NX + c) * EPB] = Gc[j];
        }
        // ---- H = R + Bd' (Sm Bd), row m of SB = Sm Bd at a time (summed over m ascending)
#pragma unroll
        for (int j = 0; j < NU; ++j) {
#pragma unroll
            for (int c = 0; c < NU; ++c) H[j][c] = (T)0;
        }
#pragma unroll
        for (int m = 0; m < NX; ++m) {
            T row[NX], SB[NU];
#pragma unroll
            for (int l = 0; l < NX; ++l) row[l] = sm[(m * NX + l) * EPB];
#pragma unroll
            for (int c = 0; c < NU; ++c) {
                T a = (T)0;
#pragma unroll
                for (int l = 0; l < NX; ++l) a += row[l] * Bd[l][c];
                SB[c] = a;
            }
#pragma unroll
            for (int j = 0; j < NU; ++j) {
#pragma unroll
                for (int c = 0; c < NU; ++c) H[j][c] += Bd[m][j] * SB[c];
            }
            ILQR_WIDE_FENCE();
        }
        // ---- g = Rv + Bd' Sv;  the finite-sum test on H
        T g[NU];
        T hsum = (T)0;
#pragma unroll
        for (int j = 0; j < NU; ++j) {
            T a = (T)0;
#pragma unroll
            for (int m = 0; m < NX; ++m) a += Bd[m][j] * Sv[m];
            g[j] = B.r[j] * (u[j] - B.u_eq[j]) + a;
#pragma unroll
            for (int c = 0; c < NU; ++c) {
                H[j][c] = (j == c ? B.r[j] : (T)0) + H[j][c];
                hsum += H[j][c];
            }
        }
        if (!(hsum - hsum == (T)0)) { bad = true; continue; }     // inf or nan: this step's gains and Sm, Sv stay (SA, Ad, G, K are rebuilt per step)
        // ---- H symmetrised, eigenvalues clipped at 0, + lamb, inverted through the eigenvectors
        T Hi[NU][NU];
        if constexpr (NU == 1) {
            Hi[0][0] = (T)1 / ((H[0][0] < (T)0 ? (T)0 : H[0][0]) + lamb);
        } else if constexpr (NU == 2) {
            const T off = (T)0.5 * (H[0][1] + H[1][0]);
            H[0][1] = H[1][0] = off;
            T l1, l2, vx, vy;
            sym2_eig(H[0][0], off, H[1][1], l1, l2, vx, vy);
            const T i1 = (T)1 / ((l1 < (T)0 ? (T)0 : l1) + lamb), i2 = (T)1 / ((l2 < (T)0 ? (T)0 : l2) + lamb);
            Hi[0][0] = vx * vx * i1 + vy * vy * i2;
            Hi[0][1] = Hi[1][0] = vx * vy * (i1 - i2);
            Hi[1][1] = vy * vy * i1 + vx * vx * i2;
        } else {
#pragma unroll
            for (int j = 0; j < NU; ++j) {
#pragma unroll
                for (int c = j + 1; c < NU; ++c) H[j][c] = H[c][j] = (T)0.5 * (H[j][c] + H[c][j]);
            }
            sym4_jacobi_inverse(H, lamb, Hi);
        }
        // ---- duff = -Hinv g;  K = -Hinv G, column by column: to LDS and to the schedule;  ff = u + duff - K x
        T duff[NU], kx[NU];
#pragma unroll
        for (int j = 0; j < NU; ++j) {
            T a = (T)0;
#pragma unroll
            for (int m = 0; m < NU; ++m) a += Hi[j][m] * g[m];
            duff[j] = -a;
            kx[j] = (T)0;
        }
        T* const gk = B.gains + (size_t)k * NU * NX * N + i;
        T* const fk = B.ff + (size_t)k * NU * N + i;
#pragma unroll
        for (int c = 0; c < NX; ++c) {
            T Gc[NU];
#pragma unroll
            for (int m = 0; m < NU; ++m) Gc[m] = gl[(m * NX + c) * EPB];
#pragma unroll
            for (int j = 0; j < NU; ++j) {
                T b = (T)0;
#pragma unroll
                for (int m = 0; m < NU; ++m) b += Hi[j][m] * Gc[m];
                const T Kjc = -b;
                kl[(j * NX + c) * EPB] = Kjc;
                gk[(size_t)(j * NX + c) * N] = Kjc;
                kx[j] += Kjc * x[c];
            }
            ILQR_WIDE_FENCE();
        }
#pragma unroll
        for (int j = 0; j < NU; ++j) fk[(size_t)j * N] = u[j] + duff[j] - kx[j];
        // ---- Sv = Qv + Ad' Sv + K' (H duff) + K' g + G' duff
        T Hd[NU];
#pragma unroll
        for (int j = 0; j < NU; ++j) {
            T a = (T)0;
#pragma unroll
            for (int m = 0; m < NU; ++m) a += H[j][m] * duff[m];
            Hd[j] = a;
        }
        const int gr = track ? (k < last_row ? k : last_row) : 0;
        T Svn[NX];
#pragma unroll
        for (int r = 0; r < NX; ++r) {
            const T Qv = B.q[r] * (x[r] - I.x_goal[gr * NX + r]);
            T a = (T)0, b = (T)0, c2 = (T)0, d2 = (T)0;
#pragma unroll
            for (int m = 0; m < NX; ++m) a += ad[(m * NX + r) * EPB] * Sv[m];
#pragma unroll
            for (int j = 0; j < NU; ++j) {
                const T Kjr = kl[(j * NX + r) * EPB];
                b += Kjr * Hd[j]; c2 += Kjr * g[j]; d2 += gl[(j * NX + r) * EPB] * duff[j];
            }
            Svn[r] = Qv + a + b + c2 + d2;
            ILQR_WIDE_FENCE();
        }
#pragma unroll
        for (int r = 0; r < NX; ++r) Sv[r] = Svn[r];
        // ---- Sm = Q + Ad' (Sm Ad) + K' (H K) + K' G + G' K, written over the old Sm: nothing reads it once SA and H exist
#pragma unroll 1
        for (int c = 0; c < NX; ++c) {
            T col[NX], Kc[NU], Gc[NU], HK[NU];
            T qc = (T)0;
#pragma unroll
            for (int m = 0; m < NX; ++m) { col[m] = sa[(m * NX + c) * EPB]; qc = m == c ? B.q[m] : qc; }
#pragma unroll
            for (int j = 0; j < NU; ++j) { Kc[j] = kl[(j * NX + c) * EPB]; Gc[j] = gl[(j * NX + c) * EPB]; }
#pragma unroll
            for (int j = 0; j < NU; ++j) {
                T b = (T)0;
#pragma unroll
                for (int m = 0; m < NU; ++m) b += H[j][m] * Kc[m];
                HK[j] = b;
            }
#pragma unroll 1
            for (int r = 0; r < NX; ++r) {
                T a = (T)0, b = (T)0, c2 = (T)0, d2 = (T)0;
#pragma unroll
                for (int m = 0; m < NX; ++m) a += ad[(m * NX + r) * EPB] * col[m];
#pragma unroll
                for (int j = 0; j < NU; ++j) {
                    const T Kjr = kl[(j * NX + r) * EPB];
                    b += Kjr * HK[j]; c2 += Kjr * Gc[j]; d2 += gl[(j * NX + r) * EPB] * Kc[j];
                }
                sm[(r * NX + c) * EPB] = (r == c ? qc : (T)0) + a + b + c2 + d2;
            }
        }
    }
    if (bad) B.unstable[i] = 1;
}

}  // namespace scg

extern "C" int scg_ilqr_backward_wide(scg_env* env, const scg_ilqr_model* model, int k_steps, const void* d_x, const void* d_u,
                                      const int32_t* d_n_steps, const void* d_lamb, const uint8_t* d_mask, void* d_gains, void* d_ff,
                                      uint8_t* d_unstable, void* stream) {
    using namespace scg;
    using T = IlqrT;
    if (!env || !model) return fail(SCG_ERR_INVALID, "NULL argument to scg_ilqr_backward_wide");
    if (k_steps <= 0) return fail(SCG_ERR_INVALID, "k_steps must be positive");
    if (!d_x || !d_u || !d_n_steps || !d_lamb || !d_gains || !d_ff || !d_unstable)
        return fail(SCG_ERR_INVALID, "scg_ilqr_backward_wide needs d_x, d_u, d_n_steps, d_lamb, d_gains, d_ff and d_unstable");
    if (!(model->dt > 0.0) || !(model->eps > 0.0)) return fail(SCG_ERR_INVALID, "scg_ilqr_model: dt and eps must be positive");
    constexpr int S = SCG_SPEC_SYS;
    constexpr int EPB = sizeof(T) == 8 ? 32 : 64;                // 528 words per env on Quadrotor 3D: 135 168 B either way
    constexpr int bytes = (3 * Dims<S>::NX + 2 * Dims<S>::NU) * Dims<S>::NX * EPB * (int)sizeof(T);
    static_assert(bytes <= 160 * 1024, "the LDS image must fit one workgroup's 160 KB");
    HIP_TRY(hipSetDevice(env->device));
    static scg::PerDeviceOnce attr;         // (per device, scg_once.h: the handle's device is current)
    int dev;
    if (attr.pending(&dev)) {
        HIP_TRY(hipFuncSetAttribute((const void*)ilqr_backward_wide_kernel<S, T, EPB>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
        attr.commit(dev);
    }
    BwArgs<T> B;
    B.x = (const T*)d_x; B.u = (const T*)d_u; B.n_steps = d_n_steps; B.lamb = (const T*)d_lamb; B.mask = d_mask;
    B.gains = (T*)d_gains; B.ff = (T*)d_ff; B.unstable = d_unstable; B.k_steps = k_steps;
    for (int k = 0; k < 12; ++k) B.q[k] = (T)model->q[k];
    for (int k = 0; k < 4; ++k) { B.r[k] = (T)model->r[k]; B.u_eq[k] = (T)model->u_eq[k]; B.par[k] = (T)model->par[k]; }
    B.arm = (T)model->arm; B.dt = (T)model->dt; B.eps = (T)model->eps;
    const InstParams<T> I = inst_of<T>(env);
    const int grid = (env->cfg.num_envs + EPB - 1) / EPB;
    ilqr_backward_wide_kernel<S, T, EPB><<<dim3(grid), dim3(EPB), bytes, (hipStream_t)stream>>>(I, B);
    HIP_TRY(hipGetLastError());
    return SCG_OK;
}

#endif /* SCG_CSRC_ILQR_WIDE_H */

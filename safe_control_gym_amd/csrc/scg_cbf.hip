// scg_cbf.hip — libscg_cbfroll_<spechash>_<H>_<act>.so: the CBF-QP safety filter (include/scg_cbf.h) as a batched certify kernel and
// as the policy rollout with the filter between the actor and the env step, next to everything libscg_spec_<hash>.so carries.
//
// Built only as   hipcc ... -DSCG_SPEC -include <spec header> -DSCG_POLICY_H=<H> -DSCG_POLICY_ACT=<act> scg_cbf.hip
// (safe_control_gym_amd/_cbf.py).  As in scg_safe_explorer.hip the simulator's translation unit is included whole, without any edit to
// it; rollout_cbf_kernel follows rollout_policy_kernel (scg_env_kernels.h) step for step and adds cbf_certify between the action and
// the env step.  The filter is ~60 flops, one sincos and three divisions per env-step beside the ~9 k-flop actor and the engine
// substeps; its temporaries die before the env step, so the kernel keeps rollout_policy_kernel's register class and LDS layout
// (the actor image + the obs transpose scratch) and adds no scratch (DESIGN.md has the numbers).
#include "scg_kernels.hip"

#include "../../include/scg_cbf.h"

#if !defined(SCG_SPEC) || !defined(SCG_POLICY_H)
#error "scg_cbf.hip is built with -DSCG_SPEC -include <spec header> -DSCG_POLICY_H= -DSCG_POLICY_ACT="
#endif

namespace scg {

struct CbfResult { float u0, u, s, feasible; };

// The closed-form minimiser of the reference's CBF-QP (include/scg_cbf.h) for one (state, physical action).  Every operation is an
// explicitly rounded float32 one (no contraction), so the two kernels that call it agree bit for bit.
__device__ __forceinline__ CbfResult cbf_certify(const scg_cbf_params& p, const float* X, float u_phys) {
    // barrier and its gradient
    float h = 1.0f, gr[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float q = __fdiv_rn(X[i], p.L[i]);
        h = __fsub_rn(h, __fmul_rn(q, q));
        gr[i] = __fdiv_rn(__fmul_rn(-2.0f, X[i]), __fmul_rn(p.L[i], p.L[i]));
    }
    // prior dynamics f(X, 0) and f(X, 1) - f(X, 0)  (cartpole.py:412-414; f is affine in the force)
    float sn, cs;
    m_sincos(X[2], &sn, &cs);
    const float Mm = __fadd_rn(p.m, p.M), ml = __fmul_rn(p.m, p.l);
    const float tmp0 = __fdiv_rn(__fmul_rn(__fmul_rn(ml, __fmul_rn(X[3], X[3])), sn), Mm);
    const float den = __fmul_rn(p.l, __fsub_rn(4.0f / 3.0f, __fdiv_rn(__fmul_rn(p.m, __fmul_rn(cs, cs)), Mm)));
    const float thdd0 = __fdiv_rn(__fsub_rn(__fmul_rn(p.g, sn), __fmul_rn(cs, tmp0)), den);
    const float xdd0 = __fsub_rn(tmp0, __fdiv_rn(__fmul_rn(__fmul_rn(ml, thdd0), cs), Mm));
    const float dtmp = __fdiv_rn(1.0f, Mm);
    const float dthdd = __fdiv_rn(-__fmul_rn(cs, dtmp), den);
    const float dxdd = __fsub_rn(dtmp, __fdiv_rn(__fmul_rn(__fmul_rn(ml, dthdd), cs), Mm));
    const float a = __fadd_rn(__fadd_rn(__fmul_rn(gr[0], X[1]), __fmul_rn(gr[1], xdd0)), __fadd_rn(__fmul_rn(gr[2], X[3]), __fmul_rn(gr[3], thdd0)));
    const float b = __fadd_rn(__fmul_rn(gr[1], dxdd), __fmul_rn(gr[3], dthdd));
    const float k = __fadd_rn(__fmul_rn(p.slope, h), a);
    CbfResult o;
    o.u0 = fminf(fmaxf(u_phys, p.lo), p.hi);
    const float r0 = __fsub_rn(-k, __fmul_rn(b, o.u0));
    o.u = o.u0; o.s = 0.0f; o.feasible = 1.0f;
    if (r0 > 0.0f) {
        if (p.soft) {
            const float wb2 = __fmul_rn(__fmul_rn(2.0f, p.slack_weight), b);                    // 2 w b
            const float u1 = __fdiv_rn(__fsub_rn(o.u0, __fmul_rn(wb2, k)), __fadd_rn(1.0f, __fmul_rn(wb2, b)));
            o.u = fminf(fmaxf(u1, p.lo), p.hi);
            o.s = fmaxf(0.0f, __fsub_rn(-k, __fmul_rn(b, o.u)));
            o.feasible = o.s <= p.slack_tolerance ? 1.0f : 0.0f;
        } else {
            const float ub = __fdiv_rn(-k, b);                      // the row's boundary: u >= ub (b > 0) or u <= ub (b < 0)
            const bool ok = (b > 0.0f || b < 0.0f) && ub >= p.lo && ub <= p.hi;
            o.u = ok ? ub : o.u0;
            o.feasible = ok ? 1.0f : 0.0f;
        }
    }
    return o;
}

__global__ __launch_bounds__(256) void cbf_certify_kernel(const scg_cbf_params p, const float* __restrict__ state, const float* __restrict__ action,
                                                          float* __restrict__ certified, float* __restrict__ slack, uint8_t* __restrict__ feasible,
                                                          int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const f32x4 x = *reinterpret_cast<const f32x4*>(state + (size_t)4 * i);
    const float X[4] = {x.x, x.y, x.z, x.w};
    const CbfResult o = cbf_certify(p, X, action[i]);
    certified[i] = o.u;
    if (slack) slack[i] = o.s;
    feasible[i] = o.feasible != 0.0f ? 1 : 0;
}

#if SCG_SPEC_SYS == 0 && SCG_SPEC_DTYPE == 0     // SCG_CARTPOLE, float32
#define SCG_CBF_ROLLOUT 1

struct CbfArgs {
    MlpWeights actor;
    const float* logstd;                           // [NU]
    scg_cbf_params p;
    float* rows;                                   // [K][N][4]
    float* applied;                                // [K][N]
};

// rollout_policy_kernel + the filter.  The LDS layout is rollout_policy_kernel's: the actor image, then the obs transpose scratch.
template <int EPW, int WPW>
__global__ __launch_bounds__(64 * WPW) void rollout_cbf_kernel(const InstParams<float> I, const PolicyArgs A, const CbfArgs B) {
    using T = float;
    constexpr int SYS = SCG_SPEC_SYS;
    constexpr bool DIST = SCG_SPEC_DIST != 0;
    using Ops = EnvOps<SYS, T, DIST, SCG_SEQ_ST_AUX>;
    using D = Dims<SYS>;
    constexpr CfgParams<T> kcfg = scg_make_spec_cfg<T>();
    constexpr int NIN = kcfg.nobs, NU = D::NU, HID = SCG_POLICY_H, ACT = SCG_POLICY_ACT;
    static_assert(NU == 1 && D::NX == 4, "the CBF filter serves the cartpole (one input, four states)");
    static_assert(NIN == D::NX || NIN == 2 * D::NX, "the fused rollout serves single-row observations (goal horizon <= 1)");
    using LP = MlpLds<NIN, HID, NU, 16>;
    constexpr int L1Q = LP::L1Q;
    extern __shared__ __align__(16) float lds[];
    unsigned char* const s_obs = reinterpret_cast<unsigned char*>(lds + LP::END);       // [WPW waves][64 rows][NIN] transpose scratch
    const PV<T> P{kcfg, I};
    const GoalTab<T> goal{nullptr, I.x_goal, false};
    mlp_fill_lds<NIN, HID, NU, 16, 64 * WPW>(lds, B.actor, threadIdx.x);
    __syncthreads();
    const int N = I.num_envs;
    static_assert(EPW == 64 || EPW == 32, "envs per wave");
    const int lane = threadIdx.x & 63, h = lane >> 5;
    const int i0 = EPW == 64 ? blockIdx.x * (64 * WPW) + threadIdx.x : (blockIdx.x * WPW + (threadIdx.x >> 6)) * 32 + (lane & 31);
    const bool live = i0 < N && (EPW == 64 || h == 0);
    const int i = i0 < N ? i0 : N - 1;                // surplus lanes shadow the last env (they take part in the MFMAs, never store)
    const bool full_wave = EPW == 64 && (blockIdx.x * (64 * WPW) + (threadIdx.x & ~63) + 64) <= N;
    unsigned char* const s_wave = s_obs + (threadIdx.x >> 6) * (64 * NIN * (int)sizeof(T));
    typename Ops::E e;
    Ops::load_state(P, i, e);
    Ops::load_params(P, i, e);
    const RngKey key{I.key0, I.key1};
    float ep[4] = {0.0f, 0.0f, 0.0f, 0.0f}, acc[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (A.ep_stats) seq_slot(A.ep_stats, i, 4).template load_row<4>(ep);
    if (A.episode_acc) seq_slot(A.episode_acc, i, 8).template load_row<8>(acc);
    float logstd[NU], sigma[NU], logp_const = 0.0f;
#pragma unroll
    for (int a = 0; a < NU; ++a) {
        logstd[a] = B.logstd[a];
        sigma[a] = __expf(logstd[a]);
        logp_const -= logstd[a] + 0.91893853320467274f;
    }
    T st[D::NX], row[2 * D::NX];
    Ops::state_vector(e, st);
    {
        const bool fresh = e.step == 0;
        const int32_t c0 = e.step - 1;
        Ops::obs_row(P, goal, st, e, key, fresh ? 1 : c0 + 2, fresh ? 0u : (uint32_t)(c0 + 1), fresh ? 0 : c0, i, nullptr, row);
    }
    bool dirty = false;
    for (int t = 0; t <= A.k_steps; ++t) {
        // ---- rollout row obs[t]
        {
            const Slot<T, SCG_SEQ_ST_AUX> dst = seq_slot(A.obs + (size_t)t * N * NIN, i, NIN);
            if constexpr ((NIN * (int)sizeof(T)) % 16 == 0) {
                if (full_wave) store_rows_coalesced<T, NIN>(dst, row, s_wave, lane);
                else if (live) dst.template store_row<NIN>(row);
            } else {
                if (live) dst.template store_row<NIN>(row);
            }
        }
        if (t == A.k_steps) break;
        // ---- actor forward (rollout_policy_kernel's sequence)
        float xo[L1Q], xr[L1Q];
#pragma unroll
        for (int q = 0; q < L1Q; ++q) {
            const float a0 = d_row(q, 0) < NIN ? row[d_row(q, 0) < NIN ? d_row(q, 0) : 0] : 0.0f;
            const float a1 = d_row(q, 1) < NIN ? row[d_row(q, 1) < NIN ? d_row(q, 1) : 0] : 0.0f;
            xo[q] = h ? a1 : a0;
            if constexpr (EPW == 64) xr[q] = __shfl_xor(h ? a0 : a1, 32, 64);
        }
        float mean[NU];
        if constexpr (EPW == 32) {
            f32x16 h1[LP::NT], h2[LP::NT];
            mlp_forward_tile<NIN, HID, NU, ACT, 16>(lds, xo, h1, h2, mean, lane);
        } else {
            float x[L1Q], out[NU];
            f32x16 h1[LP::NT], h2[LP::NT];
#pragma unroll
            for (int q = 0; q < L1Q; ++q) x[q] = h == 0 ? xo[q] : xr[q];
            mlp_forward_tile<NIN, HID, NU, ACT, 16>(lds, x, h1, h2, out, lane);
#pragma unroll
            for (int a = 0; a < NU; ++a) mean[a] = out[a];
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int q = 0; q < L1Q; ++q) x[q] = h == 1 ? xo[q] : xr[q];
            mlp_forward_tile<NIN, HID, NU, ACT, 16>(lds, x, h1, h2, out, lane);
#pragma unroll
            for (int a = 0; a < NU; ++a) mean[a] = h ? out[a] : mean[a];
        }
        // ---- the policy's action and its log-probability (rollout_policy_kernel's draw)
        T act[NU];
        float logp = logp_const;
        if (A.deterministic) {
#pragma unroll
            for (int a = 0; a < NU; ++a) act[a] = mean[a];
        } else {
            const U4 w = rng_words(key, e.gid, e.episode, (uint32_t)e.step, rng_tag(RNG_CH_POLICY, 0, 0));
            float eps[4];
            {
                const float r0 = m_sqrt(-2.0f * m_log(u01<float>(w.x))), u0 = u01<float>(w.y);
                eps[0] = r0 * cos_2pi(u0);
                eps[1] = r0 * cos_2pi(u0 < 0.25f ? u0 + 0.75f : u0 - 0.25f);
                const float r1 = m_sqrt(-2.0f * m_log(u01<float>(w.z))), u1 = u01<float>(w.w);
                eps[2] = r1 * cos_2pi(u1);
                eps[3] = r1 * cos_2pi(u1 < 0.25f ? u1 + 0.75f : u1 - 0.25f);
            }
#pragma unroll
            for (int a = 0; a < NU; ++a) {
                act[a] = __builtin_fmaf(sigma[a], eps[a], mean[a]);
                logp -= 0.5f * eps[a] * eps[a];
            }
        }
        // ---- the filter: denormalise, certify on the state the policy saw (the observation's first four entries), normalise; an
        // infeasible row applies the policy's own action (base_experiment.py:183-184)
        const size_t tn = (size_t)t * N + i;
        T applied[NU];
        {
            const float u_phys = kcfg.normalized_action ? __fmul_rn((float)kcfg.act_scale, act[0]) : act[0];
            const CbfResult c = cbf_certify(B.p, row, u_phys);
            const float u_norm = kcfg.normalized_action ? __fdiv_rn(c.u, (float)kcfg.act_scale) : c.u;
            applied[0] = c.feasible != 0.0f ? u_norm : act[0];
            if (live) {
                f32x4 v;
                v.x = c.u0; v.y = c.u; v.z = c.s; v.w = c.feasible;
                *reinterpret_cast<f32x4*>(B.rows + 4 * tn) = v;
                B.applied[tn] = applied[0];
            }
        }
        // ---- the control step (identical code to scg_step's kernel)
        const int32_t c0 = e.step;
        T noisy[NU];
        typename Ops::StepResult r = Ops::step(P, goal, e, applied, nullptr, key, i, st, noisy, seq_slot((T*)nullptr, 0), 0);
        if (live) {
#pragma unroll
            for (int a = 0; a < NU; ++a) A.act[tn * NU + a] = act[a];
            A.logp[tn] = logp;
            A.reward[tn] = r.reward;
            A.done[tn] = r.done ? 1 : 0;
            A.flags[tn] = r.flags;
        }
        ep[0] += r.reward; ep[1] += 1.0f; ep[2] += (r.flags & FLAG_VIOLATION) ? 1.0f : 0.0f; ep[3] += r.mse;
        Ops::obs_row(P, goal, st, e, key, c0 + 2, (uint32_t)(c0 + 1), c0, i, nullptr, row);
        if (r.done) {
            if (A.terminal_obs && live) seq_slot(A.terminal_obs + (size_t)t * N * NIN, i, NIN).template store_row<NIN>(row);
            if (A.max_episodes <= 0 || acc[0] < (float)A.max_episodes) {
                acc[0] += 1.0f; acc[1] += ep[0]; acc[2] += ep[1]; acc[3] += ep[2]; acc[4] += ep[3];
            }
            ep[0] = ep[1] = ep[2] = ep[3] = 0.0f;
            if (P.c.auto_reset) {
                dirty = true;
                Ops::reset(P, i, e, key, st);
                Ops::obs_row(P, goal, st, e, key, 1, 0u, 0, i, nullptr, row);
            }
        }
    }
    if (live) {
        if (A.ep_stats) seq_slot(A.ep_stats, i, 4).template store_row<4>(ep);
        if (A.episode_acc) seq_slot(A.episode_acc, i, 8).template store_row<8>(acc);
        Ops::store(P, i, e, dirty);
    }
}
#endif  // cartpole, float32

static int cbf_check_params(const scg_cbf_params* p) {
    for (int i = 0; i < 4; ++i)
        if (!(p->L[i] > 0.0f)) return fail(SCG_ERR_INVALID, "scg_cbf_params: every state limit L[i] must be positive");
    if (!(p->m > 0.0f) || !(p->M > 0.0f) || !(p->l > 0.0f)) return fail(SCG_ERR_INVALID, "scg_cbf_params: m, M and l must be positive");
    if (!(p->lo <= p->hi)) return fail(SCG_ERR_INVALID, "scg_cbf_params: lo must not exceed hi");
    if (!(p->slack_weight >= 0.0f)) return fail(SCG_ERR_INVALID, "scg_cbf_params: slack_weight must not be negative");
    return SCG_OK;
}

}  // namespace scg

extern "C" int scg_cbf_shape(int32_t* hidden, int32_t* activation, int32_t* obs_dim, int32_t* act_dim) {
#ifdef SCG_CBF_ROLLOUT
    if (hidden) *hidden = SCG_POLICY_H;
    if (activation) *activation = SCG_POLICY_ACT;
    if (obs_dim) *obs_dim = scg::scg_make_spec_cfg<float>().nobs;
    if (act_dim) *act_dim = scg::Dims<SCG_SPEC_SYS>::NU;
#else
    if (hidden) *hidden = 0;
    if (activation) *activation = 0;
    if (obs_dim) *obs_dim = 0;
    if (act_dim) *act_dim = 0;
#endif
    return SCG_OK;
}

extern "C" int scg_cbf_certify(scg_env* env, const scg_cbf_params* params, const float* d_state, const float* d_action, float* d_certified,
                               float* d_slack, uint8_t* d_feasible, int n, void* stream) {
    if (!env || !params || !d_state || !d_action || !d_certified || !d_feasible)
        return fail(SCG_ERR_INVALID, "scg_cbf_certify needs env, params, d_state, d_action, d_certified and d_feasible");
#ifdef SCG_CBF_ROLLOUT
    if (n < 0) return fail(SCG_ERR_INVALID, "n must not be negative");
    if ((uintptr_t)d_state & 15) return fail(SCG_ERR_INVALID, "d_state must be 16-byte aligned");
    if (const int rc = scg::cbf_check_params(params)) return rc;
    if (n == 0) return SCG_OK;
    HIP_TRY(hipSetDevice(env->device));
    scg::cbf_certify_kernel<<<dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream>>>(*params, d_state, d_action, d_certified, d_slack,
                                                                                         d_feasible, n);
    HIP_TRY(hipGetLastError());
    return SCG_OK;
#else
    (void)d_slack; (void)n; (void)stream;
    return fail(SCG_ERR_INVALID, "the CBF filter serves float32 cartpole envs");
#endif
}

extern "C" int scg_rollout_cbf(scg_env* env, const scg_actor_ptrs* actor, const scg_cbf_params* params, int deterministic, int k_steps,
                               const scg_policy_rollout* out, float* d_filter_rows, float* d_applied, void* stream) {
    if (!env || !actor || !params || !out) return fail(SCG_ERR_INVALID, "NULL argument to scg_rollout_cbf");
#ifdef SCG_CBF_ROLLOUT
    using namespace scg;
    if (k_steps <= 0) return fail(SCG_ERR_INVALID, "k_steps must be positive");
    if (!env->has_reset) return fail(SCG_ERR_STATE, "scg_reset (all envs) must be called before scg_rollout_cbf");
    if (!actor->W1 || !actor->b1 || !actor->W2 || !actor->b2 || !actor->W3 || !actor->b3 || !actor->logstd)
        return fail(SCG_ERR_INVALID, "the actor has a NULL parameter pointer");
    if (!d_filter_rows || !d_applied || !out->d_obs || !out->d_act || !out->d_logp || !out->d_reward || !out->d_done || !out->d_flags)
        return fail(SCG_ERR_INVALID, "scg_rollout_cbf needs d_filter_rows, d_applied, d_obs, d_act, d_logp, d_reward, d_done and d_flags");
    if (((uintptr_t)out->d_obs | (uintptr_t)out->d_terminal_obs | (uintptr_t)out->d_ep_stats | (uintptr_t)out->d_episode_acc |
         (uintptr_t)d_filter_rows) & 15)
        return fail(SCG_ERR_INVALID, "row outputs and the filter rows must be 16-byte aligned");
    if (const int rc = cbf_check_params(params)) return rc;
    constexpr int nobs = scg_make_spec_cfg<float>().nobs;
    constexpr int NU = Dims<SCG_SPEC_SYS>::NU;
    if (((size_t)env->cfg.num_envs * nobs * sizeof(float)) % 16 != 0)
        return fail(SCG_ERR_INVALID, "num_envs x obs_dim x 4 must be a multiple of 16 (row alignment of the [t]-stacked obs)");
    HIP_TRY(hipSetDevice(env->device));
    PolicyArgs A;
    A.params = nullptr; A.W1 = A.b1 = A.W2 = A.b2 = A.W3 = A.b3 = A.logstd_off = 0;
    A.deterministic = deterministic ? 1 : 0; A.k_steps = k_steps;
    A.obs = (float*)out->d_obs; A.act = (float*)out->d_act; A.logp = (float*)out->d_logp; A.reward = (float*)out->d_reward;
    A.done = out->d_done; A.flags = out->d_flags; A.terminal_obs = (float*)out->d_terminal_obs;
    A.ep_stats = (float*)out->d_ep_stats; A.episode_acc = (float*)out->d_episode_acc; A.max_episodes = out->max_episodes;
    CbfArgs B;
    B.actor = MlpWeights{actor->W1, actor->b1, actor->W2, actor->b2, actor->W3, actor->b3};
    B.logstd = actor->logstd; B.p = *params; B.rows = d_filter_rows; B.applied = d_applied;
    const InstParams<float> I = inst_of<float>(env);
    // launch geometry: scg_rollout_policy's rule and overrides (results do not depend on them)
    int epw = env->cfg.num_envs <= 65536 ? 32 : 64;
    int wpw = env->cfg.num_envs <= 32768 ? 4 : 8;
    if (const char* o = getenv("SCG_ROLLOUT_EPW")) { if (atoi(o) == 32 || atoi(o) == 64) epw = atoi(o); }
    if (const char* o = getenv("SCG_ROLLOUT_WPW")) { if (atoi(o) == 4 || atoi(o) == 8) wpw = atoi(o); }
    const size_t bytes = MlpLds<nobs, SCG_POLICY_H, NU, 16>::END * sizeof(float) + (size_t)wpw * 64 * nobs * sizeof(float);
    const size_t bytes8 = MlpLds<nobs, SCG_POLICY_H, NU, 16>::END * sizeof(float) + (size_t)8 * 64 * nobs * sizeof(float);
    static scg::PerDeviceOnce attr;         // (per device, scg_once.h: the caller has made the handle's device current)
    int attr_dev;
    if (attr.pending(&attr_dev)) {
        HIP_TRY(hipFuncSetAttribute((const void*)rollout_cbf_kernel<64, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes8));
        HIP_TRY(hipFuncSetAttribute((const void*)rollout_cbf_kernel<32, 4>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes8));
        HIP_TRY(hipFuncSetAttribute((const void*)rollout_cbf_kernel<64, 8>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes8));
        HIP_TRY(hipFuncSetAttribute((const void*)rollout_cbf_kernel<32, 8>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes8));
        attr.commit(attr_dev);
    }
    const int per_wg = epw * wpw;
    const dim3 grid((env->cfg.num_envs + per_wg - 1) / per_wg), block(64 * wpw);
    hipStream_t st = (hipStream_t)stream;
    if (epw == 64 && wpw == 4) rollout_cbf_kernel<64, 4><<<grid, block, bytes, st>>>(I, A, B);
    else if (epw == 64) rollout_cbf_kernel<64, 8><<<grid, block, bytes, st>>>(I, A, B);
    else if (wpw == 4) rollout_cbf_kernel<32, 4><<<grid, block, bytes, st>>>(I, A, B);
    else rollout_cbf_kernel<32, 8><<<grid, block, bytes, st>>>(I, A, B);
    HIP_TRY(hipGetLastError());
    return SCG_OK;
#else
    (void)deterministic; (void)k_steps; (void)d_filter_rows; (void)d_applied; (void)stream;
    return fail(SCG_ERR_INVALID, "the CBF filter serves float32 cartpole envs");
#endif
}

// ---- the filter behind the SAC / DDPG actor (scg_rollout_cbf_actor) ---------------------------------------------------------------
#include "scg_actor_rollout.h"
#include "scg_cbf_actor.h"

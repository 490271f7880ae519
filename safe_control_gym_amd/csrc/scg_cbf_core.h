// scg_cbf_core.h — the CBF-QP safety filter (include/scg_cbf.h), one copy for every CBF library: the closed form of the QP as device
// functions (cbf_row: the barrier row; cbf_solve: its minimiser; cbf_certify: their composition; cbf_nn_certify: the row with a learned
// residual added, include/scg_cbf_nn.h), the batched certify kernel, the parameter checks, the filter functor of the SAC / DDPG actor
// rollouts, and the entry points that do not depend on the rollout kernel (scg_cbf_shape, scg_cbf_certify).  Included by scg_cbf.hip,
// scg_cbf_wide.hip and scg_cbf_nn.hip behind the simulator's translation unit; the includer names the actor shape its library was compiled for:
//   SCG_CBF_HIDDEN, SCG_CBF_ACTIVATION     what scg_cbf_shape reports
// The filter serves float32 CartPole configs (SCG_CBF_SERVED); any other library exports the entry points and refuses.
#pragma once

#include "../../include/scg_cbf.h"
#include "scg_mlp.h"                               // (f32x4)

#if !defined(SCG_SPEC) || !defined(SCG_CBF_HIDDEN) || !defined(SCG_CBF_ACTIVATION)
#error "scg_cbf_core.h is included in a specialised build after SCG_CBF_HIDDEN and SCG_CBF_ACTIVATION are defined"
#endif
#if SCG_SPEC_SYS == 0 && SCG_SPEC_DTYPE == 0     // SCG_CARTPOLE, float32
#define SCG_CBF_SERVED 1
#endif

namespace scg {

struct CbfResult { float u0, u, s, feasible; };

struct CbfRow { float k, b; };

// The barrier row of the reference's CBF-QP (include/scg_cbf.h) at one state: r(u) = -k - b u.  Every operation here and in cbf_solve
// is an explicitly rounded float32 one (no contraction), so every kernel that calls them agrees bit for bit.
__device__ __forceinline__ CbfRow cbf_row(const scg_cbf_params& p, const float* X) {
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
    CbfRow r;
    r.k = __fadd_rn(__fmul_rn(p.slope, h), a);
    r.b = b;
    return r;
}

// The closed-form minimiser of the QP with the row (k, b) for one physical action.
__device__ __forceinline__ CbfResult cbf_solve(const scg_cbf_params& p, float k, float b, float u_phys) {
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

// The filter for one (state, physical action): the row, then its minimiser.
__device__ __forceinline__ CbfResult cbf_certify(const scg_cbf_params& p, const float* X, float u_phys) {
    const CbfRow r = cbf_row(p, X);
    return cbf_solve(p, r.k, r.b, u_phys);
}

// The same with a learned correction of the Lie derivative (safety_filters/cbf/cbf_nn.py:104-124): the barrier row becomes
// -slope h - LfV(X, u) - (a_nn u + b_nn) <= s, which is the QP above with k' = k + b_nn and b' = b + a_nn (include/scg_cbf_nn.h).
__device__ __forceinline__ CbfResult cbf_nn_certify(const scg_cbf_params& p, const float* X, float u_phys, float a_nn, float b_nn) {
    const CbfRow r = cbf_row(p, X);
    return cbf_solve(p, __fadd_rn(r.k, b_nn), __fadd_rn(r.b, a_nn), u_phys);
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

// The filter between an action and the env step, and its record: denormalise, certify on the state the policy saw (the observation's
// first four entries), normalise; an infeasible row applies the policy's own action (base_experiment.py:183-184).  A row equals
// scg_cbf_certify of the same state and action bit for bit.  This is the FILTER of rollout_actor_kernel / rollout_actor_wide_kernel
// and the middle of rollout_cbf_kernel.
struct CbfActorFilter {
    scg_cbf_params p;
    float* rows;                                   // [K][N][4]
    float* applied;                                // [K][N]
    template <int NU>
    __device__ __forceinline__ void operator()(const float* row, const float* act, float* out, size_t tn, bool live) const {
        static_assert(NU == 1, "the CBF filter serves the cartpole (one input)");
        constexpr CfgParams<float> kcfg = scg_make_spec_cfg<float>();
        const float u_phys = kcfg.normalized_action ? __fmul_rn((float)kcfg.act_scale, act[0]) : act[0];
        const CbfResult c = cbf_certify(p, row, u_phys);
        const float u_norm = kcfg.normalized_action ? __fdiv_rn(c.u, (float)kcfg.act_scale) : c.u;
        out[0] = c.feasible != 0.0f ? u_norm : act[0];
        if (live) {
            f32x4 v;
            v.x = c.u0; v.y = c.u; v.z = c.s; v.w = c.feasible;
            *reinterpret_cast<f32x4*>(rows + 4 * tn) = v;
            applied[tn] = out[0];
        }
    }
};

static int cbf_check_params(const scg_cbf_params* p) {
    for (int i = 0; i < 4; ++i)
        if (!(p->L[i] > 0.0f)) return fail(SCG_ERR_INVALID, "scg_cbf_params: every state limit L[i] must be positive");
    if (!(p->m > 0.0f) || !(p->M > 0.0f) || !(p->l > 0.0f)) return fail(SCG_ERR_INVALID, "scg_cbf_params: m, M and l must be positive");
    if (!(p->lo <= p->hi)) return fail(SCG_ERR_INVALID, "scg_cbf_params: lo must not exceed hi");
    if (!(p->slack_weight >= 0.0f)) return fail(SCG_ERR_INVALID, "scg_cbf_params: slack_weight must not be negative");
    return SCG_OK;
}

// The filter's own arguments of scg_rollout_cbf_actor, after the actor rollout's checks
static int cbf_actor_filter(const scg_cbf_params* params, float* d_filter_rows, float* d_applied, CbfActorFilter* F) {
    if (!d_filter_rows || !d_applied) return fail(SCG_ERR_INVALID, "scg_rollout_cbf_actor needs d_filter_rows and d_applied");
    if ((uintptr_t)d_filter_rows & 15) return fail(SCG_ERR_INVALID, "the filter rows must be 16-byte aligned");
    if (const int rc = cbf_check_params(params)) return rc;
    F->p = *params; F->rows = d_filter_rows; F->applied = d_applied;
    return SCG_OK;
}

}  // namespace scg

extern "C" int scg_cbf_shape(int32_t* hidden, int32_t* activation, int32_t* obs_dim, int32_t* act_dim) {
#ifdef SCG_CBF_SERVED
    if (hidden) *hidden = SCG_CBF_HIDDEN;
    if (activation) *activation = SCG_CBF_ACTIVATION;
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
#ifdef SCG_CBF_SERVED
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

// scg_cbf_wide.hip — libscg_cbfroll_<spechash>_256_<act>_<sac|ddpg>.so: the CBF-QP safety filter (include/scg_cbf.h) behind the SAC /
// DDPG actor of hidden width 256 (scg_rollout_cbf_actor on rollout_actor_wide_kernel), the batched certify kernel and everything
// libscg_spec_<hash>.so carries.
//
// Built only as   hipcc ... -DSCG_SPEC -include <spec header> -DSCG_ACTOR_WIDE_H=256 -DSCG_ACTOR_WIDE_ACT=<act> -DSCG_ACTOR_WIDE_KIND=<kind> scg_cbf_wide.hip
// (safe_control_gym_amd/_cbf.py, kind given and hidden 256).  scg_cbf.hip cannot be the base of this library: it is built with
// -DSCG_POLICY_H=, which makes the simulator's translation unit instantiate rollout_policy_kernel, and that kernel has no launchable LDS
// image at 256.  So this file includes scg_kernels.hip itself (plain, as scg_actor_rollout_wide.hip does) and carries its own copy of
// the filter's closed form: cbf_certify below is scg_cbf.hip's, operation for operation (every one an explicitly rounded float32 one),
// and tests/test_gpu_rollout_actor_wide.py holds the rows of this library to scg_cbf_certify of a scg_cbf.hip library bit for bit.
// scg_rollout_cbf (PPO's Gaussian actor) is exported and refuses: there is no PPO rollout at 256.
#include "scg_kernels.hip"

#include "../../include/scg_cbf.h"
#include "scg_mlp_rows.h"                          // (f32x4: scg_mlp.h)

#if !defined(SCG_SPEC) || !defined(SCG_ACTOR_WIDE_H)
#error "scg_cbf_wide.hip is built with -DSCG_SPEC -include <spec header> -DSCG_ACTOR_WIDE_H=256 -DSCG_ACTOR_WIDE_ACT= -DSCG_ACTOR_WIDE_KIND="
#endif

namespace scg {

struct CbfResult { float u0, u, s, feasible; };

// The closed-form minimiser of the reference's CBF-QP (include/scg_cbf.h) for one (state, physical action): scg_cbf.hip's cbf_certify.
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

static int cbf_check_params(const scg_cbf_params* p) {
    for (int i = 0; i < 4; ++i)
        if (!(p->L[i] > 0.0f)) return fail(SCG_ERR_INVALID, "scg_cbf_params: every state limit L[i] must be positive");
    if (!(p->m > 0.0f) || !(p->M > 0.0f) || !(p->l > 0.0f)) return fail(SCG_ERR_INVALID, "scg_cbf_params: m, M and l must be positive");
    if (!(p->lo <= p->hi)) return fail(SCG_ERR_INVALID, "scg_cbf_params: lo must not exceed hi");
    if (!(p->slack_weight >= 0.0f)) return fail(SCG_ERR_INVALID, "scg_cbf_params: slack_weight must not be negative");
    return SCG_OK;
}

}  // namespace scg

#if SCG_SPEC_SYS == 0 && SCG_SPEC_DTYPE == 0     // SCG_CARTPOLE, float32
#define SCG_CBF_WIDE 1
#endif

extern "C" int scg_cbf_shape(int32_t* hidden, int32_t* activation, int32_t* obs_dim, int32_t* act_dim) {
#ifdef SCG_CBF_WIDE
    if (hidden) *hidden = SCG_ACTOR_WIDE_H;
    if (activation) *activation = SCG_ACTOR_WIDE_ACT;
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
#ifdef SCG_CBF_WIDE
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
    (void)env; (void)actor; (void)params; (void)deterministic; (void)k_steps; (void)out; (void)d_filter_rows; (void)d_applied; (void)stream;
    return fail(SCG_ERR_INVALID, "scg_rollout_cbf (PPO's actor) is not served at hidden width 256: this library carries scg_rollout_cbf_actor");
}

// ---- the filter behind the SAC / DDPG actor (scg_rollout_cbf_actor) ---------------------------------------------------------------
#include "scg_actor_rollout_wide.h"

#if defined(SCG_CBF_WIDE) && defined(SCG_ACTOR_ROLLOUT_WIDE)
#define SCG_CBF_ACTOR_ROLLOUT_WIDE 1
namespace scg {

// scg_cbf_actor.h's CbfActorFilter: denormalise, certify on the state the policy saw (the observation's first four entries),
// normalise; an infeasible row applies the policy's own action (base_experiment.py:183-184)
struct CbfWideActorFilter {
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

}  // namespace scg
#endif

extern "C" int scg_rollout_cbf_actor(scg_env* env, const scg_actor* actor, const scg_cbf_params* params, int k_steps,
                                     const scg_policy_rollout* out, float* d_filter_rows, float* d_applied, void* stream) {
    if (!env || !actor || !params || !out) return fail(SCG_ERR_INVALID, "NULL argument to scg_rollout_cbf_actor");
#ifdef SCG_CBF_ACTOR_ROLLOUT_WIDE
    if (const int rc = actor_rollout_wide_check("scg_rollout_cbf_actor", env, actor, k_steps, out)) return rc;
    if (!d_filter_rows || !d_applied) return fail(SCG_ERR_INVALID, "scg_rollout_cbf_actor needs d_filter_rows and d_applied");
    if ((uintptr_t)d_filter_rows & 15) return fail(SCG_ERR_INVALID, "the filter rows must be 16-byte aligned");
    if (const int rc = scg::cbf_check_params(params)) return rc;
    scg::CbfWideActorFilter F;
    F.p = *params; F.rows = d_filter_rows; F.applied = d_applied;
    return launch_rollout_actor_wide(env, actor, k_steps, out, F, stream);
#else
    (void)k_steps; (void)d_filter_rows; (void)d_applied; (void)stream;
    return fail(SCG_ERR_INVALID, "scg_rollout_cbf_actor needs a float32 cartpole library compiled for the actor's kind "
                                 "(_cbf.build(cfg, hidden, activation, kind))");
#endif
}

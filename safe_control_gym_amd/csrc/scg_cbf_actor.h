// scg_cbf_actor.h — scg_rollout_cbf_actor (include/scg_cbf.h): the CBF filter behind the SAC / DDPG actor of scg_actor_rollout.h.
// Included at the end of scg_cbf.hip.  rollout_actor_kernel's FILTER hook is CbfActorFilter here: scg_cbf.hip's own cbf_certify device
// function between the head and the env step, with rollout_cbf_kernel's row layout and applied-action rule, so a row equals
// scg_cbf_certify of the same state and action bit for bit.  Built when the library is compiled with -DSCG_POLICY_KIND= for a float32
// CartPole config; scg_rollout_cbf and its kernel are not touched.
#pragma once

#if defined(SCG_CBF_ROLLOUT) && defined(SCG_ACTOR_ROLLOUT)
#define SCG_CBF_ACTOR_ROLLOUT 1
namespace scg {

struct CbfActorFilter {
    scg_cbf_params p;
    float* rows;                                   // [K][N][4]
    float* applied;                                // [K][N]
    // denormalise, certify on the state the policy saw (the observation's first four entries), normalise; an infeasible row applies
    // the policy's own action (base_experiment.py:183-184)
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
#ifdef SCG_CBF_ACTOR_ROLLOUT
    if (const int rc = actor_rollout_check("scg_rollout_cbf_actor", env, actor, k_steps, out)) return rc;
    if (!d_filter_rows || !d_applied) return fail(SCG_ERR_INVALID, "scg_rollout_cbf_actor needs d_filter_rows and d_applied");
    if ((uintptr_t)d_filter_rows & 15) return fail(SCG_ERR_INVALID, "the filter rows must be 16-byte aligned");
    if (const int rc = scg::cbf_check_params(params)) return rc;
    scg::CbfActorFilter F;
    F.p = *params; F.rows = d_filter_rows; F.applied = d_applied;
    return launch_rollout_actor(env, actor, k_steps, out, F, stream);
#else
    (void)k_steps; (void)d_filter_rows; (void)d_applied; (void)stream;
    return fail(SCG_ERR_INVALID, "scg_rollout_cbf_actor needs a float32 cartpole library compiled for the actor's kind "
                                 "(_cbf.build(cfg, hidden, activation, kind))");
#endif
}

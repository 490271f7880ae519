// scg_cbf_actor.h — scg_rollout_cbf_actor (include/scg_cbf.h): the CBF filter behind the SAC / DDPG actor of scg_actor_rollout.h.
// Included at the end of scg_cbf.hip: rollout_actor_kernel with scg_cbf_core.h's CbfActorFilter in its FILTER slot.  Built when the
// library is compiled with -DSCG_POLICY_KIND= for a float32 CartPole config.
#pragma once

extern "C" int scg_rollout_cbf_actor(scg_env* env, const scg_actor* actor, const scg_cbf_params* params, int k_steps,
                                     const scg_policy_rollout* out, float* d_filter_rows, float* d_applied, void* stream) {
    if (!env || !actor || !params || !out) return fail(SCG_ERR_INVALID, "NULL argument to scg_rollout_cbf_actor");
#if defined(SCG_CBF_SERVED) && defined(SCG_ACTOR_ROLLOUT)
    std::string why;
    if (const int rc = actor_rollout_check(&why, "scg_rollout_cbf_actor", env, actor, k_steps, out, SCG_POLICY_H, SCG_POLICY_ACT, SCG_POLICY_KIND))
        return fail(rc, why);
    scg::CbfActorFilter F;
    if (const int rc = scg::cbf_actor_filter(params, d_filter_rows, d_applied, &F)) return rc;
    return launch_rollout_actor(env, actor, k_steps, out, F, stream);
#else
    (void)k_steps; (void)d_filter_rows; (void)d_applied; (void)stream;
    return fail(SCG_ERR_INVALID, "scg_rollout_cbf_actor needs a float32 cartpole library compiled for the actor's kind "
                                 "(_cbf.build(cfg, hidden, activation, kind))");
#endif
}

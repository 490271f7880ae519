// scg_cbf_wide.hip — libscg_cbfroll_<spechash>_256_<act>_<sac|ddpg>.so: the CBF-QP safety filter (include/scg_cbf.h) behind the SAC /
// DDPG actor of hidden width 256 (scg_rollout_cbf_actor on rollout_actor_wide_kernel), the batched certify kernel and everything
// libscg_spec_<hash>.so carries.
//
// Built only as   hipcc ... -DSCG_SPEC -include <spec header> -DSCG_ACTOR_WIDE_H=256 -DSCG_ACTOR_WIDE_ACT=<act> -DSCG_ACTOR_WIDE_KIND=<kind> scg_cbf_wide.hip
// (safe_control_gym_amd/_cbf.py, kind given and hidden 256).  scg_cbf.hip cannot be the base of this library: it is built with
// -DSCG_POLICY_H=, which makes the simulator's translation unit instantiate rollout_policy_kernel, and that kernel has no launchable LDS
// image at 256.  So this file includes scg_kernels.hip itself (plain, as scg_actor_rollout_wide.hip does); the filter is the one copy
// in scg_cbf_core.h, which scg_cbf.hip includes too.  This file adds the wide scg_rollout_cbf_actor; scg_rollout_cbf (PPO's Gaussian
// actor) is exported and refuses: there is no PPO rollout at 256.
#include "scg_kernels.hip"

#if !defined(SCG_SPEC) || !defined(SCG_ACTOR_WIDE_H)
#error "scg_cbf_wide.hip is built with -DSCG_SPEC -include <spec header> -DSCG_ACTOR_WIDE_H=256 -DSCG_ACTOR_WIDE_ACT= -DSCG_ACTOR_WIDE_KIND="
#endif
#define SCG_CBF_HIDDEN SCG_ACTOR_WIDE_H
#define SCG_CBF_ACTIVATION SCG_ACTOR_WIDE_ACT
#include "scg_cbf_core.h"

extern "C" int scg_rollout_cbf(scg_env* env, const scg_actor_ptrs* actor, const scg_cbf_params* params, int deterministic, int k_steps,
                               const scg_policy_rollout* out, float* d_filter_rows, float* d_applied, void* stream) {
    (void)env; (void)actor; (void)params; (void)deterministic; (void)k_steps; (void)out; (void)d_filter_rows; (void)d_applied; (void)stream;
    return fail(SCG_ERR_INVALID, "scg_rollout_cbf (PPO's actor) is not served at hidden width 256: this library carries scg_rollout_cbf_actor");
}

#include "scg_actor_rollout_wide.h"

extern "C" int scg_rollout_cbf_actor(scg_env* env, const scg_actor* actor, const scg_cbf_params* params, int k_steps,
                                     const scg_policy_rollout* out, float* d_filter_rows, float* d_applied, void* stream) {
    if (!env || !actor || !params || !out) return fail(SCG_ERR_INVALID, "NULL argument to scg_rollout_cbf_actor");
#if defined(SCG_CBF_SERVED) && defined(SCG_ACTOR_ROLLOUT_WIDE)
    std::string why;
    if (const int rc = actor_rollout_check(&why, "scg_rollout_cbf_actor", env, actor, k_steps, out, SCG_ACTOR_WIDE_H, SCG_ACTOR_WIDE_ACT, SCG_ACTOR_WIDE_KIND))
        return fail(rc, why);
    scg::CbfActorFilter F;
    if (const int rc = scg::cbf_actor_filter(params, d_filter_rows, d_applied, &F)) return rc;
    return launch_rollout_actor_wide(env, actor, k_steps, out, F, stream);
#else
    (void)k_steps; (void)d_filter_rows; (void)d_applied; (void)stream;
    return fail(SCG_ERR_INVALID, "scg_rollout_cbf_actor needs a float32 cartpole library compiled for the actor's kind "
                                 "(_cbf.build(cfg, hidden, activation, kind))");
#endif
}

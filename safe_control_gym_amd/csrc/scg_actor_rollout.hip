// scg_actor_rollout.hip — libscg_spec_<spechash>_pol<H>_<act>_<sac|ddpg>.so: everything libscg_spec_<hash>_pol<H>_<act>.so carries, plus
// the fused rollout with the deterministic SAC / DDPG actor in the loop (include/scg_actor_rollout.h).
//
// Built only as   hipcc ... -DSCG_SPEC -include <spec header> -DSCG_POLICY_H=<H> -DSCG_POLICY_ACT=<act> -DSCG_POLICY_KIND=<kind> scg_actor_rollout.hip
// (_lib.build_spec(cfg, policy=(hidden, activation, 'sac' | 'ddpg'))).  As in scg_cbf.hip the simulator's translation unit is included
// whole, without any edit to it; the kernel and the entry points are in scg_actor_rollout.h, which scg_cbf.hip includes as well.
#include "scg_kernels.hip"

// kind sac: + the training collector, K vector steps into the replay ring per launch (scg_actor_collect.h, included by scg_actor_rollout.h)
#define SCG_ACTOR_COLLECT 1
#include "scg_actor_rollout.h"

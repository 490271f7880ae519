// scg_actor_rollout_wide.hip — libscg_spec_<spechash>_wide256_<act>_<sac|ddpg>.so: everything libscg_spec_<hash>.so carries, plus the
// fused rollout with the deterministic SAC / DDPG actor of hidden width 256 in the loop (include/scg_actor_rollout.h).
//
// Built only as   hipcc ... -DSCG_SPEC -include <spec header> -DSCG_ACTOR_WIDE_H=256 -DSCG_ACTOR_WIDE_ACT=<act> -DSCG_ACTOR_WIDE_KIND=<kind>
//                 scg_actor_rollout_wide.hip
// (_lib.build_spec(cfg, policy=(256, activation, 'sac' | 'ddpg'))).  The simulator's translation unit is included whole, without any
// edit to it and without -DSCG_POLICY_H=: scg_rollout_policy is exported and refuses.  The kernel and the entry points are in
// scg_actor_rollout_wide.h, which scg_cbf_wide.hip includes as well.
#include "scg_kernels.hip"

#include "scg_actor_rollout_wide.h"

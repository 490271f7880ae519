// scg_actor_rollout.h — scg_rollout_actor (include/scg_actor_rollout.h): the deterministic SAC / DDPG actor inside the env kernel.
// Included by scg_actor_rollout.hip and scg_cbf.hip behind the simulator's translation unit (scg_kernels.hip, which is not edited): the
// libraries built from those two export the entry points; only a build with -DSCG_POLICY_KIND= next to -DSCG_POLICY_H=
// -DSCG_POLICY_ACT= carries the kernel, the others refuse.
//
// rollout_actor_kernel is the shared rollout (scg_rollout_common.h: rollout_policy_kernel's geometries, LDS weight image and forward
// tiles) with its own head: no sampling and no log-probability, the second hidden layer is linear for SAC (ACT2 = MLP_ACT_NONE), and
// the output goes through tanhf and the rescale to [low, high] in the expression scg_sac_act / scg_ddpg_act use.  FILTER is a functor
// between the head and the env step: ActorNoFilter, or the CBF filter of scg_cbf_core.h (one kernel body serves both entry points).
#pragma once

#include "../../include/scg_actor_rollout.h"

#if defined(SCG_SPEC) && defined(SCG_POLICY_H) && defined(SCG_POLICY_KIND)
#if SCG_POLICY_KIND != 1 && SCG_POLICY_KIND != 2
#error "SCG_POLICY_KIND is 1 (SCG_ACTOR_SAC) or 2 (SCG_ACTOR_DDPG)"
#endif
#if SCG_SPEC_DTYPE == 0
#define SCG_ACTOR_ROLLOUT 1
#endif
#endif

#ifdef SCG_ACTOR_ROLLOUT
namespace scg {

struct ActorHead { float low[4], high[4]; };

template <int SYS, bool DIST, int EPW, int WPW, int KIND, typename FILTER>
__global__ __launch_bounds__(64 * WPW) void rollout_actor_kernel(const InstParams<float> I, const PolicyArgs A, const ActorHead B, const FILTER F) {
    using T = float;
    using Ops = EnvOps<SYS, T, DIST, SCG_SEQ_ST_AUX>;
    using D = Dims<SYS>;
    constexpr CfgParams<T> kcfg = scg_make_spec_cfg<T>();
    constexpr int NIN = kcfg.nobs, NU = D::NU, HID = SCG_POLICY_H, ACT = SCG_POLICY_ACT;
    constexpr int ACT2 = KIND == SCG_ACTOR_SAC ? (int)MLP_ACT_NONE : ACT;                 // SAC: the trunk's last layer has no activation
    static_assert(NIN == D::NX || NIN == 2 * D::NX, "the fused rollout serves single-row observations (goal horizon <= 1)");
    using L = MlpLds<NIN, HID, NU, 16>;
    constexpr int L1Q = L::L1Q;
    constexpr bool XPOSE = (NIN * (int)sizeof(T)) % 16 == 0;
    extern __shared__ __align__(16) float lds[];
    unsigned char* const s_obs = reinterpret_cast<unsigned char*>(lds + L::END);       // [WPW waves][64 rows][NIN] transpose scratch
    const PV<T> P{kcfg, I};
    const GoalTab<T> goal{nullptr, I.x_goal, false};
    {
        // SAC: W3 / b3 point at the stacked [2 NU][H] head, whose first NU rows are the mean's: a NOUT = NU image as they are
        const MlpWeights w{A.params + A.W1, A.params + A.b1, A.params + A.W2, A.params + A.b2, A.params + A.W3, A.params + A.b3};
        mlp_fill_lds<NIN, HID, NU, 16, 64 * WPW>(lds, w, threadIdx.x);
    }
    __syncthreads();
    const int N = I.num_envs;
    const RolloutLanes g = rollout_lanes<EPW, WPW>(N);
    const int i = g.i;
    unsigned char* const s_wave = rollout_wave_scratch<NIN>(s_obs);
    const RngKey key{I.key0, I.key1};
    typename Ops::E e;
    float ep[4], acc[8];
    T st[D::NX], row[2 * D::NX];
    bool dirty = false;
    rollout_enter<Ops>(P, goal, key, i, A.ep_stats, A.episode_acc, e, ep, acc, st, row);
    for (int t = 0; t <= A.k_steps; ++t) {
        store_obs_row<XPOSE, NIN>(A.obs + (size_t)t * N * NIN, g, row, s_wave);
        if (t == A.k_steps) break;
        float xo[L1Q], xr[L1Q], u[NU];
        b_operand<NIN, L1Q, EPW>(row, g.h, xo, xr);
        // (inline, not mlp_forward_lanes: through the helper this kernel's 64-envs-per-wave instantiations take 4 more registers)
        if constexpr (EPW == 32) {                                      // both halves hold env c: xo IS the B operand
            f32x16 h1[L::NT], h2[L::NT];
            mlp_forward_tile<NIN, HID, NU, ACT, 16, ACT2>(lds, xo, h1, h2, u, g.lane);
        } else {
            const int h = g.h;
            float x[L1Q], out[NU];
            f32x16 h1[L::NT], h2[L::NT];
#pragma unroll
            for (int q = 0; q < L1Q; ++q) x[q] = h == 0 ? xo[q] : xr[q];                // column tile 0: envs 0..31 of the wave
            mlp_forward_tile<NIN, HID, NU, ACT, 16, ACT2>(lds, x, h1, h2, out, g.lane);
#pragma unroll
            for (int a = 0; a < NU; ++a) u[a] = out[a];
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int q = 0; q < L1Q; ++q) x[q] = h == 1 ? xo[q] : xr[q];                // column tile 1: envs 32..63
            mlp_forward_tile<NIN, HID, NU, ACT, 16, ACT2>(lds, x, h1, h2, out, g.lane);
#pragma unroll
            for (int a = 0; a < NU; ++a) u[a] = h ? out[a] : u[a];
        }
        // ---- the head (sac_utils.py:209-215 deterministic, ddpg_utils.py:141-143): scg_sac_act's / scg_ddpg_act's expression
        T act[NU], applied[NU];
#pragma unroll
        for (int a = 0; a < NU; ++a) act[a] = B.low[a] + 0.5f * (tanhf(u[a]) + 1.0f) * (B.high[a] - B.low[a]);
        const size_t tn = (size_t)t * N + i;
        F.template operator()<NU>(row, act, applied, tn, g.live);
        // ---- the control step (identical code to scg_step's kernel)
        const int32_t c0 = e.step;
        T noisy[NU];
        typename Ops::StepResult r = Ops::step(P, goal, e, applied, nullptr, key, i, st, noisy, seq_slot((T*)nullptr, 0), 0);
        if (g.live) store_step_row<NU, false>(A.act, nullptr, A.reward, A.done, A.flags, tn, act, 0.0f, r);
        after_step<Ops, NIN>(P, goal, key, i, g.live, c0, r, A.terminal_obs, (size_t)t * N * NIN, A.max_episodes, e, ep, acc, st, row, dirty);
    }
    store_tail<Ops>(P, i, g.live, A.ep_stats, A.episode_acc, e, ep, acc, dirty);
}

}  // namespace scg

// The launch; one set of kernel attributes per FILTER and device.
template <typename FILTER>
static int launch_rollout_actor(scg_env* env, const scg_actor* actor, int k_steps, const scg_policy_rollout* out, const FILTER& F, void* stream) {
    HIP_TRY(hipSetDevice(env->device));
    constexpr int S = SCG_SPEC_SYS, KIND = SCG_POLICY_KIND;
    constexpr bool DD = SCG_SPEC_DIST != 0;
    PolicyArgs A = policy_args(actor, out, k_steps, 1);
    A.logp = nullptr;
    ActorHead B;
    for (int j = 0; j < 4; ++j) { B.low[j] = actor->act_low[j]; B.high[j] = actor->act_high[j]; }
    constexpr int nobs = scg_make_spec_cfg<float>().nobs;
    const RolloutGeometry g = rollout_geometry(env->cfg.num_envs);
    constexpr size_t image = MlpLds<nobs, SCG_POLICY_H, Dims<S>::NU, 16>::END * sizeof(float), scratch = 64 * nobs * sizeof(float);
    static void (*const k[4])(InstParams<float>, PolicyArgs, ActorHead, FILTER) = {
        rollout_actor_kernel<S, DD, 64, 4, KIND, FILTER>, rollout_actor_kernel<S, DD, 64, 8, KIND, FILTER>,
        rollout_actor_kernel<S, DD, 32, 4, KIND, FILTER>, rollout_actor_kernel<S, DD, 32, 8, KIND, FILTER>};
    static scg::PerDeviceOnce attr;
    HIP_TRY(launch_rollout(k, attr, (int)(image + 8 * scratch), (int)(image + 8 * scratch), g, env->cfg.num_envs, image + g.wpw * scratch,
                           (hipStream_t)stream, inst_of<float>(env), A, B, F));
    return SCG_OK;
}
#endif  // SCG_ACTOR_ROLLOUT

extern "C" int scg_actor_rollout_shape(int32_t* hidden, int32_t* activation, int32_t* kind) {
#ifdef SCG_ACTOR_ROLLOUT
    if (hidden) *hidden = SCG_POLICY_H;
    if (activation) *activation = SCG_POLICY_ACT;
    if (kind) *kind = SCG_POLICY_KIND;
#else
    if (hidden) *hidden = 0;
    if (activation) *activation = 0;
    if (kind) *kind = 0;
#endif
    return SCG_OK;
}

extern "C" int scg_rollout_actor(scg_env* env, const scg_actor* actor, int k_steps, const scg_policy_rollout* out, void* stream) {
    if (!env || !actor || !out) return fail(SCG_ERR_INVALID, "NULL argument to scg_rollout_actor");
#ifdef SCG_ACTOR_ROLLOUT
    std::string why;
    if (const int rc = actor_rollout_check(&why, "scg_rollout_actor", env, actor, k_steps, out, SCG_POLICY_H, SCG_POLICY_ACT, SCG_POLICY_KIND))
        return fail(rc, why);
    return launch_rollout_actor(env, actor, k_steps, out, scg::ActorNoFilter(), stream);
#else
    (void)k_steps; (void)stream;
    return fail(SCG_ERR_INVALID, "scg_rollout_actor needs a library specialised for the task config and the actor's shape and kind "
                                 "(float32): build it with _lib.build_spec(cfg, policy=(hidden, activation, 'sac' | 'ddpg'))");
#endif
}

// scg_rollout_sac_collect (include/scg_actor_collect.h): SAC's training collection; the kernel only where SCG_ACTOR_COLLECT is defined
#include "scg_actor_collect.h"

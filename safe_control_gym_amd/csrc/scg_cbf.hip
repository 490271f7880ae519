// scg_cbf.hip — libscg_cbfroll_<spechash>_<H>_<act>.so: the CBF-QP safety filter (include/scg_cbf.h) as a batched certify kernel and
// as the policy rollout with the filter between the actor and the env step, next to everything libscg_spec_<hash>.so carries.
//
// Built only as   hipcc ... -DSCG_SPEC -include <spec header> -DSCG_POLICY_H=<H> -DSCG_POLICY_ACT=<act> scg_cbf.hip
// (safe_control_gym_amd/_cbf.py).  The simulator's translation unit is included whole, without any edit to it.  The filter itself is
// scg_cbf_core.h; this file adds rollout_cbf_kernel (PPO's Gaussian actor: the shared rollout pieces of scg_rollout_common.h with the
// filter between the action and the env step) and, through scg_cbf_actor.h, the filter behind the SAC / DDPG actor.  The filter is
// ~60 flops, one sincos and three divisions per env-step beside the ~9 k-flop actor and the engine substeps; its temporaries die
// before the env step, so the kernel keeps rollout_policy_kernel's register class and LDS layout (the actor image + the obs transpose
// scratch) and adds no scratch (DESIGN.md has the numbers).
#include "scg_kernels.hip"

#if !defined(SCG_SPEC) || !defined(SCG_POLICY_H)
#error "scg_cbf.hip is built with -DSCG_SPEC -include <spec header> -DSCG_POLICY_H= -DSCG_POLICY_ACT="
#endif
#define SCG_CBF_HIDDEN SCG_POLICY_H
#define SCG_CBF_ACTIVATION SCG_POLICY_ACT
#include "scg_cbf_core.h"

#ifdef SCG_CBF_SERVED
namespace scg {

struct CbfArgs {
    MlpWeights actor;
    const float* logstd;                           // [NU]
    CbfActorFilter filter;
};

// The LDS layout is rollout_policy_kernel's: the actor image, then the obs transpose scratch.
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
    constexpr bool XPOSE = (NIN * (int)sizeof(T)) % 16 == 0;
    extern __shared__ __align__(16) float lds[];
    unsigned char* const s_obs = reinterpret_cast<unsigned char*>(lds + LP::END);       // [WPW waves][64 rows][NIN] transpose scratch
    const PV<T> P{kcfg, I};
    const GoalTab<T> goal{nullptr, I.x_goal, false};
    mlp_fill_lds<NIN, HID, NU, 16, 64 * WPW>(lds, B.actor, threadIdx.x);
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
    float sigma[NU];
    const float logp_const = gaussian_setup<NU>(B.logstd, sigma);
    for (int t = 0; t <= A.k_steps; ++t) {
        store_obs_row<XPOSE, NIN>(A.obs + (size_t)t * N * NIN, g, row, s_wave);
        if (t == A.k_steps) break;
        float xo[L1Q], xr[L1Q], mean[NU];
        b_operand<NIN, L1Q, EPW>(row, g.h, xo, xr);
        // (inline, not mlp_forward_lanes: through the helper this kernel's 64-envs-per-wave instantiations take 4 more registers)
        if constexpr (EPW == 32) {                                      // both halves hold env c: xo IS the B operand
            f32x16 h1[LP::NT], h2[LP::NT];
            mlp_forward_tile<NIN, HID, NU, ACT, 16>(lds, xo, h1, h2, mean, g.lane);
        } else {
            const int h = g.h;
            float x[L1Q], out[NU];
            f32x16 h1[LP::NT], h2[LP::NT];
#pragma unroll
            for (int q = 0; q < L1Q; ++q) x[q] = h == 0 ? xo[q] : xr[q];                // column tile 0: envs 0..31 of the wave
            mlp_forward_tile<NIN, HID, NU, ACT, 16>(lds, x, h1, h2, out, g.lane);
#pragma unroll
            for (int a = 0; a < NU; ++a) mean[a] = out[a];
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int q = 0; q < L1Q; ++q) x[q] = h == 1 ? xo[q] : xr[q];                // column tile 1: envs 32..63
            mlp_forward_tile<NIN, HID, NU, ACT, 16>(lds, x, h1, h2, out, g.lane);
#pragma unroll
            for (int a = 0; a < NU; ++a) mean[a] = h ? out[a] : mean[a];
        }
        T act[NU], applied[NU];
        const float logp = gaussian_action<NU>(A.deterministic, key, e, RNG_CH_POLICY, sigma, mean, logp_const, act);
        const size_t tn = (size_t)t * N + i;
        B.filter.template operator()<NU>(row, act, applied, tn, g.live);
        // ---- the control step (identical code to scg_step's kernel)
        const int32_t c0 = e.step;
        T noisy[NU];
        typename Ops::StepResult r = Ops::step(P, goal, e, applied, nullptr, key, i, st, noisy, seq_slot((T*)nullptr, 0), 0);
        if (g.live) store_step_row<NU, true>(A.act, A.logp, A.reward, A.done, A.flags, tn, act, logp, r);
        after_step<Ops, NIN>(P, goal, key, i, g.live, c0, r, A.terminal_obs, (size_t)t * N * NIN, A.max_episodes, e, ep, acc, st, row, dirty);
    }
    store_tail<Ops>(P, i, g.live, A.ep_stats, A.episode_acc, e, ep, acc, dirty);
}

}  // namespace scg
#endif  // SCG_CBF_SERVED

extern "C" int scg_rollout_cbf(scg_env* env, const scg_actor_ptrs* actor, const scg_cbf_params* params, int deterministic, int k_steps,
                               const scg_policy_rollout* out, float* d_filter_rows, float* d_applied, void* stream) {
    if (!env || !actor || !params || !out) return fail(SCG_ERR_INVALID, "NULL argument to scg_rollout_cbf");
#ifdef SCG_CBF_SERVED
    using namespace scg;
    if (k_steps <= 0) return fail(SCG_ERR_INVALID, "k_steps must be positive");
    if (!env->has_reset) return fail(SCG_ERR_STATE, "scg_reset (all envs) must be called before scg_rollout_cbf");
    if (!actor->W1 || !actor->b1 || !actor->W2 || !actor->b2 || !actor->W3 || !actor->b3 || !actor->logstd)
        return fail(SCG_ERR_INVALID, "the actor has a NULL parameter pointer");
    if (!d_filter_rows || !d_applied || !rollout_outputs_present(out, true))
        return fail(SCG_ERR_INVALID, "scg_rollout_cbf needs d_filter_rows, d_applied, d_obs, d_act, d_logp, d_reward, d_done and d_flags");
    if (!rollout_rows_aligned(out, (uintptr_t)d_filter_rows))
        return fail(SCG_ERR_INVALID, "row outputs and the filter rows must be 16-byte aligned");
    if (const int rc = cbf_check_params(params)) return rc;
    constexpr int nobs = scg_make_spec_cfg<float>().nobs;
    constexpr int NU = Dims<SCG_SPEC_SYS>::NU;
    if (const char* why = rollout_obs_stack_error(true, env->cfg.num_envs, nobs)) return fail(SCG_ERR_INVALID, why);
    HIP_TRY(hipSetDevice(env->device));
    const PolicyArgs A = policy_args(out, k_steps, deterministic ? 1 : 0);
    CbfArgs B;
    B.actor = MlpWeights{actor->W1, actor->b1, actor->W2, actor->b2, actor->W3, actor->b3};
    B.logstd = actor->logstd; B.filter.p = *params; B.filter.rows = d_filter_rows; B.filter.applied = d_applied;
    const RolloutGeometry g = rollout_geometry(env->cfg.num_envs);
    constexpr size_t image = MlpLds<nobs, SCG_POLICY_H, NU, 16>::END * sizeof(float), scratch = 64 * nobs * sizeof(float);
    static void (*const k[4])(InstParams<float>, PolicyArgs, CbfArgs) = {rollout_cbf_kernel<64, 4>, rollout_cbf_kernel<64, 8>,
                                                                        rollout_cbf_kernel<32, 4>, rollout_cbf_kernel<32, 8>};
    static PerDeviceOnce attr;
    HIP_TRY(launch_rollout(k, attr, (int)(image + 8 * scratch), (int)(image + 8 * scratch), g, env->cfg.num_envs, image + g.wpw * scratch,
                           (hipStream_t)stream, inst_of<float>(env), A, B));
    return SCG_OK;
#else
    (void)deterministic; (void)k_steps; (void)d_filter_rows; (void)d_applied; (void)stream;
    return fail(SCG_ERR_INVALID, "the CBF filter serves float32 cartpole envs");
#endif
}

// ---- the filter behind the SAC / DDPG actor (scg_rollout_cbf_actor) ---------------------------------------------------------------
#include "scg_actor_rollout.h"
#include "scg_cbf_actor.h"

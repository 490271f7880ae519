// scg_actor_rollout.h — scg_rollout_actor (include/scg_actor_rollout.h): the deterministic SAC / DDPG actor inside the env kernel.
// Included by scg_actor_rollout.hip and scg_cbf.hip behind the simulator's translation unit (scg_kernels.hip, which is not edited): the
// libraries built from those two export the entry points; only a build with -DSCG_POLICY_KIND= next to -DSCG_POLICY_H=
// -DSCG_POLICY_ACT= carries the kernel, the others refuse.
//
// rollout_actor_kernel follows rollout_policy_kernel (scg_env_kernels.h) step for step: the same EPW / WPW geometries, the same LDS
// weight image (MlpLds<NIN, HID, NU, 16>) and forward tile, the same EnvOps::step, auto-reset, terminal observation, ep_stats and
// episode_acc, the same obs-row stores.  What differs is the head: no sampling and no log-probability, the second hidden layer is
// linear for SAC (mlp_forward_tile's ACT2 = MLP_ACT_NONE), and the output goes through tanhf and the rescale to [low, high] in the
// expression scg_sac_act / scg_ddpg_act use.  FILTER is a functor between the head and the env step: ActorNoFilter here, the CBF
// filter in scg_cbf_actor.h (one kernel body serves both entry points).
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

// The action the env step receives is the actor's own; nothing is recorded.
struct ActorNoFilter {
    template <int NU>
    __device__ __forceinline__ void operator()(const float*, const float* act, float* applied, size_t, bool) const {
#pragma unroll
        for (int a = 0; a < NU; ++a) applied[a] = act[a];
    }
};

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
    // observation of the current state (what the previous step / reset returned)
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
            if constexpr ((NIN * (int)sizeof(T)) % 16 == 0) {              // 16-byte rows leave through the LDS transpose (as in step_kernel)
                if (full_wave) store_rows_coalesced<T, NIN>(dst, row, s_wave, lane);
                else if (live) dst.template store_row<NIN>(row);
            } else {                                                       // e.g. 6-float rows (Quadrotor2D stabilisation)
                if (live) dst.template store_row<NIN>(row);
            }
        }
        if (t == A.k_steps) break;
        // ---- actor forward for the wave's two 32-env column tiles (lane (c, h) owns env 32 h + c of the wave)
        float xo[L1Q], xr[L1Q];
#pragma unroll
        for (int q = 0; q < L1Q; ++q) {
            const float a0 = d_row(q, 0) < NIN ? row[d_row(q, 0) < NIN ? d_row(q, 0) : 0] : 0.0f;
            const float a1 = d_row(q, 1) < NIN ? row[d_row(q, 1) < NIN ? d_row(q, 1) : 0] : 0.0f;
            xo[q] = h ? a1 : a0;                                        // my own env's rows row(q, h)
            if constexpr (EPW == 64) xr[q] = __shfl_xor(h ? a0 : a1, 32, 64);      // the partner env's rows row(q, h)
        }
        float u[NU];
        if constexpr (EPW == 32) {                                      // both halves hold env c: xo IS the B operand
            f32x16 h1[L::NT], h2[L::NT];
            mlp_forward_tile<NIN, HID, NU, ACT, 16, ACT2>(lds, xo, h1, h2, u, lane);
        } else {
            float x[L1Q], out[NU];
            f32x16 h1[L::NT], h2[L::NT];
#pragma unroll
            for (int q = 0; q < L1Q; ++q) x[q] = h == 0 ? xo[q] : xr[q];                // column tile 0: envs 0..31 of the wave
            mlp_forward_tile<NIN, HID, NU, ACT, 16, ACT2>(lds, x, h1, h2, out, lane);
#pragma unroll
            for (int a = 0; a < NU; ++a) u[a] = out[a];
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int q = 0; q < L1Q; ++q) x[q] = h == 1 ? xo[q] : xr[q];                // column tile 1: envs 32..63
            mlp_forward_tile<NIN, HID, NU, ACT, 16, ACT2>(lds, x, h1, h2, out, lane);
#pragma unroll
            for (int a = 0; a < NU; ++a) u[a] = h ? out[a] : u[a];
        }
        // ---- the head (sac_utils.py:209-215 deterministic, ddpg_utils.py:141-143): scg_sac_act's / scg_ddpg_act's expression
        T act[NU], applied[NU];
#pragma unroll
        for (int a = 0; a < NU; ++a) act[a] = B.low[a] + 0.5f * (tanhf(u[a]) + 1.0f) * (B.high[a] - B.low[a]);
        const size_t tn = (size_t)t * N + i;
        F.template operator()<NU>(row, act, applied, tn, live);
        // ---- the control step (identical code to scg_step's kernel)
        const int32_t c0 = e.step;
        T noisy[NU];
        typename Ops::StepResult r = Ops::step(P, goal, e, applied, nullptr, key, i, st, noisy, seq_slot((T*)nullptr, 0), 0);
        if (live) {
#pragma unroll
            for (int a = 0; a < NU; ++a) A.act[tn * NU + a] = act[a];
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

}  // namespace scg

// Argument checks shared by scg_rollout_actor and scg_rollout_cbf_actor; nothing is launched when one fails.
static int actor_rollout_check(const char* who, const scg_env* env, const scg_actor* actor, int k_steps, const scg_policy_rollout* out) {
    const std::string w(who);
    if (k_steps <= 0) return fail(SCG_ERR_INVALID, "k_steps must be positive");
    if (!env->has_reset) return fail(SCG_ERR_STATE, "scg_reset (all envs) must be called before " + w);
    if (actor->hidden != SCG_POLICY_H || actor->activation != SCG_POLICY_ACT || actor->kind != SCG_POLICY_KIND)
        return fail(SCG_ERR_INVALID, "this library was compiled for another actor shape (hidden / activation / kind)");
    if (!actor->d_params || !out->d_obs || !out->d_act || !out->d_reward || !out->d_done || !out->d_flags)
        return fail(SCG_ERR_INVALID, w + " needs d_params, d_obs, d_act, d_reward, d_done and d_flags");
    if (((uintptr_t)out->d_obs | (uintptr_t)out->d_terminal_obs | (uintptr_t)out->d_ep_stats | (uintptr_t)out->d_episode_acc) & 15)
        return fail(SCG_ERR_INVALID, "row outputs must be 16-byte aligned");
    if constexpr ((scg_make_spec_cfg<float>().nobs * sizeof(float)) % 16 == 0) {      // rows leave as 16-byte pieces: obs[t] must stay aligned
        if (((size_t)env->cfg.num_envs * scg_make_spec_cfg<float>().nobs * sizeof(float)) % 16 != 0)
            return fail(SCG_ERR_INVALID, "num_envs x obs_dim x 4 must be a multiple of 16 (row alignment of the [t]-stacked obs)");
    }
    return SCG_OK;
}

// The launch, scg_rollout_policy's geometry rule and overrides; one set of kernel attributes per FILTER and device.
template <typename FILTER>
static int launch_rollout_actor(scg_env* env, const scg_actor* actor, int k_steps, const scg_policy_rollout* out, const FILTER& F, void* stream) {
    HIP_TRY(hipSetDevice(env->device));
    constexpr int S = SCG_SPEC_SYS, KIND = SCG_POLICY_KIND;
    constexpr bool DD = SCG_SPEC_DIST != 0;
    PolicyArgs A;
    A.params = actor->d_params; A.W1 = actor->W1; A.b1 = actor->b1; A.W2 = actor->W2; A.b2 = actor->b2; A.W3 = actor->W3; A.b3 = actor->b3;
    A.logstd_off = 0; A.deterministic = 1; A.k_steps = k_steps;
    A.obs = (float*)out->d_obs; A.act = (float*)out->d_act; A.logp = nullptr; A.reward = (float*)out->d_reward;
    A.done = out->d_done; A.flags = out->d_flags; A.terminal_obs = (float*)out->d_terminal_obs;
    A.ep_stats = (float*)out->d_ep_stats; A.episode_acc = (float*)out->d_episode_acc; A.max_episodes = out->max_episodes;
    ActorHead B;
    for (int j = 0; j < 4; ++j) { B.low[j] = actor->act_low[j]; B.high[j] = actor->act_high[j]; }
    const InstParams<float> I = inst_of<float>(env);
    constexpr int nobs = scg_make_spec_cfg<float>().nobs;
    int epw = env->cfg.num_envs <= 65536 ? 32 : 64;
    int wpw = env->cfg.num_envs <= 32768 ? 4 : 8;
    if (const char* o = getenv("SCG_ROLLOUT_EPW")) { if (atoi(o) == 32 || atoi(o) == 64) epw = atoi(o); }
    if (const char* o = getenv("SCG_ROLLOUT_WPW")) { if (atoi(o) == 4 || atoi(o) == 8) wpw = atoi(o); }
    const size_t bytes = MlpLds<nobs, SCG_POLICY_H, Dims<S>::NU, 16>::END * sizeof(float) + (size_t)wpw * 64 * nobs * sizeof(float);
    const size_t bytes8 = MlpLds<nobs, SCG_POLICY_H, Dims<S>::NU, 16>::END * sizeof(float) + (size_t)8 * 64 * nobs * sizeof(float);
    static scg::PerDeviceOnce attr;         // (per device, scg_once.h: the caller has made the handle's device current)
    int attr_dev;
    if (attr.pending(&attr_dev)) {
        HIP_TRY(hipFuncSetAttribute((const void*)rollout_actor_kernel<S, DD, 64, 4, KIND, FILTER>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes8));
        HIP_TRY(hipFuncSetAttribute((const void*)rollout_actor_kernel<S, DD, 32, 4, KIND, FILTER>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes8));
        HIP_TRY(hipFuncSetAttribute((const void*)rollout_actor_kernel<S, DD, 64, 8, KIND, FILTER>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes8));
        HIP_TRY(hipFuncSetAttribute((const void*)rollout_actor_kernel<S, DD, 32, 8, KIND, FILTER>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes8));
        attr.commit(attr_dev);
    }
    const int per_wg = epw * wpw;
    const dim3 grid((env->cfg.num_envs + per_wg - 1) / per_wg), block(64 * wpw);
    hipStream_t st = (hipStream_t)stream;
    if (epw == 64 && wpw == 4) rollout_actor_kernel<S, DD, 64, 4, KIND, FILTER><<<grid, block, bytes, st>>>(I, A, B, F);
    else if (epw == 64) rollout_actor_kernel<S, DD, 64, 8, KIND, FILTER><<<grid, block, bytes, st>>>(I, A, B, F);
    else if (wpw == 4) rollout_actor_kernel<S, DD, 32, 4, KIND, FILTER><<<grid, block, bytes, st>>>(I, A, B, F);
    else rollout_actor_kernel<S, DD, 32, 8, KIND, FILTER><<<grid, block, bytes, st>>>(I, A, B, F);
    HIP_TRY(hipGetLastError());
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
    if (const int rc = actor_rollout_check("scg_rollout_actor", env, actor, k_steps, out)) return rc;
    return launch_rollout_actor(env, actor, k_steps, out, scg::ActorNoFilter(), stream);
#else
    (void)k_steps; (void)stream;
    return fail(SCG_ERR_INVALID, "scg_rollout_actor needs a library specialised for the task config and the actor's shape and kind "
                                 "(float32): build it with _lib.build_spec(cfg, policy=(hidden, activation, 'sac' | 'ddpg'))");
#endif
}

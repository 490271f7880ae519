// scg_actor_rollout_wide.h — scg_rollout_actor (include/scg_actor_rollout.h) at hidden width 256: the deterministic SAC / DDPG actor
// inside the env kernel with layer 2 in registers (scg_mlp_rows.h).  Included by scg_actor_rollout_wide.hip and scg_cbf_wide.hip behind
// the simulator's translation unit (scg_kernels.hip, which is not edited).  A wide library is built with -DSCG_ACTOR_WIDE_H=256
// -DSCG_ACTOR_WIDE_ACT= -DSCG_ACTOR_WIDE_KIND= and WITHOUT -DSCG_POLICY_H=, so scg_kernels.hip compiles as in a plain specialised
// library: rollout_policy_kernel (whose LDS image cannot be launched at 256) is not instantiated and scg_rollout_policy refuses.
//
// rollout_actor_wide_kernel is rollout_actor_kernel's loop (scg_actor_rollout.h) with another forward pass and the stepper-wave
// geometry; the head expression and the FILTER slot are the narrow kernel's.  It keeps its own text for the entry, the block after
// the env step and the tail (inside `if (stepper)` the shared pieces of scg_rollout_common.h cost some instantiations 2 registers);
// the no-filter functor, the argument checks and PolicyArgs-free host helpers are the shared ones.
// Geometry: 8 waves per workgroup, G column tiles; wave w < G steps the 32 envs of tile w in the EPW = 32 lane mapping (both lane
// halves hold env c, half 0 stores), all 8 waves take part in every tile's forward pass.  The waves
// w >= G (G = 1: seven of eight) hold their rows of W2 and otherwise only run the forward pass.  A surplus tile (a ragged last
// workgroup) shadows the last env, takes part in barriers and MFMAs and stores nothing; every barrier is reached by all 512 threads
// on every step (k_steps is a kernel argument).  Since no wave holds 64 envs, obs rows never leave through the LDS transpose: there
// is no transpose scratch in this kernel's LDS.
#pragma once

#include "../../include/scg_actor_rollout.h"
#include "scg_mlp_rows.h"
#include "scg_rollout_common.h"

#if defined(SCG_SPEC) && defined(SCG_ACTOR_WIDE_H)
#if defined(SCG_POLICY_H)
#error "a wide actor library is built without -DSCG_POLICY_H= (rollout_policy_kernel has no launchable LDS image at 256)"
#endif
#if SCG_ACTOR_WIDE_H != 256
#error "SCG_ACTOR_WIDE_H is 256"
#endif
#if SCG_ACTOR_WIDE_KIND != 1 && SCG_ACTOR_WIDE_KIND != 2
#error "SCG_ACTOR_WIDE_KIND is 1 (SCG_ACTOR_SAC) or 2 (SCG_ACTOR_DDPG)"
#endif
#if SCG_SPEC_DTYPE == 0
#define SCG_ACTOR_ROLLOUT_WIDE 1
#endif
#endif

#ifdef SCG_ACTOR_ROLLOUT_WIDE
namespace scg {

struct WideActorArgs {
    const float* params; int32_t W1, b1, W2, b2, W3, b3;
    int32_t k_steps;
    float* obs; float* act; float* reward; uint8_t* done; uint8_t* flags; float* terminal_obs;
    float* ep_stats; float* episode_acc; int32_t max_episodes;
    float low[4], high[4];
};

template <int SYS, bool DIST, int G, int KIND, typename FILTER>
__global__ __launch_bounds__(64 * MLP_ROWS_WAVES) void rollout_actor_wide_kernel(const InstParams<float> I, const WideActorArgs A, const FILTER F) {
    using T = float;
    using Ops = EnvOps<SYS, T, DIST, SCG_SEQ_ST_AUX>;
    using D = Dims<SYS>;
    constexpr CfgParams<T> kcfg = scg_make_spec_cfg<T>();
    constexpr int NIN = kcfg.nobs, NU = D::NU, ACT = SCG_ACTOR_WIDE_ACT;
    constexpr int ACT2 = KIND == SCG_ACTOR_SAC ? (int)MLP_ACT_NONE : ACT;                 // SAC: the trunk's last layer has no activation
    static_assert(NIN == D::NX || NIN == 2 * D::NX, "the fused rollout serves single-row observations (goal horizon <= 1)");
    using L = MlpRowsLds<NIN, NU, G>;
    constexpr int L1Q = L::L1Q;
    extern __shared__ __align__(16) float lds[];
    const PV<T> P{kcfg, I};
    const GoalTab<T> goal{nullptr, I.x_goal, false};
    const int lane = threadIdx.x & 63, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float w2[MLP_ROWS_WAVES][16];
    {
        // SAC: W3 / b3 point at the stacked [2 NU][H] head, whose first NU rows are the mean's: a NOUT = NU image as they are
        const MlpWeights w{A.params + A.W1, A.params + A.b1, A.params + A.W2, A.params + A.b2, A.params + A.W3, A.params + A.b3};
        mlp_rows_load_w2(w.W2, wave, lane, w2);
        mlp_rows_fill_lds<NIN, NU, G>(lds, w, threadIdx.x);
    }
    __syncthreads();
    const int N = I.num_envs;
    const bool stepper = wave < G;                    // this wave steps the 32 envs of column tile `wave`
    const int i0 = (blockIdx.x * G + (stepper ? wave : 0)) * 32 + (lane & 31);
    const bool live = stepper && i0 < N && h == 0;
    const int i = i0 < N ? i0 : N - 1;                // surplus lanes shadow the last env (they take part in the MFMAs, never store)
    typename Ops::E e;
    const RngKey key{I.key0, I.key1};
    float ep[4] = {0.0f, 0.0f, 0.0f, 0.0f}, acc[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    T st[D::NX], row[2 * D::NX] = {};
    if (stepper) {                                    // (wave-uniform; the waves w >= G hold no env: nothing to load, no row to form)
        Ops::load_state(P, i, e);
        Ops::load_params(P, i, e);
        if (A.ep_stats) seq_slot(A.ep_stats, i, 4).template load_row<4>(ep);
        if (A.episode_acc) seq_slot(A.episode_acc, i, 8).template load_row<8>(acc);
        // observation of the current state (what the previous step / reset returned)
        Ops::state_vector(e, st);
        const bool fresh = e.step == 0;
        const int32_t c0 = e.step - 1;
        Ops::obs_row(P, goal, st, e, key, fresh ? 1 : c0 + 2, fresh ? 0u : (uint32_t)(c0 + 1), fresh ? 0 : c0, i, nullptr, row);
    }
    bool dirty = false;
    for (int t = 0; t <= A.k_steps; ++t) {
        // ---- rollout row obs[t]
        if (live) seq_slot(A.obs + (size_t)t * N * NIN, i, NIN).template store_row<NIN>(row);
        if (t == A.k_steps) break;
        // ---- actor forward: both lane halves hold env c, so the rows row(q, h) ARE the B operand of layer 1
        float xo[L1Q], u[NU];
#pragma unroll
        for (int q = 0; q < L1Q; ++q) {
            const float a0 = d_row(q, 0) < NIN ? row[d_row(q, 0) < NIN ? d_row(q, 0) : 0] : 0.0f;
            const float a1 = d_row(q, 1) < NIN ? row[d_row(q, 1) < NIN ? d_row(q, 1) : 0] : 0.0f;
            xo[q] = h ? a1 : a0;
        }
        mlp_rows_forward<NIN, NU, ACT, ACT2, G>(lds, w2, xo, u, wave, lane);
        if (!stepper) continue;                       // (wave-uniform; no barrier below)
        // ---- the head (sac_utils.py:209-215 deterministic, ddpg_utils.py:141-143): scg_sac_act's / scg_ddpg_act's expression
        T act[NU], applied[NU];
#pragma unroll
        for (int a = 0; a < NU; ++a) act[a] = A.low[a] + 0.5f * (tanhf(u[a]) + 1.0f) * (A.high[a] - A.low[a]);
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

// Column tiles per workgroup.  G = 1 (32 envs per workgroup, 8 waves on one tile's layer 2) has the shorter step; G = 8 (256 envs per
// workgroup) the throughput.  Measured on MI355X (profiles/actor_rollout_wide_cost.json): a 250-step evaluation with
// G = 1 takes 4.1-4.3 ms up to 8 192 envs (256 workgroups, one per CU) and doubles with every further 8 192, with G = 8 a flat 20.0-20.8 ms
// up to 65 536; G = 1 wins at 32 768 (15.3 against 20.3 ms), G = 8 at 65 536 (20.8 against 30.1 ms): the rule switches at the largest size
// measured in G = 1's favour.
// SCG_ROLLOUT_WIDE_TILES=1|8 overrides it (measurement only: results do not depend on it).
constexpr int SCG_WIDE_G1_MAX_ENVS = 32768;
static int actor_wide_tiles(int num_envs) {
    int g = num_envs <= SCG_WIDE_G1_MAX_ENVS ? 1 : 8;
    if (const char* o = getenv("SCG_ROLLOUT_WIDE_TILES")) { if (atoi(o) == 1 || atoi(o) == 8) g = atoi(o); }
    return g;
}

template <typename FILTER>
static int launch_rollout_actor_wide(scg_env* env, const scg_actor* actor, int k_steps, const scg_policy_rollout* out, const FILTER& F, void* stream) {
    HIP_TRY(hipSetDevice(env->device));
    constexpr int S = SCG_SPEC_SYS, KIND = SCG_ACTOR_WIDE_KIND;
    constexpr bool DD = SCG_SPEC_DIST != 0;
    constexpr int nobs = scg_make_spec_cfg<float>().nobs, NU = Dims<S>::NU;
    WideActorArgs A;
    A.params = actor->d_params; A.W1 = actor->W1; A.b1 = actor->b1; A.W2 = actor->W2; A.b2 = actor->b2; A.W3 = actor->W3; A.b3 = actor->b3;
    A.k_steps = k_steps;
    A.obs = (float*)out->d_obs; A.act = (float*)out->d_act; A.reward = (float*)out->d_reward;
    A.done = out->d_done; A.flags = out->d_flags; A.terminal_obs = (float*)out->d_terminal_obs;
    A.ep_stats = (float*)out->d_ep_stats; A.episode_acc = (float*)out->d_episode_acc; A.max_episodes = out->max_episodes;
    for (int j = 0; j < 4; ++j) { A.low[j] = actor->act_low[j]; A.high[j] = actor->act_high[j]; }
    hipStream_t st = (hipStream_t)stream;
    const InstParams<float> I = inst_of<float>(env);
    constexpr size_t bytes1 = MlpRowsLds<nobs, NU, 1>::END * sizeof(float), bytes8 = MlpRowsLds<nobs, NU, 8>::END * sizeof(float);
    static scg::PerDeviceOnce attr;         // (per device, scg_once.h: the caller has made the handle's device current)
    int attr_dev;
    if (attr.pending(&attr_dev)) {
        HIP_TRY(hipFuncSetAttribute((const void*)rollout_actor_wide_kernel<S, DD, 1, KIND, FILTER>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes1));
        HIP_TRY(hipFuncSetAttribute((const void*)rollout_actor_wide_kernel<S, DD, 8, KIND, FILTER>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes8));
        attr.commit(attr_dev);
    }
    const int g = actor_wide_tiles(env->cfg.num_envs), per_wg = 32 * g;
    const dim3 grid((env->cfg.num_envs + per_wg - 1) / per_wg), block(64 * MLP_ROWS_WAVES);
    if (g == 1) rollout_actor_wide_kernel<S, DD, 1, KIND, FILTER><<<grid, block, bytes1, st>>>(I, A, F);
    else rollout_actor_wide_kernel<S, DD, 8, KIND, FILTER><<<grid, block, bytes8, st>>>(I, A, F);
    HIP_TRY(hipGetLastError());
    return SCG_OK;
}
#endif  // SCG_ACTOR_ROLLOUT_WIDE

extern "C" int scg_actor_rollout_shape(int32_t* hidden, int32_t* activation, int32_t* kind) {
#ifdef SCG_ACTOR_ROLLOUT_WIDE
    if (hidden) *hidden = SCG_ACTOR_WIDE_H;
    if (activation) *activation = SCG_ACTOR_WIDE_ACT;
    if (kind) *kind = SCG_ACTOR_WIDE_KIND;
#else
    if (hidden) *hidden = 0;
    if (activation) *activation = 0;
    if (kind) *kind = 0;
#endif
    return SCG_OK;
}

extern "C" int scg_rollout_actor(scg_env* env, const scg_actor* actor, int k_steps, const scg_policy_rollout* out, void* stream) {
    if (!env || !actor || !out) return fail(SCG_ERR_INVALID, "NULL argument to scg_rollout_actor");
#ifdef SCG_ACTOR_ROLLOUT_WIDE
    std::string why;
    if (const int rc = actor_rollout_check(&why, "scg_rollout_actor", env, actor, k_steps, out, SCG_ACTOR_WIDE_H, SCG_ACTOR_WIDE_ACT, SCG_ACTOR_WIDE_KIND))
        return fail(rc, why);
    return launch_rollout_actor_wide(env, actor, k_steps, out, scg::ActorNoFilter(), stream);
#else
    (void)k_steps; (void)stream;
    return fail(SCG_ERR_INVALID, "scg_rollout_actor at width 256 needs a float32 library built with -DSCG_ACTOR_WIDE_H=256 "
                                 "(_lib.build_spec(cfg, policy=(256, activation, 'sac' | 'ddpg')))");
#endif
}

// scg_rollout_sac_collect (include/scg_actor_collect.h) is exported and refuses: the collector has no width 256
#include "scg_actor_collect.h"

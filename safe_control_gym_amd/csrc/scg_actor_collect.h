// scg_actor_collect.h — scg_rollout_sac_collect (include/scg_actor_collect.h): SAC's training collection, K vector steps into the replay
// ring per launch.  Included at the end of scg_actor_rollout.h and scg_actor_rollout_wide.h, so every library that exports
// scg_rollout_actor exports the entry point; the kernel is carried only by a translation unit that defines SCG_ACTOR_COLLECT in front
// of a float32 build of kind sac (scg_actor_rollout.hip), every other one refuses.
//
// sac_collect_kernel is the shared rollout (scg_rollout_common.h: geometries, rollout_enter, store_obs_row, b_operand,
// mlp_forward_lanes, normal4, store_step_row, store_tail) with
//   - the whole stacked head (NOUT = 2 NU: mean rows, then log_std rows) in the LDS image, and scg_sac_sample's expression behind it;
//   - the warm-up's uniform action instead, on a kernel-uniform branch (no weight image is filled then);
//   - its own text after the env step, because the ring's next-observation row is the TERMINAL observation for a truncated env and the
//     post-reset one otherwise: the terminal row waits in the lane's own piece of the wave's transpose scratch while the reset
//     redraws the episode (held in registers it would be a second observation row per lane across the reset);
//   - ring rows (pos0 + t N + i) mod capacity: consecutive envs are consecutive rows unless the ring wraps inside the wave, so 16-byte
//     rows of a full wave leave through store_rows_coalesced exactly as obs[t] does, and row by row otherwise.
// The ring's counters are read here by everybody and advanced by the one-thread launch behind it (as ring_advance_kernel, scg_sac.hip).
#pragma once

#include "../../include/scg_actor_collect.h"

#if defined(SCG_ACTOR_ROLLOUT) && defined(SCG_ACTOR_COLLECT)
#if SCG_POLICY_KIND == 1
#define SCG_ACTOR_COLLECT_KERNEL 1
#endif
#endif

#ifdef SCG_ACTOR_COLLECT_KERNEL
namespace scg {

struct CollectRing {
    float* obs; float* act; float* rew; float* next_obs; float* mask; uint32_t capacity;
    long long* pos; float* size_f; int32_t* size_i;
    float* cur_obs; int32_t uniform;
};

// Row `rr` of a ring array of NROW-float rows.  contig (wave-uniform): the wave's 64 rows are consecutive in memory.
template <bool XPOSE, int NROW>
__device__ __forceinline__ void store_ring_row(float* base, uint32_t rr, bool contig, bool live, const float* x, unsigned char* s_wave, int lane) {
    const Slot<float, SCG_SEQ_ST_AUX> dst = seq_slot(base, (int)rr, NROW);
    if constexpr (XPOSE) {
        if (contig) { store_rows_coalesced<float, NROW>(dst, x, s_wave, lane); return; }
    }
    if (live) dst.template store_row<NROW>(x);
}

template <int SYS, bool DIST, int EPW, int WPW>
__global__ __launch_bounds__(64 * WPW) void sac_collect_kernel(const InstParams<float> I, const PolicyArgs A, const ActorHead B, const CollectRing R) {
    using T = float;
    using Ops = EnvOps<SYS, T, DIST, SCG_SEQ_ST_AUX>;
    using D = Dims<SYS>;
    constexpr CfgParams<T> kcfg = scg_make_spec_cfg<T>();
    constexpr int NIN = kcfg.nobs, NU = D::NU, NOUT = 2 * NU, HID = SCG_POLICY_H, ACT = SCG_POLICY_ACT;
    static_assert(NIN == D::NX || NIN == 2 * D::NX, "the fused rollout serves single-row observations (goal horizon <= 1)");
    using L = MlpLds<NIN, HID, NOUT, 16>;
    constexpr int L1Q = L::L1Q;
    constexpr bool XPOSE = (NIN * (int)sizeof(T)) % 16 == 0;
    extern __shared__ __align__(16) float lds[];
    unsigned char* const s_obs = reinterpret_cast<unsigned char*>(lds + L::END);       // [WPW waves][64 rows][NIN] transpose scratch
    const PV<T> P{kcfg, I};
    const GoalTab<T> goal{nullptr, I.x_goal, false};
    const bool uniform = R.uniform != 0;
    if (!uniform) {
        const MlpWeights w{A.params + A.W1, A.params + A.b1, A.params + A.W2, A.params + A.b2, A.params + A.W3, A.params + A.b3};
        mlp_fill_lds<NIN, HID, NOUT, 16, 64 * WPW>(lds, w, threadIdx.x);
    }
    __syncthreads();
    const int N = I.num_envs;
    const RolloutLanes g = rollout_lanes<EPW, WPW>(N);
    const int i = g.i;
    unsigned char* const s_wave = rollout_wave_scratch<NIN>(s_obs);
    float* const s_mine = reinterpret_cast<float*>(s_wave) + g.lane * NIN;              // this lane's row of the scratch
    const RngKey key{I.key0, I.key1};
    const uint32_t cap = R.capacity;
    const uint32_t pos0 = (uint32_t)((unsigned long long)*R.pos % cap);                 // (a position outside the ring cannot leave it)
    // first env of this wave when all 64 lanes hold envs of their own (g.full_wave)
    const uint32_t wave_first = (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * (64 * WPW) + (threadIdx.x & ~63u)));
    typename Ops::E e;
    float ep[4], acc[8];
    T st[D::NX], row[2 * D::NX];
    bool dirty = false;
    rollout_enter<Ops>(P, goal, key, i, A.ep_stats, A.episode_acc, e, ep, acc, st, row);
    for (int t = 0; t <= A.k_steps; ++t) {
        if (A.obs) store_obs_row<XPOSE, NIN>(A.obs + (size_t)t * N * NIN, g, row, s_wave);
        if (t == A.k_steps) {
            store_obs_row<XPOSE, NIN>(R.cur_obs, g, row, s_wave);
            break;
        }
        // ---- the ring row of (t, i): t N + i < K N <= capacity and pos0 < capacity <= 2^31 - 1, so one subtraction wraps
        const uint32_t tn32 = (uint32_t)t * (uint32_t)N;
        const uint32_t s = pos0 + tn32 + (uint32_t)i, rr = s >= cap ? s - cap : s;
        const uint32_t s0 = pos0 + tn32 + wave_first, rr0 = s0 >= cap ? s0 - cap : s0;
        const bool contig = g.full_wave && rr0 + 64u <= cap;
        store_ring_row<XPOSE, NIN>(R.obs, rr, contig, g.live, row, s_wave, g.lane);
        // ---- the action
        T act[NU];
        if (uniform) {                                      // action_space.sample() (sac.py:276-277): rollout_random_kernel's draw
            const U4 w = rng_words(key, e.gid, e.episode, (uint32_t)e.step, rng_tag(RNG_CH_RANDOM_ACTION, 0, 0));
#pragma unroll
            for (int a = 0; a < NU; ++a) act[a] = B.low[a] + (B.high[a] - B.low[a]) * u01<T>(u4_get(w, a));
        } else {                                            // MLPActorCritic.act(obs) (sac_utils.py:185-222, :258-262): scg_sac_sample's expression
            float xo[L1Q], xr[L1Q], out[NOUT], eps[4];
            b_operand<NIN, L1Q, EPW>(row, g.h, xo, xr);
            mlp_forward_lanes<NIN, HID, NOUT, ACT, (int)MLP_ACT_NONE, EPW>(lds, xo, xr, g.lane, out);
            normal4(rng_words(key, e.gid, e.episode, (uint32_t)e.step, rng_tag(RNG_CH_POLICY, 0, 0)), eps);
#pragma unroll
            for (int a = 0; a < NU; ++a) {
                const float ls = fminf(fmaxf(out[NU + a], -20.0f), 2.0f);
                const float u = __builtin_fmaf(expf(ls), eps[a], out[a]);
                act[a] = B.low[a] + 0.5f * (tanhf(u) + 1.0f) * (B.high[a] - B.low[a]);
            }
        }
        // ---- the control step (identical code to scg_step's kernel)
        const size_t tn = (size_t)t * N + i;
        const int32_t c0 = e.step;
        T noisy[NU];
        typename Ops::StepResult r = Ops::step(P, goal, e, act, nullptr, key, i, st, noisy, seq_slot((T*)nullptr, 0), 0);
        const bool trunc = r.done && (r.flags & 1);         // ended by the time limit: not a termination (sac.py:287-305)
        if (g.live) {
            if (A.act) store_step_row<NU, false>(A.act, nullptr, A.reward, A.done, A.flags, tn, act, 0.0f, r);
            seq_slot(R.act, (int)rr, NU).template store_row<NU>(act);
            seq_slot(R.rew, (int)rr).store(r.reward);
            seq_slot(R.mask, (int)rr).store(trunc ? 1.0f : (r.done ? 0.0f : 1.0f));
        }
        // ---- after the step: after_step's text (scg_rollout_common.h) with the terminal row kept for the ring
        ep[0] += r.reward; ep[1] += 1.0f; ep[2] += (r.flags & FLAG_VIOLATION) ? 1.0f : 0.0f; ep[3] += r.mse;
        Ops::obs_row(P, goal, st, e, key, c0 + 2, (uint32_t)(c0 + 1), c0, i, nullptr, row);
        if (r.done) {
            if (A.terminal_obs && g.live) seq_slot(A.terminal_obs + (size_t)t * N * NIN, i, NIN).template store_row<NIN>(row);
            if (trunc) {
#pragma unroll
                for (int k = 0; k < NIN; ++k) s_mine[k] = row[k];
            }
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
        T nxt[NIN];
#pragma unroll
        for (int k = 0; k < NIN; ++k) nxt[k] = row[k];
        if (trunc) {
#pragma unroll
            for (int k = 0; k < NIN; ++k) nxt[k] = s_mine[k];
        }
        store_ring_row<XPOSE, NIN>(R.next_obs, rr, contig, g.live, nxt, s_wave, g.lane);
    }
    store_tail<Ops>(P, i, g.live, A.ep_stats, A.episode_acc, e, ep, acc, dirty);
}

// The ring's counters behind sac_collect_kernel, which every thread of that launch reads.
__global__ void sac_collect_advance_kernel(const CollectRing R, int n) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const long long cap = (long long)R.capacity;
    *R.pos = (long long)(((unsigned long long)*R.pos % R.capacity + (unsigned long long)n) % R.capacity);
    if (R.size_f) *R.size_f = fminf(*R.size_f + (float)n, (float)cap);
    if (R.size_i) *R.size_i = (int32_t)(((long long)*R.size_i + n) < cap ? ((long long)*R.size_i + n) : cap);
}

}  // namespace scg
#endif  // SCG_ACTOR_COLLECT_KERNEL

extern "C" int scg_rollout_sac_collect(scg_env* env, const scg_actor* actor, int k_steps, const scg_sac_collect* c, void* stream) {
    if (!env || !actor || !c) return fail(SCG_ERR_INVALID, "NULL argument to scg_rollout_sac_collect");
#ifdef SCG_ACTOR_COLLECT_KERNEL
    using namespace scg;
    constexpr int S = SCG_SPEC_SYS, NU = Dims<S>::NU;
    constexpr bool DD = SCG_SPEC_DIST != 0;
    constexpr int nobs = scg_make_spec_cfg<float>().nobs;
    constexpr bool xpose = (nobs * sizeof(float)) % 16 == 0;
    const int N = env->cfg.num_envs;
    const int given = (c->d_obs != nullptr) + (c->d_act != nullptr) + (c->d_reward != nullptr) + (c->d_done != nullptr) + (c->d_flags != nullptr) +
                      (c->d_terminal_obs != nullptr);
    const uintptr_t rows = (uintptr_t)c->d_ring_obs | (uintptr_t)c->d_ring_act | (uintptr_t)c->d_ring_next_obs | (uintptr_t)c->d_cur_obs |
                           (uintptr_t)c->d_obs | (uintptr_t)c->d_terminal_obs | (uintptr_t)c->d_ep_stats |
                           (uintptr_t)c->d_episode_acc;
    const char* stack = given ? rollout_obs_stack_error(xpose, N, nobs) : nullptr;
    if (k_steps < 1) return fail(SCG_ERR_INVALID, "scg_rollout_sac_collect: k_steps must be positive");
    if (!env->has_reset) return fail(SCG_ERR_STATE, "scg_reset (all envs) must be called before scg_rollout_sac_collect");
    if (actor->hidden != SCG_POLICY_H || actor->activation != SCG_POLICY_ACT || actor->kind != SCG_POLICY_KIND)
        return fail(SCG_ERR_INVALID, "scg_rollout_sac_collect: this library was compiled for another actor shape (hidden / activation / kind)");
    if (!actor->d_params || !c->d_ring_obs || !c->d_ring_act || !c->d_ring_rew || !c->d_ring_next_obs || !c->d_ring_mask || !c->d_pos ||
        !c->d_cur_obs)
        return fail(SCG_ERR_INVALID, "scg_rollout_sac_collect needs d_params, the five ring arrays, d_pos and d_cur_obs");
    if (c->capacity < 1 || (long long)k_steps * N > (long long)c->capacity)
        return fail(SCG_ERR_INVALID, "scg_rollout_sac_collect: k_steps x num_envs exceeds the replay capacity (a launch may not overwrite its own rows)");
    if ((unsigned long long)c->capacity * nobs * sizeof(float) > 0xFFFFFF00ull)
        return fail(SCG_ERR_INVALID, "scg_rollout_sac_collect: the ring's observation array exceeds 4 GiB (32-bit row offsets)");
    if (given != 0 && given != 6)
        return fail(SCG_ERR_INVALID, "scg_rollout_sac_collect: the trace outputs (d_obs, d_act, d_reward, d_done, d_flags, d_terminal_obs) are given "
                                     "all together or not at all");
    if (rows & 15) return fail(SCG_ERR_INVALID, "scg_rollout_sac_collect: row arrays must be 16-byte aligned");
    if (((uintptr_t)c->d_ring_rew | (uintptr_t)c->d_ring_mask | (uintptr_t)c->d_reward | (uintptr_t)c->d_act) & 3)
        return fail(SCG_ERR_INVALID, "scg_rollout_sac_collect: float arrays must be 4-byte aligned");
    if (stack) return fail(SCG_ERR_INVALID, stack);
    HIP_TRY(hipSetDevice(env->device));
    PolicyArgs A;
    A.params = actor->d_params; A.W1 = actor->W1; A.b1 = actor->b1; A.W2 = actor->W2; A.b2 = actor->b2; A.W3 = actor->W3; A.b3 = actor->b3;
    A.logstd_off = 0; A.deterministic = 0; A.k_steps = k_steps;
    A.obs = c->d_obs; A.act = c->d_act; A.logp = nullptr; A.reward = c->d_reward; A.done = c->d_done; A.flags = c->d_flags;
    A.terminal_obs = c->d_terminal_obs; A.ep_stats = c->d_ep_stats; A.episode_acc = c->d_episode_acc; A.max_episodes = c->max_episodes;
    ActorHead B;
    for (int j = 0; j < 4; ++j) { B.low[j] = actor->act_low[j]; B.high[j] = actor->act_high[j]; }
    const CollectRing R{c->d_ring_obs, c->d_ring_act, c->d_ring_rew, c->d_ring_next_obs, c->d_ring_mask, (uint32_t)c->capacity,
                        (long long*)c->d_pos, c->d_size_f, c->d_size_i32, c->d_cur_obs, c->uniform != 0 ? 1 : 0};
    const RolloutGeometry g = rollout_geometry(N);
    constexpr size_t image = MlpLds<nobs, SCG_POLICY_H, 2 * NU, 16>::END * sizeof(float), scratch = 64 * nobs * sizeof(float);
    static void (*const k[4])(InstParams<float>, PolicyArgs, ActorHead, CollectRing) = {
        sac_collect_kernel<S, DD, 64, 4>, sac_collect_kernel<S, DD, 64, 8>, sac_collect_kernel<S, DD, 32, 4>, sac_collect_kernel<S, DD, 32, 8>};
    static scg::PerDeviceOnce attr;
    HIP_TRY(launch_rollout(k, attr, (int)(image + 8 * scratch), (int)(image + 8 * scratch), g, N, image + g.wpw * scratch, (hipStream_t)stream,
                           inst_of<float>(env), A, B, R));
    sac_collect_advance_kernel<<<dim3(1), dim3(64), 0, (hipStream_t)stream>>>(R, k_steps * N);
    HIP_TRY(hipGetLastError());
    return SCG_OK;
#else
    (void)k_steps; (void)stream;
#if defined(SCG_ACTOR_ROLLOUT_WIDE)
    return fail(SCG_ERR_INVALID, "scg_rollout_sac_collect does not serve hidden width 256 (the agent trains in PyTorch there): widths 32 / 64 / 96 / 128");
#elif defined(SCG_ACTOR_ROLLOUT) && SCG_POLICY_KIND == 2
    return fail(SCG_ERR_INVALID, "scg_rollout_sac_collect serves kind sac: DDPG's exploration noise is ONE process continued across the envs in env "
                                 "order, a dependency across the batch inside every step");
#elif defined(SCG_ACTOR_ROLLOUT)
    return fail(SCG_ERR_INVALID, "scg_rollout_sac_collect is carried by the actor-rollout library of kind sac, not by this one: build it with "
                                 "_lib.build_spec(cfg, policy=(hidden, activation, 'sac'))");
#else
    return fail(SCG_ERR_INVALID, "scg_rollout_sac_collect needs a library specialised for the task config and the actor's shape with kind sac "
                                 "(float32): build it with _lib.build_spec(cfg, policy=(hidden, activation, 'sac'))");
#endif
#endif
}

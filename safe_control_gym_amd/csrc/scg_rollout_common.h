// scg_rollout_common.h — what the "K control steps with a network in the loop" kernels share.  rollout_cbf_kernel (scg_cbf.hip) and
// rollout_actor_kernel (scg_actor_rollout.h) are built from the device pieces: fill the weight image, rollout_lanes + rollout_enter,
// then per step store_obs_row, b_operand, their own forward pass / draw / filter, EnvOps::step, store_step_row, after_step, and
// store_tail at the end.  rollout_policy_kernel (scg_env_kernels.h), rollout_actor_wide_kernel (scg_actor_rollout_wide.h),
// rollout_adversarial_kernel (scg_adversarial.hip) and rollout_safe_kernel (scg_safe_explorer.hip) keep that loop in their own
// text, because on these pieces some of their instantiations took more registers or scratch; the last two use normal4 and
// mlp_forward_lanes.  All six entry points use the host helpers at the end.
//
// Every helper here is parameterised by values and compile-time shapes (NIN, NU, EPW, WPW, whether rows leave through the LDS
// transpose, the scratch pointer), never by which kernel calls it: a piece that would have to branch on its caller stays in that
// kernel.  The host helpers at the end report instead of failing (a message, a hipError_t), because the error plumbing of the
// translation unit (scg_kernels.hip: fail, HIP_TRY) is defined after this header is read.
#pragma once

#include <cstdlib>
#include <string>

#include "scg_env_kernels.h"
#include "scg_mlp.h"
#include "scg_once.h"

namespace scg {

struct PolicyArgs {
    const float* params; int32_t W1, b1, W2, b2, W3, b3, logstd_off; int32_t deterministic;
    int32_t k_steps;
    float* obs; float* act; float* logp; float* reward; uint8_t* done; uint8_t* flags; float* terminal_obs;
    float* ep_stats; float* episode_acc; int32_t max_episodes;
};
constexpr uint32_t RNG_CH_POLICY = 5;

// ---- lanes ------------------------------------------------------------------------------------------------------------------------
// EPW = envs per wave.  64: lane = env, the wave runs its network on its two 32-env column tiles one after the other.  32: lane
// (c, h) of both halves carries env c (the halves simulate the same env and hold the two k-rows of the MFMA's B operand); half 0
// stores.  WPW = waves per workgroup behind one weight image.
struct RolloutLanes {
    int lane, h;                 // lane of the wave, its half
    int i;                       // the env this lane simulates; surplus lanes shadow the last env (they take part in the MFMAs, never store)
    bool live;                   // this lane stores
    bool full_wave;              // all 64 lanes hold envs of their own: rows may leave through the LDS transpose
};
template <int EPW, int WPW>
__device__ __forceinline__ RolloutLanes rollout_lanes(int N) {
    static_assert(EPW == 64 || EPW == 32, "envs per wave");
    RolloutLanes g;
    g.lane = threadIdx.x & 63;
    g.h = g.lane >> 5;
    const int i0 = EPW == 64 ? blockIdx.x * (64 * WPW) + threadIdx.x : (blockIdx.x * WPW + (threadIdx.x >> 6)) * 32 + (g.lane & 31);
    g.live = i0 < N && (EPW == 64 || g.h == 0);
    g.i = i0 < N ? i0 : N - 1;
    g.full_wave = EPW == 64 && (blockIdx.x * (64 * WPW) + (threadIdx.x & ~63) + 64) <= N;
    return g;
}
// The wave's [64 rows][NIN] piece of the transpose scratch `s_obs` ([WPW waves][64 rows][NIN]).
template <int NIN>
__device__ __forceinline__ unsigned char* rollout_wave_scratch(unsigned char* s_obs) {
    return s_obs + (threadIdx.x >> 6) * (64 * NIN * (int)sizeof(float));
}

// ---- the env of a lane across the K steps -----------------------------------------------------------------------------------------
// A kernel holds, per lane: e (EnvOps::E), ep[4] (the running episode's tallies), acc[8] (the finished episodes' sums), st[NX] (state
// vector), row[2 NX] (observation row) and dirty (an auto-reset redrew the episode's parameters).
// Entry: state, parameters, ep_stats and episode_acc of env i, and the observation of the current state (what the previous step or
// reset returned).
template <typename Ops, typename PVT, typename GOAL>
__device__ __forceinline__ void rollout_enter(const PVT& P, const GOAL& goal, const RngKey& key, int i, float* ep_stats, float* episode_acc,
                                              typename Ops::E& e, float* ep, float* acc, float* st, float* row) {
    Ops::load_state(P, i, e);
    Ops::load_params(P, i, e);
#pragma unroll
    for (int k = 0; k < 4; ++k) ep[k] = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = 0.0f;
    if (ep_stats) seq_slot(ep_stats, i, 4).template load_row<4>(ep);
    if (episode_acc) seq_slot(episode_acc, i, 8).template load_row<8>(acc);
    Ops::state_vector(e, st);
    const bool fresh = e.step == 0;
    const int32_t c0 = e.step - 1;
    Ops::obs_row(P, goal, st, e, key, fresh ? 1 : c0 + 2, fresh ? 0u : (uint32_t)(c0 + 1), fresh ? 0 : c0, i, nullptr, row);
}

// Rollout row obs[t] (`obs_t` = obs + t N NIN).  XPOSE: 16-byte rows of a full wave leave through the LDS transpose (as in step_kernel);
// otherwise row by row (6-float rows of Quadrotor2D stabilisation, or no room for the scratch).
template <bool XPOSE, int NIN>
__device__ __forceinline__ void store_obs_row(float* obs_t, const RolloutLanes& g, const float* row, unsigned char* s_wave) {
    const Slot<float, SCG_SEQ_ST_AUX> dst = seq_slot(obs_t, g.i, NIN);
    if constexpr (XPOSE) {
        if (g.full_wave) store_rows_coalesced<float, NIN>(dst, row, s_wave, g.lane);
        else if (g.live) dst.template store_row<NIN>(row);
    } else {
        if (g.live) dst.template store_row<NIN>(row);
    }
}

// The B operand of layer 1 from the lane's row: xo = my own env's rows row(q, h); EPW 64: xr = the partner env's (lane ^ 32).
template <int NIN, int L1Q, int EPW>
__device__ __forceinline__ void b_operand(const float* row, int h, float* xo, float* xr) {
#pragma unroll
    for (int q = 0; q < L1Q; ++q) {
        const float a0 = d_row(q, 0) < NIN ? row[d_row(q, 0) < NIN ? d_row(q, 0) : 0] : 0.0f;
        const float a1 = d_row(q, 1) < NIN ? row[d_row(q, 1) < NIN ? d_row(q, 1) : 0] : 0.0f;
        xo[q] = h ? a1 : a0;
        if constexpr (EPW == 64) xr[q] = __shfl_xor(h ? a0 : a1, 32, 64);
        else xr[q] = 0.0f;
    }
}

// One MLP's outputs for the lane's env from the LDS image `img`: EPW 32 = one column tile (both lane halves hold env c: xo IS the B
// operand), EPW 64 = the wave's two tiles one after the other (lane (c, h) owns env 32 h + c of the wave).
template <int NIN, int HID, int NOUT, int ACT, int ACT2, int EPW>
__device__ __forceinline__ void mlp_forward_lanes(const float* img, const float* xo, const float* xr, int lane, float* mean) {
    using L = MlpLds<NIN, HID, NOUT, 16>;
    constexpr int L1Q = L::L1Q;
    if constexpr (EPW == 32) {
        f32x16 h1[L::NT], h2[L::NT];
        mlp_forward_tile<NIN, HID, NOUT, ACT, 16, ACT2>(img, xo, h1, h2, mean, lane);
    } else {
        const int h = lane >> 5;
        float x[L1Q], out[NOUT];
        f32x16 h1[L::NT], h2[L::NT];
#pragma unroll
        for (int q = 0; q < L1Q; ++q) x[q] = h == 0 ? xo[q] : xr[q];                    // column tile 0: envs 0..31 of the wave
        mlp_forward_tile<NIN, HID, NOUT, ACT, 16, ACT2>(img, x, h1, h2, out, lane);
#pragma unroll
        for (int a = 0; a < NOUT; ++a) mean[a] = out[a];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 0; q < L1Q; ++q) x[q] = h == 1 ? xo[q] : xr[q];                    // column tile 1: envs 32..63
        mlp_forward_tile<NIN, HID, NOUT, ACT, 16, ACT2>(img, x, h1, h2, out, lane);
#pragma unroll
        for (int a = 0; a < NOUT; ++a) mean[a] = h ? out[a] : mean[a];
    }
}

// ---- the Gaussian head (ppo_utils.py:224-231; distributions.py:12-22) -----------------------------------------------------------------
// Box-Muller of one 4-word Philox draw
__device__ __forceinline__ void normal4(const U4 w, float* eps) {
    const float r0 = m_sqrt(-2.0f * m_log(u01<float>(w.x))), u0 = u01<float>(w.y);
    eps[0] = r0 * cos_2pi(u0);
    eps[1] = r0 * cos_2pi(u0 < 0.25f ? u0 + 0.75f : u0 - 0.25f);        // sin(2 pi u) = cos(2 pi (u - 1/4))
    const float r1 = m_sqrt(-2.0f * m_log(u01<float>(w.z))), u1 = u01<float>(w.w);
    eps[2] = r1 * cos_2pi(u1);
    eps[3] = r1 * cos_2pi(u1 < 0.25f ? u1 + 0.75f : u1 - 0.25f);
}

// sigma = exp(logstd) and the constant part of the log-probability, - sum (logstd + ln sqrt(2 pi))
template <int N>
__device__ __forceinline__ float gaussian_setup(const float* logstd, float* sigma) {
    float logp_const = 0.0f;
#pragma unroll
    for (int a = 0; a < N; ++a) {
        const float ls = logstd[a];
        sigma[a] = __expf(ls);
        logp_const -= ls + 0.91893853320467274f;
    }
    return logp_const;
}

// act = mean (deterministic) or mean + sigma eps with eps the env's draw of this step on `channel`; returns the log-probability.
template <int N, typename E>
__device__ __forceinline__ float gaussian_action(bool deterministic, const RngKey& key, const E& e, uint32_t channel, const float* sigma,
                                                 const float* mean, float logp_const, float* act) {
    static_assert(N <= 4, "one Philox block serves four components");
    float logp = logp_const;
    if (deterministic) {
#pragma unroll
        for (int a = 0; a < N; ++a) act[a] = mean[a];
    } else {
        float eps[4];
        normal4(rng_words(key, e.gid, e.episode, (uint32_t)e.step, rng_tag(channel, 0, 0)), eps);
#pragma unroll
        for (int a = 0; a < N; ++a) {
            act[a] = __builtin_fmaf(sigma[a], eps[a], mean[a]);
            logp -= 0.5f * eps[a] * eps[a];
        }
    }
    return logp;
}

// ---- after the env step -------------------------------------------------------------------------------------------------------------
// The rollout-buffer row of step t (tn = t N + i) of a live lane; logp may be null (a deterministic actor records none).
template <int NU, bool LOGP, typename R>
__device__ __forceinline__ void store_step_row(float* act_out, float* logp_out, float* reward, uint8_t* done, uint8_t* flags, size_t tn,
                                               const float* act, float logp, const R& r) {
#pragma unroll
    for (int a = 0; a < NU; ++a) act_out[tn * NU + a] = act[a];
    if constexpr (LOGP) logp_out[tn] = logp;
    reward[tn] = r.reward;
    done[tn] = r.done ? 1 : 0;
    flags[tn] = r.flags;
}

// Episode tallies, the next observation, and where the episode ended: its terminal observation (into terminal_obs + obs_t_off, the
// offset t N NIN of obs[t]; terminal_obs may be null), its sums into acc while fewer than max_episodes are counted (<= 0: no limit), the auto-reset.  c0 = e.step
// before the step.
template <typename Ops, int NIN, typename PVT, typename GOAL, typename R>
__device__ __forceinline__ void after_step(const PVT& P, const GOAL& goal, const RngKey& key, int i, bool live, int32_t c0, const R& r,
                                           float* terminal_obs, size_t obs_t_off, int32_t max_episodes, typename Ops::E& e, float* ep,
                                           float* acc, float* st, float* row, bool& dirty) {
    ep[0] += r.reward; ep[1] += 1.0f; ep[2] += (r.flags & FLAG_VIOLATION) ? 1.0f : 0.0f; ep[3] += r.mse;
    Ops::obs_row(P, goal, st, e, key, c0 + 2, (uint32_t)(c0 + 1), c0, i, nullptr, row);
    if (r.done) {
        if (terminal_obs && live) seq_slot(terminal_obs + obs_t_off, i, NIN).template store_row<NIN>(row);
        if (max_episodes <= 0 || acc[0] < (float)max_episodes) {
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

template <typename Ops, typename PVT>
__device__ __forceinline__ void store_tail(const PVT& P, int i, bool live, float* ep_stats, float* episode_acc, typename Ops::E& e,
                                           const float* ep, const float* acc, bool dirty) {
    if (live) {
        if (ep_stats) seq_slot(ep_stats, i, 4).template store_row<4>(ep);
        if (episode_acc) seq_slot(episode_acc, i, 8).template store_row<8>(acc);
        Ops::store(P, i, e, dirty);
    }
}

// FILTER of the actor rollouts (a functor between the head and the env step) that filters nothing: the action the env step receives
// is the actor's own; nothing is recorded.
struct ActorNoFilter {
    template <int NU>
    __device__ __forceinline__ void operator()(const float*, const float* act, float* applied, size_t, bool) const {
#pragma unroll
        for (int a = 0; a < NU; ++a) applied[a] = act[a];
    }
};

// ---- host ---------------------------------------------------------------------------------------------------------------------------
// Launch geometry: envs per wave 32 while that gives at most two waves per SIMD (2 x 4 x 256 CUs), else 64; waves per workgroup 4 up
// to one wave per SIMD, 8 above (two waves per SIMD behind one weight image).  SCG_ROLLOUT_EPW = 32 | 64 and SCG_ROLLOUT_WPW = 4 | 8
// override (tests run the geometries on small batches; results do not depend on them: Philox streams are per env, the MFMA sequence
// per env is the same).
struct RolloutGeometry { int epw, wpw; };
inline RolloutGeometry rollout_geometry(int num_envs) {
    RolloutGeometry g{num_envs <= 65536 ? 32 : 64, num_envs <= 32768 ? 4 : 8};
    if (const char* o = getenv("SCG_ROLLOUT_EPW")) { if (atoi(o) == 32 || atoi(o) == 64) g.epw = atoi(o); }
    if (const char* o = getenv("SCG_ROLLOUT_WPW")) { if (atoi(o) == 4 || atoi(o) == 8) g.wpw = atoi(o); }
    return g;
}

// PolicyArgs of a rollout's outputs; the network's offsets are zero (the caller sets the ones its kernel reads).
inline PolicyArgs policy_args(const scg_policy_rollout* out, int k_steps, int deterministic) {
    PolicyArgs A;
    A.params = nullptr; A.W1 = A.b1 = A.W2 = A.b2 = A.W3 = A.b3 = A.logstd_off = 0;
    A.deterministic = deterministic; A.k_steps = k_steps;
    A.obs = (float*)out->d_obs; A.act = (float*)out->d_act; A.logp = (float*)out->d_logp; A.reward = (float*)out->d_reward;
    A.done = out->d_done; A.flags = out->d_flags; A.terminal_obs = (float*)out->d_terminal_obs;
    A.ep_stats = (float*)out->d_ep_stats; A.episode_acc = (float*)out->d_episode_acc; A.max_episodes = out->max_episodes;
    return A;
}
// The same with the network's parameter block and offsets (scg_policy, scg_actor)
template <typename NET>
inline PolicyArgs policy_args(const NET* net, const scg_policy_rollout* out, int k_steps, int deterministic) {
    PolicyArgs A = policy_args(out, k_steps, deterministic);
    A.params = net->d_params; A.W1 = net->W1; A.b1 = net->b1; A.W2 = net->W2; A.b2 = net->b2; A.W3 = net->W3; A.b3 = net->b3;
    return A;
}

inline bool rollout_outputs_present(const scg_policy_rollout* out, bool logp) {
    return out->d_obs && out->d_act && (!logp || out->d_logp) && out->d_reward && out->d_done && out->d_flags;
}
// 16-byte alignment of the per-env row outputs and of `extra` (a caller's own row buffers, or'ed together)
inline bool rollout_rows_aligned(const scg_policy_rollout* out, uintptr_t extra = 0) {
    return (((uintptr_t)out->d_obs | (uintptr_t)out->d_terminal_obs | (uintptr_t)out->d_ep_stats | (uintptr_t)out->d_episode_acc | extra) & 15) == 0;
}
// Rows that leave as 16-byte pieces need every obs[t] aligned; null when fine, else the message.
inline const char* rollout_obs_stack_error(bool xpose, int num_envs, int nobs) {
    if (xpose && ((size_t)num_envs * nobs * sizeof(float)) % 16 != 0)
        return "num_envs x obs_dim x 4 must be a multiple of 16 (row alignment of the [t]-stacked obs)";
    return nullptr;
}

// Argument checks of the SAC / DDPG actor rollouts (scg_rollout_actor, scg_rollout_cbf_actor) of a library compiled for the actor
// shape (H, ACT, KIND): SCG_OK, or the error code with *why set (the caller fails with it).  ENV / ACTOR are scg_env / scg_actor,
// which are complete only after this header is read.
template <typename ENV, typename ACTOR>
inline int actor_rollout_check(std::string* why, const char* who, const ENV* env, const ACTOR* actor, int k_steps, const scg_policy_rollout* out,
                               int H, int ACT, int KIND) {
    const std::string w(who);
    constexpr int nobs = scg_make_spec_cfg<float>().nobs;
    const char* stack = rollout_obs_stack_error((nobs * sizeof(float)) % 16 == 0, env->cfg.num_envs, nobs);
    int rc = SCG_ERR_INVALID;
    if (k_steps <= 0) *why = "k_steps must be positive";
    else if (!env->has_reset) { *why = "scg_reset (all envs) must be called before " + w; rc = SCG_ERR_STATE; }
    else if (actor->hidden != H || actor->activation != ACT || actor->kind != KIND)
        *why = "this library was compiled for another actor shape (hidden / activation / kind)";
    else if (!actor->d_params || !rollout_outputs_present(out, false)) *why = w + " needs d_params, d_obs, d_act, d_reward, d_done and d_flags";
    else if (!rollout_rows_aligned(out)) *why = "row outputs must be 16-byte aligned";
    else if (stack) *why = stack;
    else rc = SCG_OK;
    return rc;
}

// Sets the dynamic-LDS attribute of a kernel's four EPW x WPW instantiations once per device (`once`; the caller has made the
// handle's device current), then launches the one `g` names.  k = {<64, 4>, <64, 8>, <32, 4>, <32, 8>}; attr4 / attr8 = the
// attribute of the 4- and 8-wave kernels, bytes = this launch's dynamic LDS.
template <typename... KA, typename... A>
inline hipError_t launch_rollout(void (*const (&k)[4])(KA...), PerDeviceOnce& once, int attr4, int attr8, RolloutGeometry g, int num_envs,
                                 size_t bytes, hipStream_t st, const A&... args) {
    int dev;
    if (once.pending(&dev)) {
        for (int j = 0; j < 4; ++j)
            if (const hipError_t e = hipFuncSetAttribute((const void*)k[j], hipFuncAttributeMaxDynamicSharedMemorySize, j & 1 ? attr8 : attr4))
                return e;
        once.commit(dev);
    }
    const int per_wg = g.epw * g.wpw;
    const dim3 grid((num_envs + per_wg - 1) / per_wg), block(64 * g.wpw);
    k[(g.epw == 64 ? 0 : 2) + (g.wpw == 4 ? 0 : 1)]<<<grid, block, bytes, st>>>(args...);
    return hipGetLastError();
}

}  // namespace scg

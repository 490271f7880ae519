// scg_adversarial.hip — libscg_advroll_<spechash>_<H>_<act>_<n>.so: the RARL / RAP collector (include/scg_adversarial.h) as one
// launch per T-step collection, next to everything libscg_spec_<hash>_pol<H>_<act>.so carries.
//
// Built only as   hipcc ... -DSCG_SPEC -include <spec header> -DSCG_POLICY_H=<H> -DSCG_POLICY_ACT=<act> -DSCG_ADV_N=<n> scg_adversarial.hip
// (safe_control_gym_amd/_adversarial.py).  The simulator's translation unit is included whole, so that this file reaches struct
// scg_env and the shared device code without any edit to it; the kernel below is rollout_policy_kernel's loop with the adversary's
// forward pass, draw and control between the protagonist's action and the env step (scg_rollout_common.h: the forward, the draw and
// the host side).
#include "scg_kernels.hip"

#include "../../include/scg_adversarial.h"

#if !defined(SCG_SPEC) || !defined(SCG_POLICY_H) || !defined(SCG_ADV_N)
#error "scg_adversarial.hip is built with -DSCG_SPEC -include <spec header> -DSCG_POLICY_H= -DSCG_POLICY_ACT= -DSCG_ADV_N="
#endif
static_assert(SCG_ADV_N >= 1 && SCG_ADV_N <= 4, "adversary population of 1..4");

namespace scg {

constexpr uint32_t RNG_CH_ADVERSARY = 6;          // the adversary's sampling noise (channels 0-5: scg_rng.h / scg_env_kernels.h)
constexpr int LDS_BUDGET = 163840;                 // 160 KiB of LDS per CU (MI355X)

struct AdvActor { const float *W1, *b1, *W2, *b2, *W3, *b3, *logstd; };
struct AdvArgs {
    AdvActor adv[SCG_ADV_N];
    const int32_t* adv_index;                      // [N] or null (one adversary)
    int32_t deterministic;
    float scale, offset;                           // float32 adversary_disturbance_scale / _offset
    float* act;                                    // [K][N][AD] raw sampled actions
    float* logp;                                   // [K][N]
};

// Compile-time shape of this library's kernel and its LDS budget.
struct AdvShape {
    static constexpr CfgParams<float> kcfg = scg_make_spec_cfg<float>();
    static constexpr int SYS = SCG_SPEC_SYS;
    static constexpr int NIN = kcfg.nobs, NU = Dims<SYS>::NU, HID = SCG_POLICY_H, ACT = SCG_POLICY_ACT, N_ADV = SCG_ADV_N;
    static constexpr bool HAS_ADV = kcfg.adversary_channel == SCG_CH_ACTION || kcfg.adversary_channel == SCG_CH_DYNAMICS;
    static constexpr int AD = kcfg.adversary_channel == SCG_CH_ACTION ? NU : Dims<SYS>::DYN;
    using LP = MlpLds<NIN, HID, NU, 16>;
    using LA = MlpLds<NIN, HID, AD, 16>;
    static constexpr int IMG_BYTES = (LP::END + N_ADV * LA::END) * (int)sizeof(float);
    static constexpr int SCRATCH_PER_WAVE = 64 * NIN * (int)sizeof(float);
    // 16-byte rows leave through the LDS transpose as long as the images leave room for it at 4 waves; otherwise row by row
    static constexpr bool XPOSE = (NIN * (int)sizeof(float)) % 16 == 0 && IMG_BYTES + 4 * SCRATCH_PER_WAVE <= LDS_BUDGET;
    static constexpr int bytes(int wpw) { return IMG_BYTES + (XPOSE ? wpw * SCRATCH_PER_WAVE : 0); }
    // waves per workgroup the launcher uses when asked for `wpw` (0: does not fit).  At H = 128 the 8-wave kernels (at most 256
    // registers per lane) spill 84-92 bytes per lane: those shapes run 4 waves per workgroup (no spill) whatever was asked for.
    static constexpr bool WIDE_OK = HID < 128;
    static constexpr int wpw_used(int wpw) {
        return wpw == 8 && WIDE_OK && bytes(8) <= LDS_BUDGET ? 8 : bytes(4) <= LDS_BUDGET ? 4 : 0;
    }
};

// This kernel keeps its own text (on the shared entry / after_step pieces some of its instantiations took more registers); it shares
// normal4 and mlp_forward_lanes.  Per step: protagonist means and sample (channel 5); for every adversary index present in
// the wave (a wave-uniform loop over a ballot) that adversary's MLP on the wave's column tiles, each lane keeping its own env's
// result; the adversary's sample (channel 6) and log-probability; set_adversary_control; the env step.
template <int EPW, int WPW>
__global__ __launch_bounds__(64 * WPW) void rollout_adversarial_kernel(const InstParams<float> I, const PolicyArgs A, const AdvArgs B) {
    using T = float;
    using S = AdvShape;
    constexpr int SYS = S::SYS;
    constexpr bool DIST = SCG_SPEC_DIST != 0;
    using Ops = EnvOps<SYS, T, DIST, SCG_SEQ_ST_AUX>;
    using D = Dims<SYS>;
    constexpr CfgParams<T> kcfg = scg_make_spec_cfg<T>();
    constexpr int NIN = S::NIN, NU = S::NU, HID = S::HID, AD = S::AD, NADV = S::N_ADV;
    static_assert(NIN == D::NX || NIN == 2 * D::NX, "the fused rollout serves single-row observations (goal horizon <= 1)");
    using LP = typename S::LP;
    using LA = typename S::LA;
    constexpr int L1Q = LP::L1Q;
    extern __shared__ __align__(16) float lds[];
    unsigned char* const s_obs = reinterpret_cast<unsigned char*>(lds + LP::END + NADV * LA::END);   // [WPW][64][NIN] (XPOSE only)
    const PV<T> P{kcfg, I};
    const GoalTab<T> goal{nullptr, I.x_goal, false};
    {
        const MlpWeights w{A.params + A.W1, A.params + A.b1, A.params + A.W2, A.params + A.b2, A.params + A.W3, A.params + A.b3};
        mlp_fill_lds<NIN, HID, NU, 16, 64 * WPW>(lds, w, threadIdx.x);
#pragma unroll
        for (int k = 0; k < NADV; ++k) {
            const MlpWeights wa{B.adv[k].W1, B.adv[k].b1, B.adv[k].W2, B.adv[k].b2, B.adv[k].W3, B.adv[k].b3};
            mlp_fill_lds<NIN, HID, AD, 16, 64 * WPW>(lds + LP::END + k * LA::END, wa, threadIdx.x);
        }
    }
    __syncthreads();
    const int N = I.num_envs;
    static_assert(EPW == 64 || EPW == 32, "envs per wave");
    const int lane = threadIdx.x & 63, h = lane >> 5;
    const int i0 = EPW == 64 ? blockIdx.x * (64 * WPW) + threadIdx.x : (blockIdx.x * WPW + (threadIdx.x >> 6)) * 32 + (lane & 31);
    const bool live = i0 < N && (EPW == 64 || h == 0);
    const int i = i0 < N ? i0 : N - 1;                // surplus lanes shadow the last env (they take part in the MFMAs, never store)
    const bool full_wave = EPW == 64 && (blockIdx.x * (64 * WPW) + (threadIdx.x & ~63) + 64) <= N;
    unsigned char* const s_wave = s_obs + (threadIdx.x >> 6) * S::SCRATCH_PER_WAVE;
    typename Ops::E e;
    Ops::load_state(P, i, e);
    Ops::load_params(P, i, e);
    const RngKey key{I.key0, I.key1};
    float ep[4] = {0.0f, 0.0f, 0.0f, 0.0f}, acc[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (A.ep_stats) seq_slot(A.ep_stats, i, 4).template load_row<4>(ep);
    if (A.episode_acc) seq_slot(A.episode_acc, i, 8).template load_row<8>(acc);
    float sigma[NU], logp_const = 0.0f;
#pragma unroll
    for (int a = 0; a < NU; ++a) {
        const float ls = A.params[A.logstd_off + a];
        sigma[a] = __expf(ls);
        logp_const -= ls + 0.91893853320467274f;
    }
    // this env's adversary (fixed for the launch) and its noise scale
    int my = 0;
    if constexpr (NADV > 1) {
        const int32_t v = B.adv_index[i];
        my = v < 0 ? 0 : v >= NADV ? NADV - 1 : v;
    }
    const float* my_logstd = B.adv[0].logstd;
#pragma unroll
    for (int k = 1; k < NADV; ++k) my_logstd = my == k ? B.adv[k].logstd : my_logstd;     // (no dynamic index into the argument block)
    float sigma_a[AD], logp_const_a = 0.0f;
#pragma unroll
    for (int a = 0; a < AD; ++a) {
        const float ls = my_logstd[a];
        sigma_a[a] = __expf(ls);
        logp_const_a -= ls + 0.91893853320467274f;
    }
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
            if constexpr (S::XPOSE) {
                if (full_wave) store_rows_coalesced<T, NIN>(dst, row, s_wave, lane);
                else if (live) dst.template store_row<NIN>(row);
            } else {
                if (live) dst.template store_row<NIN>(row);
            }
        }
        if (t == A.k_steps) break;
        float xo[L1Q], xr[L1Q];
#pragma unroll
        for (int q = 0; q < L1Q; ++q) {
            const float a0 = d_row(q, 0) < NIN ? row[d_row(q, 0) < NIN ? d_row(q, 0) : 0] : 0.0f;
            const float a1 = d_row(q, 1) < NIN ? row[d_row(q, 1) < NIN ? d_row(q, 1) : 0] : 0.0f;
            xo[q] = h ? a1 : a0;
            if constexpr (EPW == 64) xr[q] = __shfl_xor(h ? a0 : a1, 32, 64);
            else xr[q] = 0.0f;
        }
        // ---- protagonist (rollout_policy_kernel's action and log-probability)
        float mean[NU];
        mlp_forward_lanes<NIN, HID, NU, S::ACT, S::ACT, EPW>(lds, xo, xr, lane, mean);
        T act[NU];
        float logp = logp_const;
        if (A.deterministic) {
#pragma unroll
            for (int a = 0; a < NU; ++a) act[a] = mean[a];
        } else {
            float eps[4];
            normal4(rng_words(key, e.gid, e.episode, (uint32_t)e.step, rng_tag(RNG_CH_POLICY, 0, 0)), eps);
#pragma unroll
            for (int a = 0; a < NU; ++a) {
                act[a] = __builtin_fmaf(sigma[a], eps[a], mean[a]);
                logp -= 0.5f * eps[a] * eps[a];
            }
        }
        // ---- adversary: every index present in the wave, uniformly; each lane keeps its own env's means
        float amean[AD];
#pragma unroll
        for (int a = 0; a < AD; ++a) amean[a] = 0.0f;
#pragma unroll 1
        for (int k = 0; k < NADV; ++k) {
            if (NADV > 1 && __ballot(my == k) == 0) continue;
            float m[AD];
            mlp_forward_lanes<NIN, HID, AD, S::ACT, S::ACT, EPW>(lds + LP::END + k * LA::END, xo, xr, lane, m);
#pragma unroll
            for (int a = 0; a < AD; ++a) amean[a] = my == k ? m[a] : amean[a];
        }
        float aact[AD], alogp = logp_const_a;
        if (B.deterministic) {
#pragma unroll
            for (int a = 0; a < AD; ++a) aact[a] = amean[a];
        } else {
            float eps[4];
            normal4(rng_words(key, e.gid, e.episode, (uint32_t)e.step, rng_tag(RNG_CH_ADVERSARY, 0, 0)), eps);
#pragma unroll
            for (int a = 0; a < AD; ++a) {
                aact[a] = __builtin_fmaf(sigma_a[a], eps[a], amean[a]);
                alogp -= 0.5f * eps[a] * eps[a];
            }
        }
        // ---- set_adversary_control (benchmark_env.py:216-228): clip, scale, offset — two roundings, as the PyTorch path
        T actrl[AD];
#pragma unroll
        for (int a = 0; a < AD; ++a) actrl[a] = __fadd_rn(__fmul_rn(fminf(fmaxf(aact[a], -1.0f), 1.0f), B.scale), B.offset);
        // ---- the control step (identical code to scg_step's kernel)
        const int32_t c0 = e.step;
        T noisy[NU];
        typename Ops::StepResult r = Ops::step(P, goal, e, act, actrl, key, i, st, noisy, seq_slot((T*)nullptr, 0), 0);
        const size_t tn = (size_t)t * N + i;
        if (live) {
#pragma unroll
            for (int a = 0; a < NU; ++a) A.act[tn * NU + a] = act[a];
            A.logp[tn] = logp;
#pragma unroll
            for (int a = 0; a < AD; ++a) B.act[tn * AD + a] = aact[a];
            B.logp[tn] = alogp;
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

extern "C" int scg_adversarial_shape(int32_t* n_adversaries, int32_t* hidden, int32_t* activation, int32_t* adv_dim) {
    if (n_adversaries) *n_adversaries = AdvShape::N_ADV;
    if (hidden) *hidden = AdvShape::HID;
    if (activation) *activation = AdvShape::ACT;
    if (adv_dim) *adv_dim = AdvShape::HAS_ADV ? AdvShape::AD : 0;
    return SCG_OK;
}

extern "C" int scg_adversarial_lds(int wpw, int32_t* lds_bytes, int32_t* wpw_used) {
    if (wpw != 4 && wpw != 8) return fail(SCG_ERR_INVALID, "waves per workgroup must be 4 or 8");
    const int w = AdvShape::wpw_used(wpw);
    if (lds_bytes) *lds_bytes = w ? AdvShape::bytes(w) : AdvShape::bytes(4);
    if (wpw_used) *wpw_used = w;
    return SCG_OK;
}

extern "C" int scg_rollout_adversarial(scg_env* env, const scg_policy* pol, const scg_actor_ptrs* advs, int n_adversaries,
                                       const int32_t* d_adv_index, int deterministic_adversary, int k_steps, const scg_policy_rollout* out,
                                       void* d_adv_act, void* d_adv_logp, void* stream) {
    using S = AdvShape;
    if (!env || !pol || !advs || !out) return fail(SCG_ERR_INVALID, "NULL argument to scg_rollout_adversarial");
#if SCG_SPEC_DTYPE == 0
    if (!S::HAS_ADV) return fail(SCG_ERR_INVALID, "scg_rollout_adversarial needs a task config with adversary_disturbance set");
    if (n_adversaries != S::N_ADV)
        return fail(SCG_ERR_INVALID, "this library was compiled for " + std::to_string(S::N_ADV) + " adversaries, not " +
                                         std::to_string(n_adversaries));
    if (S::N_ADV > 1 && !d_adv_index) return fail(SCG_ERR_INVALID, "a population of adversaries needs d_adv_index");
    if (k_steps <= 0) return fail(SCG_ERR_INVALID, "k_steps must be positive");
    if (!env->has_reset) return fail(SCG_ERR_STATE, "scg_reset (all envs) must be called before scg_rollout_adversarial");
    if (pol->hidden != S::HID || pol->activation != S::ACT)
        return fail(SCG_ERR_INVALID, "this library was compiled for another policy shape (hidden / activation)");
    if (!pol->d_params || !rollout_outputs_present(out, true) || !d_adv_act || !d_adv_logp)
        return fail(SCG_ERR_INVALID, "scg_rollout_adversarial needs d_params, d_obs, d_act, d_logp, d_reward, d_done, d_flags, d_adv_act "
                                     "and d_adv_logp");
    for (int k = 0; k < n_adversaries; ++k) {
        const scg_actor_ptrs& a = advs[k];
        if (!a.W1 || !a.b1 || !a.W2 || !a.b2 || !a.W3 || !a.b3 || !a.logstd)
            return fail(SCG_ERR_INVALID, "adversary " + std::to_string(k) + " has a NULL parameter pointer");
    }
    if (!rollout_rows_aligned(out)) return fail(SCG_ERR_INVALID, "row outputs must be 16-byte aligned");
    if (const char* why = rollout_obs_stack_error(S::XPOSE, env->cfg.num_envs, S::NIN)) return fail(SCG_ERR_INVALID, why);
    // the LDS budget may lower the waves per workgroup
    RolloutGeometry g = rollout_geometry(env->cfg.num_envs);
    g.wpw = S::wpw_used(g.wpw);
    if (g.wpw == 0)
        return fail(SCG_ERR_INVALID, "the weight images of the protagonist and " + std::to_string(S::N_ADV) + " adversaries need " +
                                         std::to_string(S::bytes(4)) + " B of LDS per workgroup, more than the 163840 B of a CU");
    HIP_TRY(hipSetDevice(env->device));
    PolicyArgs A = policy_args(pol, out, k_steps, pol->deterministic);
    A.logstd_off = pol->logstd_off;
    AdvArgs B;
    for (int k = 0; k < S::N_ADV; ++k)
        B.adv[k] = {advs[k].W1, advs[k].b1, advs[k].W2, advs[k].b2, advs[k].W3, advs[k].b3, advs[k].logstd};
    B.adv_index = d_adv_index; B.deterministic = deterministic_adversary;
    B.scale = (float)env->cfg.adversary_scale; B.offset = (float)env->cfg.adversary_offset;
    B.act = (float*)d_adv_act; B.logp = (float*)d_adv_logp;
    static void (*const k[4])(InstParams<float>, PolicyArgs, AdvArgs) = {rollout_adversarial_kernel<64, 4>, rollout_adversarial_kernel<64, 8>,
                                                                        rollout_adversarial_kernel<32, 4>, rollout_adversarial_kernel<32, 8>};
    static scg::PerDeviceOnce attr;
    HIP_TRY(launch_rollout(k, attr, S::bytes(4), S::wpw_used(8) == 8 ? S::bytes(8) : S::bytes(4), g, env->cfg.num_envs, (size_t)S::bytes(g.wpw),
                           (hipStream_t)stream, inst_of<float>(env), A, B));
    return SCG_OK;
#else
    (void)d_adv_index; (void)deterministic_adversary; (void)k_steps; (void)d_adv_act; (void)d_adv_logp; (void)stream;
    return fail(SCG_ERR_INVALID, "scg_rollout_adversarial serves float32 envs");
#endif
}

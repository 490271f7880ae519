// scg_safe_explorer.hip — libscg_saferoll_<spechash>_<H>_<act>_<Hc>.so: the Safe-Explorer PPO collector (include/scg_safe_explorer.h)
// as one launch per T-step collection, next to everything libscg_spec_<hash>.so carries.
//
// Built only as   hipcc ... -DSCG_SPEC -include <spec header> -DSCG_POLICY_H=<H> -DSCG_POLICY_ACT=<act> -DSCG_SAFE_HC=<Hc> scg_safe_explorer.hip
// (safe_control_gym_amd/_safe_explorer.py).  As in scg_adversarial.hip the simulator's translation unit is included whole, without
// any edit to it; the kernel is rollout_policy_kernel's loop with the safety layer between the actor's mean and the sample, and the
// constraint values of the next state after the env step (scg_rollout_common.h: the forward, the draw and the host side).
#include "scg_kernels.hip"

#include <cstring>

#include "../../include/scg_safe_explorer.h"

#if !defined(SCG_SPEC) || !defined(SCG_POLICY_H) || !defined(SCG_SAFE_HC)
#error "scg_safe_explorer.hip is built with -DSCG_SPEC -include <spec header> -DSCG_POLICY_H= -DSCG_POLICY_ACT= -DSCG_SAFE_HC="
#endif

namespace scg {

constexpr int SAFE_LDS_BUDGET = 163840;           // 160 KiB of LDS per CU (MI355X)

struct SafeArgs {
    MlpWeights actor;
    const float* logstd;                           // [NU]
    const float* safety;                           // packed layer (include/scg_safe_explorer.h)
    const float* slack;                            // [NC]
    float* c_rows;                                 // [K][N][NC]
    float* c_carry;                                // [N][NC]
};

// Compile-time shape of this library's kernel, the packed layer and the LDS budget.
struct SafeShape {
    static constexpr CfgParams<float> kcfg = scg_make_spec_cfg<float>();
    static constexpr int SYS = SCG_SPEC_SYS;
    static constexpr int NIN = kcfg.nobs, NU = Dims<SYS>::NU, HID = SCG_POLICY_H, ACT = SCG_POLICY_ACT;
    static constexpr int NC = kcfg.n_state_con_rows, HC = SCG_SAFE_HC;
    static constexpr int HCP = (HC + 31) / 32 * 32, NTC = HCP / 32, Q = 4 * ((NIN + 7) / 8);
    // one constraint's block (words): W1f [NTC][Q][64] | b1 [HCP] | W2 [NU][HCP] | b2 [4]
    static constexpr int W1F = 0, B1 = NTC * Q * 64, W2 = B1 + HCP, B2 = W2 + NU * HCP, STRIDE = B2 + 4;
    static constexpr int SAFE_WORDS = NC * STRIDE;
    static_assert(NC >= 1 && NC <= 32, "1..32 state-constraint rows");
    static_assert(HC >= 1 && HC <= 256 && NU <= 4 && NIN <= 32, "safety layer of at most 256 hidden units, 4 actions, 32 inputs");
    using LP = MlpLds<NIN, HID, NU, 16>;
    static constexpr int IMG_BYTES = LP::END * (int)sizeof(float);
    static constexpr int SAFE_BYTES = SAFE_WORDS * (int)sizeof(float);
    static constexpr int SCRATCH_PER_WAVE = 64 * NIN * (int)sizeof(float);
    // 16-byte rows leave through the LDS transpose as long as the actor image leaves room for it at 4 waves (the safety layer then
    // goes to LDS only if it fits next to both); otherwise row by row
    static constexpr bool XPOSE = (NIN * (int)sizeof(float)) % 16 == 0 && IMG_BYTES + 4 * SCRATCH_PER_WAVE <= SAFE_LDS_BUDGET;
    static constexpr int bytes(int wpw, bool in_lds) { return IMG_BYTES + (in_lds ? SAFE_BYTES : 0) + (XPOSE ? wpw * SCRATCH_PER_WAVE : 0); }
    // waves per workgroup for `wpw` asked (0: does not fit); hidden 128 runs 4 waves (the 8-wave kernels would spill), as scg_adversarial
    static constexpr bool WIDE_OK = HID < 128;
    static constexpr int wpw_used(int wpw, bool in_lds) {
        return wpw == 8 && WIDE_OK && bytes(8, in_lds) <= SAFE_LDS_BUDGET ? 8 : bytes(4, in_lds) <= SAFE_LDS_BUDGET ? 4 : 0;
    }
};

// g = W2 relu(W1 x + b1) + b2 of one constraint block `w` (LDS or global: the same instructions, only the operand source differs)
// for one 32-sample column tile; x[q] = input row(q, h) of the lane's sample.  Layer 1 on the matrix cores (Y^T = W1 X^T, one 32x32
// tile per 32 hidden units), the output on the vector unit from the accumulator registers, the two lane halves summed at the end.
__device__ __forceinline__ void safe_constraint_tile(const float* w, const float* x, int lane, float* g) {
    using S = SafeShape;
    const int h = lane >> 5;
    float s[S::NU];
#pragma unroll
    for (int o = 0; o < S::NU; ++o) s[o] = 0.0f;
#pragma unroll
    for (int rho = 0; rho < S::NTC; ++rho) {
        f32x16 acc;
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {                                 // bias: hidden rows 32 rho + 8 g4 + 4 h + (0..3)
            const f32x4 b = *reinterpret_cast<const f32x4*>(w + S::B1 + 32 * rho + 8 * g4 + 4 * h);
            acc[4 * g4 + 0] = b.x; acc[4 * g4 + 1] = b.y; acc[4 * g4 + 2] = b.z; acc[4 * g4 + 3] = b.w;
        }
#pragma unroll
        for (int q = 0; q < S::Q; ++q) acc = mfma32(w[S::W1F + (rho * S::Q + q) * 64 + lane], x[q], acc);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[q] = fmaxf(acc[q], 0.0f);
#pragma unroll
        for (int o = 0; o < S::NU; ++o) {
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(w + S::W2 + o * S::HCP + 32 * rho + 8 * g4 + 4 * h);
                s[o] = __builtin_fmaf(v.x, acc[4 * g4 + 0], s[o]); s[o] = __builtin_fmaf(v.y, acc[4 * g4 + 1], s[o]);
                s[o] = __builtin_fmaf(v.z, acc[4 * g4 + 2], s[o]); s[o] = __builtin_fmaf(v.w, acc[4 * g4 + 3], s[o]);
            }
        }
    }
#pragma unroll
    for (int o = 0; o < S::NU; ++o) {
        s[o] += __shfl_xor(s[o], 32, 64);
        g[o] = s[o] + w[S::B2 + o];
    }
}

// SafetyLayer.get_safe_action for the lane's env: every constraint's g (both column tiles with 64 envs per wave), its multiplier, the
// first maximum kept on the fly; mean <- mean - mult* g*.
template <int EPW>
__device__ __forceinline__ void safe_project(const float* sw, const float* slack, const float* xo, const float* xr, int lane, const float* c,
                                             float* mean) {
    using S = SafeShape;
    const int h = lane >> 5;
    float x0[S::Q], x1[S::Q];
#pragma unroll
    for (int q = 0; q < S::Q; ++q) {
        x0[q] = EPW == 32 || h == 0 ? xo[q] : xr[q];
        x1[q] = h == 1 ? xo[q] : xr[q];
    }
    float best = 0.0f, bg[S::NU];
#pragma unroll
    for (int a = 0; a < S::NU; ++a) bg[a] = 0.0f;
#pragma unroll 1
    for (int k = 0; k < S::NC; ++k) {
        const float* w = sw + (size_t)k * S::STRIDE;
        float g[S::NU];
        safe_constraint_tile(w, x0, lane, g);
        if constexpr (EPW == 64) {
            float g1[S::NU];
            __builtin_amdgcn_sched_barrier(0);
            safe_constraint_tile(w, x1, lane, g1);
#pragma unroll
            for (int a = 0; a < S::NU; ++a) g[a] = h ? g1[a] : g[a];
        }
        float ck = c[0];                                                 // c[k] by a select chain (no dynamic index into registers)
#pragma unroll
        for (int j = 1; j < S::NC; ++j) ck = j == k ? c[j] : ck;
        float dot = __fmul_rn(g[0], mean[0]), gg = __fmul_rn(g[0], g[0]);
#pragma unroll
        for (int a = 1; a < S::NU; ++a) {
            dot = __fadd_rn(dot, __fmul_rn(g[a], mean[a]));
            gg = __fadd_rn(gg, __fmul_rn(g[a], g[a]));
        }
        const float numer = __fadd_rn(__fadd_rn(dot, ck), slack[k]);
        const float denom = __fadd_rn(gg, 1e-8f);
        const float mult = fmaxf(__fdiv_rn(numer, denom), 0.0f);
        if (k == 0 || mult > best) {                                    // the first maximum, as torch.max
            best = mult;
#pragma unroll
            for (int a = 0; a < S::NU; ++a) bg[a] = g[a];
        }
    }
#pragma unroll
    for (int a = 0; a < S::NU; ++a) mean[a] = __fsub_rn(mean[a], __fmul_rn(best, bg[a]));
}

// This kernel keeps its own text (on the shared entry / after_step pieces some of its instantiations spilled more); it shares normal4
// and mlp_forward_lanes.  SAFE_LDS: the packed safety layer is copied into LDS behind the
// actor image (else every wave reads it from memory).
template <int EPW, int WPW, bool SAFE_LDS>
__global__ __launch_bounds__(64 * WPW) void rollout_safe_kernel(const InstParams<float> I, const PolicyArgs A, const SafeArgs B) {
    using T = float;
    using S = SafeShape;
    constexpr int SYS = S::SYS;
    constexpr bool DIST = SCG_SPEC_DIST != 0;
    using Ops = EnvOps<SYS, T, DIST, SCG_SEQ_ST_AUX>;
    using D = Dims<SYS>;
    constexpr CfgParams<T> kcfg = scg_make_spec_cfg<T>();
    constexpr int NIN = S::NIN, NU = S::NU, HID = S::HID, NC = S::NC;
    static_assert(NIN == D::NX || NIN == 2 * D::NX, "the fused rollout serves single-row observations (goal horizon <= 1)");
    using LP = typename S::LP;
    constexpr int L1Q = LP::L1Q;
    extern __shared__ __align__(16) float lds[];
    unsigned char* const s_obs = reinterpret_cast<unsigned char*>(lds + LP::END + (SAFE_LDS ? S::SAFE_WORDS : 0));   // (XPOSE only)
    const PV<T> P{kcfg, I};
    const GoalTab<T> goal{nullptr, I.x_goal, false};
    mlp_fill_lds<NIN, HID, NU, 16, 64 * WPW>(lds, B.actor, threadIdx.x);
    if constexpr (SAFE_LDS) {                       // the packed layer is already in its operand order: a straight 16-byte copy
        for (int k = 4 * (int)threadIdx.x; k < S::SAFE_WORDS; k += 4 * 64 * WPW)
            *reinterpret_cast<f32x4*>(lds + LP::END + k) = *reinterpret_cast<const f32x4*>(B.safety + k);
    }
    __syncthreads();
    const float* sw;
    if constexpr (SAFE_LDS) sw = lds + LP::END;
    else sw = B.safety;
    const int N = I.num_envs;
    static_assert(EPW == 64 || EPW == 32, "envs per wave");
    const int lane = threadIdx.x & 63, h = lane >> 5;
    const int i0 = EPW == 64 ? blockIdx.x * (64 * WPW) + threadIdx.x : (blockIdx.x * WPW + (threadIdx.x >> 6)) * 32 + (lane & 31);
    const bool live = i0 < N && (EPW == 64 || h == 0);
    const int i = i0 < N ? i0 : N - 1;                // surplus lanes shadow the last env (they take part in the MFMAs)
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
        const float ls = B.logstd[a];
        sigma[a] = __expf(ls);
        logp_const -= ls + 0.91893853320467274f;
    }
    // the constraint values the first step's policy sees: the carry, row 0 of the stacked output
    {
        float c[NC];
        seq_slot(B.c_carry, i, NC).template load_row<NC>(c);
        if (live) seq_slot(B.c_rows, i, NC).template store_row<NC>(c);
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
        // ---- actor mean, safety projection, sample (rollout_policy_kernel's draw and log-probability around the filtered mean)
        float mean[NU];
        mlp_forward_lanes<NIN, HID, NU, S::ACT, S::ACT, EPW>(lds, xo, xr, lane, mean);
        __builtin_amdgcn_sched_barrier(0);
        {
            // step t's constraint values, read back where the previous step (or the launch) wrote them: not held in registers across
            // the actor and the env step
            float c[NC];
            seq_slot(t == 0 ? B.c_carry : B.c_rows + (size_t)t * N * NC, i, NC).template load_row<NC>(c);
            safe_project<EPW>(sw, B.slack, xo, xr, lane, c, mean);
        }
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
        // ---- the control step (identical code to scg_step's kernel)
        const int32_t c0 = e.step;
        T noisy[NU];
        typename Ops::StepResult r = Ops::step(P, goal, e, act, nullptr, key, i, st, noisy, seq_slot((T*)nullptr, 0), 0);
        const size_t tn = (size_t)t * N + i;
        if (live) {
#pragma unroll
            for (int a = 0; a < NU; ++a) A.act[tn * NU + a] = act[a];
            A.logp[tn] = logp;
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
        // ---- the next step's constraint values: the state rows of the post-step state, or of the fresh one after a reset
        // (`st` holds whichever the env now is in).  EnvOps::constraints writes through a slot: into c_rows[t + 1], or the carry after
        // the last step; the next policy step reads them back from there.  Shadow lanes write the same values as the lane of the env
        // they shadow, to the same address.
        Ops::constraints(P, st, act, seq_slot(t + 1 < A.k_steps ? B.c_rows + (size_t)(t + 1) * N * NC : B.c_carry, i, NC), 1, true);
    }
    if (live) {
        if (A.ep_stats) seq_slot(A.ep_stats, i, 4).template store_row<4>(ep);
        if (A.episode_acc) seq_slot(A.episode_acc, i, 8).template store_row<8>(acc);
        Ops::store(P, i, e, dirty);
    }
}

// The launcher's choice for `wpw` waves asked: waves per workgroup (0: nothing fits) and the placement; `why` on failure.
static int safe_choose(int wpw, bool* in_lds, std::string* why) {
    using S = SafeShape;
    const char* f = getenv("SCG_SAFE_WEIGHTS");
    const bool force_lds = f && strcmp(f, "lds") == 0, force_global = f && strcmp(f, "global") == 0;
    const int wl = S::wpw_used(wpw, true), wg = S::wpw_used(wpw, false);
    if (force_lds || (!force_global && wl)) {
        *in_lds = true;
        if (!wl && why)
            *why = "the actor image and the safety layer need " + std::to_string(S::bytes(4, true)) +
                   " B of LDS per workgroup, more than the 163840 B of a CU (SCG_SAFE_WEIGHTS=lds)";
        return wl;
    }
    *in_lds = false;
    if (!wg && why) *why = "the actor image needs " + std::to_string(S::bytes(4, false)) + " B of LDS per workgroup, more than the 163840 B of a CU";
    return wg;
}

}  // namespace scg

extern "C" int scg_safe_explorer_shape(int32_t* n_constraints, int32_t* hidden_c, int32_t* hidden, int32_t* activation, int32_t* act_dim,
                                       int32_t* obs_dim, int32_t* packed_words) {
    using S = SafeShape;
    if (n_constraints) *n_constraints = S::NC;
    if (hidden_c) *hidden_c = S::HC;
    if (hidden) *hidden = S::HID;
    if (activation) *activation = S::ACT;
    if (act_dim) *act_dim = S::NU;
    if (obs_dim) *obs_dim = S::NIN;
    if (packed_words) *packed_words = S::SAFE_WORDS;
    return SCG_OK;
}

extern "C" int scg_safe_explorer_lds(int wpw, int32_t* lds_bytes, int32_t* wpw_used, int32_t* weights_in_lds) {
    if (wpw != 4 && wpw != 8) return fail(SCG_ERR_INVALID, "waves per workgroup must be 4 or 8");
    bool in_lds = false;
    const int w = safe_choose(wpw, &in_lds, nullptr);
    if (lds_bytes) *lds_bytes = SafeShape::bytes(w ? w : 4, in_lds);
    if (wpw_used) *wpw_used = w;
    if (weights_in_lds) *weights_in_lds = in_lds ? 1 : 0;
    return SCG_OK;
}

extern "C" int scg_rollout_safe(scg_env* env, const scg_actor_ptrs* actor, const float* d_safety, const float* d_slack, int deterministic,
                                int k_steps, const scg_policy_rollout* out, float* d_c_rows, float* d_c_carry, void* stream) {
    using S = SafeShape;
    if (!env || !actor || !out) return fail(SCG_ERR_INVALID, "NULL argument to scg_rollout_safe");
#if SCG_SPEC_DTYPE == 0
    if (k_steps <= 0) return fail(SCG_ERR_INVALID, "k_steps must be positive");
    if (!env->has_reset) return fail(SCG_ERR_STATE, "scg_reset (all envs) must be called before scg_rollout_safe");
    if (!actor->W1 || !actor->b1 || !actor->W2 || !actor->b2 || !actor->W3 || !actor->b3 || !actor->logstd)
        return fail(SCG_ERR_INVALID, "the actor has a NULL parameter pointer");
    if (!d_safety || !d_slack || !d_c_rows || !d_c_carry || !rollout_outputs_present(out, true))
        return fail(SCG_ERR_INVALID, "scg_rollout_safe needs d_safety, d_slack, d_c_rows, d_c_carry, d_obs, d_act, d_logp, d_reward, d_done "
                                     "and d_flags");
    if (!rollout_rows_aligned(out, (uintptr_t)d_safety | (uintptr_t)d_c_rows | (uintptr_t)d_c_carry))
        return fail(SCG_ERR_INVALID, "row outputs, the packed safety layer and the constraint-value buffers must be 16-byte aligned");
    if (const char* stack = rollout_obs_stack_error(S::XPOSE, env->cfg.num_envs, S::NIN)) return fail(SCG_ERR_INVALID, stack);
    // the LDS budget picks the placement and may lower the waves per workgroup
    RolloutGeometry g = rollout_geometry(env->cfg.num_envs);
    bool in_lds = false;
    std::string why;
    g.wpw = safe_choose(g.wpw, &in_lds, &why);
    if (g.wpw == 0) return fail(SCG_ERR_INVALID, why);
    HIP_TRY(hipSetDevice(env->device));
    const PolicyArgs A = policy_args(out, k_steps, deterministic ? 1 : 0);
    SafeArgs B;
    B.actor = MlpWeights{actor->W1, actor->b1, actor->W2, actor->b2, actor->W3, actor->b3};
    B.logstd = actor->logstd; B.safety = d_safety; B.slack = d_slack; B.c_rows = d_c_rows; B.c_carry = d_c_carry;
    static void (*const kg[4])(InstParams<float>, PolicyArgs, SafeArgs) = {rollout_safe_kernel<64, 4, false>, rollout_safe_kernel<64, 8, false>,
                                                                         rollout_safe_kernel<32, 4, false>, rollout_safe_kernel<32, 8, false>};
    static void (*const kl[4])(InstParams<float>, PolicyArgs, SafeArgs) = {rollout_safe_kernel<64, 4, true>, rollout_safe_kernel<64, 8, true>,
                                                                         rollout_safe_kernel<32, 4, true>, rollout_safe_kernel<32, 8, true>};
    static scg::PerDeviceOnce attr;         // (both placements' attributes on the first call; a placement that does not fit gets the other's size)
    int attr_dev;
    if (attr.pending(&attr_dev)) {
        for (int il = 0; il < 2; ++il) {
            const int b4 = S::bytes(4, il) <= SAFE_LDS_BUDGET ? S::bytes(4, il) : S::bytes(4, false);
            const int b8 = S::wpw_used(8, il) == 8 ? S::bytes(8, il) : b4;
            for (int j = 0; j < 4; ++j)
                HIP_TRY(hipFuncSetAttribute((const void*)(il ? kl : kg)[j], hipFuncAttributeMaxDynamicSharedMemorySize, j & 1 ? b8 : b4));
        }
        attr.commit(attr_dev);
    }
    const int per_wg = g.epw * g.wpw;
    (in_lds ? kl : kg)[(g.epw == 64 ? 0 : 2) + (g.wpw == 4 ? 0 : 1)]<<<dim3((env->cfg.num_envs + per_wg - 1) / per_wg), dim3(64 * g.wpw),
                                                                     (size_t)S::bytes(g.wpw, in_lds), (hipStream_t)stream>>>(inst_of<float>(env), A, B);
    HIP_TRY(hipGetLastError());
    return SCG_OK;
#else
    (void)d_safety; (void)d_slack; (void)deterministic; (void)k_steps; (void)d_c_rows; (void)d_c_carry; (void)stream;
    return fail(SCG_ERR_INVALID, "scg_rollout_safe serves float32 envs");
#endif
}

// Safe-Explorer pre-training: the random-action transition collector and the fused constraint-model update (include/scg_safe_pretrain.h)
#include "scg_safe_pretrain.h"

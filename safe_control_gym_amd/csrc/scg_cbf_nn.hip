// scg_cbf_nn.hip — libscg_cbfnn_<spechash>_<H>_<act>.so: the CBF-QP safety filter with a learned correction of the Lie derivative
// (include/scg_cbf_nn.h) as a batched certify kernel and as the policy rollout with the residual network and the filter between the
// actor and the env step, next to everything libscg_spec_<hash>.so carries and the plain filter's batched certify (scg_cbf_certify).
//
// Built only as   hipcc ... -DSCG_SPEC -include <spec header> -DSCG_POLICY_H=<H> -DSCG_POLICY_ACT=<act> scg_cbf_nn.hip
// (safe_control_gym_amd/_cbf_nn.py).  The simulator's translation unit is included whole, without any edit to it; the closed form of
// the QP is the one copy in scg_cbf_core.h (cbf_row + cbf_solve; cbf_nn_certify adds the residual to the row).  The residual network
// MLP(4 -> 256 -> 256 -> 2) runs on scg_mlp_rows.h: 8 waves per workgroup, wave w keeps rows 32 w .. 32 w + 31 of W2 in registers, a
// 32-row column tile is computed by all 8 waves together.  Both kernels follow that header's rule: every one of the 512 threads makes
// every mlp_rows_forward call.  Trip counts are workgroup-uniform (kernel arguments and blockIdx only), nothing returns early, a
// surplus tile shadows the last row / env and stores nothing.
//
//   cbf_nn_certify_kernel   8 column tiles per workgroup (256 rows), grid-stride over row chunks so that W2 is read once per workgroup
//   rollout_cbf_nn_kernel   rollout_actor_wide_kernel's step loop (scg_actor_rollout_wide.h) with G = 1 | 8 stepping waves; the
//                           stepping wave forms its action from PPO's actor (an MlpLds image behind the row-split image, the EPW = 32
//                           lane mapping, scg_rollout_policy's Gaussian head) or from the uniform draw, all 8 waves run the residual
//                           forward, the stepping wave certifies, blends and steps
#include "scg_kernels.hip"

#if !defined(SCG_SPEC) || !defined(SCG_POLICY_H)
#error "scg_cbf_nn.hip is built with -DSCG_SPEC -include <spec header> -DSCG_POLICY_H= -DSCG_POLICY_ACT="
#endif
#define SCG_CBF_HIDDEN SCG_POLICY_H
#define SCG_CBF_ACTIVATION SCG_POLICY_ACT
#include "scg_cbf_core.h"

#include "../../include/scg_cbf_nn.h"
#include "scg_mlp_rows.h"

// ---- the entry points of scg_cbf.h this library does not serve ---------------------------------------------------------------------
extern "C" int scg_rollout_cbf(scg_env* env, const scg_actor_ptrs* actor, const scg_cbf_params* params, int deterministic, int k_steps,
                               const scg_policy_rollout* out, float* d_filter_rows, float* d_applied, void* stream) {
    (void)env; (void)actor; (void)params; (void)deterministic; (void)k_steps; (void)out; (void)d_filter_rows; (void)d_applied; (void)stream;
    return fail(SCG_ERR_INVALID, "scg_rollout_cbf is served by the plain filter's library (_cbf.build); this one carries scg_rollout_cbf_nn");
}
extern "C" int scg_rollout_cbf_actor(scg_env* env, const scg_actor* actor, const scg_cbf_params* params, int k_steps, const scg_policy_rollout* out,
                                     float* d_filter_rows, float* d_applied, void* stream) {
    (void)env; (void)actor; (void)params; (void)k_steps; (void)out; (void)d_filter_rows; (void)d_applied; (void)stream;
    return fail(SCG_ERR_INVALID, "no SAC / DDPG actor in front of the cbf_nn filter: a 256-wide actor and the residual do not share a register file");
}

#ifdef SCG_CBF_SERVED
namespace scg {

constexpr int CBF_NN_NX = 4, CBF_NN_NOUT = 2, CBF_NN_CERT_TILES = 8;
constexpr int CBF_NN_CERT_MAX_GROUPS = 1024;        // 256 CUs, one resident workgroup each (102 KiB of LDS): four chunks' worth of queue

struct CbfNnResidual {
    const float* params; int32_t W1, b1, W2, b2, W3, b3;
    __device__ __forceinline__ MlpWeights weights() const {
        return MlpWeights{params + W1, params + b1, params + W2, params + b2, params + W3, params + b3};
    }
};

// The residual's layer-1 B operand of a state: rows row(q, h) = q + 4 h of the 8 the step covers, i.e. the state in half 0, zeros in half 1.
__device__ __forceinline__ void cbf_nn_operand(const float* X, int h, float* x) {
#pragma unroll
    for (int q = 0; q < 4; ++q) x[q] = h ? 0.0f : X[q];
}

__global__ __launch_bounds__(64 * MLP_ROWS_WAVES) void cbf_nn_certify_kernel(const scg_cbf_params p, const CbfNnResidual R,
                                                                            const float* __restrict__ state, const float* __restrict__ action,
                                                                            float* __restrict__ certified, float* __restrict__ slack,
                                                                            uint8_t* __restrict__ feasible, float* __restrict__ ab, int n) {
    constexpr int G = CBF_NN_CERT_TILES;
    static_assert(MlpRowsLds<CBF_NN_NX, CBF_NN_NOUT, G>::L1Q == 4, "one layer-1 step group covers the state");
    extern __shared__ __align__(16) float lds[];
    const int lane = threadIdx.x & 63, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float w2[MLP_ROWS_WAVES][16];
    {
        const MlpWeights w = R.weights();
        mlp_rows_load_w2(w.W2, wave, lane, w2);
        mlp_rows_fill_lds<CBF_NN_NX, CBF_NN_NOUT, G>(lds, w, threadIdx.x);
    }
    __syncthreads();
    // chunks of 256 rows: the trip count depends on blockIdx, gridDim and n only, so all 512 threads make every forward call
    for (long long base = (long long)blockIdx.x * (32 * G); base < n; base += (long long)gridDim.x * (32 * G)) {
        const long long i0 = base + 32 * wave + (lane & 31);
        const bool live = i0 < n && h == 0;
        const size_t i = (size_t)(i0 < n ? i0 : n - 1);          // a surplus row shadows the last one (it takes part in the MFMAs, never stores)
        const f32x4 xv = *reinterpret_cast<const f32x4*>(state + 4 * i);
        const float X[4] = {xv.x, xv.y, xv.z, xv.w};
        float x[4], o[CBF_NN_NOUT];
        cbf_nn_operand(X, h, x);
        mlp_rows_forward<CBF_NN_NX, CBF_NN_NOUT, MLP_ACT_RELU, MLP_ACT_RELU, G>(lds, w2, x, o, wave, lane);
        const CbfResult c = cbf_nn_certify(p, X, action[i], o[0], o[1]);
        if (live) {
            certified[i] = c.u;
            if (slack) slack[i] = c.s;
            feasible[i] = c.feasible != 0.0f ? 1 : 0;
            if (ab) { ab[2 * i] = o[0]; ab[2 * i + 1] = o[1]; }
        }
    }
}

struct CbfNnArgs {
    MlpWeights actor;
    const float* logstd;                           // [NU]
    CbfNnResidual res;
    scg_cbf_params p;
    int32_t uniform;
    float blend, low, high;                        // low / high: the action space of the uniform draw
    float* rows;                                   // [K][N][4]
    float* applied;                                // [K][N]
    float* ab;                                     // [K][N][2]
};

// LDS: the row-split image of the residual (G tiles), then the actor's image.
template <int G>
__global__ __launch_bounds__(64 * MLP_ROWS_WAVES) void rollout_cbf_nn_kernel(const InstParams<float> I, const PolicyArgs A, const CbfNnArgs B) {
    using T = float;
    constexpr int SYS = SCG_SPEC_SYS;
    constexpr bool DIST = SCG_SPEC_DIST != 0;
    using Ops = EnvOps<SYS, T, DIST, SCG_SEQ_ST_AUX>;
    using D = Dims<SYS>;
    constexpr CfgParams<T> kcfg = scg_make_spec_cfg<T>();
    constexpr int NIN = kcfg.nobs, NU = D::NU, HID = SCG_POLICY_H, ACT = SCG_POLICY_ACT;
    static_assert(NU == 1 && D::NX == CBF_NN_NX, "the CBF filter serves the cartpole (one input, four states)");
    static_assert(NIN == D::NX || NIN == 2 * D::NX, "the fused rollout serves single-row observations (goal horizon <= 1)");
    using LR = MlpRowsLds<CBF_NN_NX, CBF_NN_NOUT, G>;
    using LP = MlpLds<NIN, HID, NU, 16>;
    constexpr int L1Q = LP::L1Q;
    extern __shared__ __align__(16) float lds[];
    float* const actor_img = lds + LR::END;
    const PV<T> P{kcfg, I};
    const GoalTab<T> goal{nullptr, I.x_goal, false};
    const int lane = threadIdx.x & 63, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool uniform = B.uniform != 0;              // (kernel-uniform)
    float w2[MLP_ROWS_WAVES][16];
    {
        const MlpWeights w = B.res.weights();
        mlp_rows_load_w2(w.W2, wave, lane, w2);
        mlp_rows_fill_lds<CBF_NN_NX, CBF_NN_NOUT, G>(lds, w, threadIdx.x);
        if (!uniform) mlp_fill_lds<NIN, HID, NU, 16, 64 * MLP_ROWS_WAVES>(actor_img, B.actor, threadIdx.x);
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
    float sigma[NU] = {}, logp_const = 0.0f;
    if (stepper) {                                    // (wave-uniform; the waves w >= G hold no env: nothing to load, no row to form)
        Ops::load_state(P, i, e);
        Ops::load_params(P, i, e);
        if (A.ep_stats) seq_slot(A.ep_stats, i, 4).template load_row<4>(ep);
        if (A.episode_acc) seq_slot(A.episode_acc, i, 8).template load_row<8>(acc);
        Ops::state_vector(e, st);
        const bool fresh = e.step == 0;
        const int32_t c0 = e.step - 1;
        Ops::obs_row(P, goal, st, e, key, fresh ? 1 : c0 + 2, fresh ? 0u : (uint32_t)(c0 + 1), fresh ? 0 : c0, i, nullptr, row);
        if (!uniform) logp_const = gaussian_setup<NU>(B.logstd, sigma);
    }
    bool dirty = false;
    // k_steps is a kernel argument: every wave makes the same k_steps forward calls
    for (int t = 0; t <= A.k_steps; ++t) {
        if (live) seq_slot(A.obs + (size_t)t * N * NIN, i, NIN).template store_row<NIN>(row);
        if (t == A.k_steps) break;
        // ---- (a) the uncertified action, on the stepping waves (wave-uniform branch without a barrier inside)
        T act[NU] = {};
        float logp = 0.0f;
        if (stepper) {
            if (uniform) {                            // action_space.sample(): sac_collect_kernel's draw (Philox channel 4)
                const U4 w = rng_words(key, e.gid, e.episode, (uint32_t)e.step, rng_tag(RNG_CH_RANDOM_ACTION, 0, 0));
#pragma unroll
                for (int a = 0; a < NU; ++a) act[a] = B.low + (B.high - B.low) * u01<T>(u4_get(w, a));
            } else {                                  // scg_rollout_policy's head
                float xo[L1Q], xr[L1Q], mean[NU];
                b_operand<NIN, L1Q, 32>(row, h, xo, xr);
                mlp_forward_lanes<NIN, HID, NU, ACT, ACT, 32>(actor_img, xo, xr, lane, mean);
                logp = gaussian_action<NU>(A.deterministic != 0, key, e, RNG_CH_POLICY, sigma, mean, logp_const, act);
            }
        }
        // ---- (b) the residual: all 8 waves
        float x[4], o[CBF_NN_NOUT];
        cbf_nn_operand(row, h, x);
        mlp_rows_forward<CBF_NN_NX, CBF_NN_NOUT, MLP_ACT_RELU, MLP_ACT_RELU, G>(lds, w2, x, o, wave, lane);
        if (!stepper) continue;                       // (wave-uniform; no barrier below)
        // ---- the filter on the state the policy saw, and what the env step receives
        const float u_phys = kcfg.normalized_action ? __fmul_rn((float)kcfg.act_scale, act[0]) : act[0];
        const CbfResult c = cbf_nn_certify(B.p, row, u_phys, o[0], o[1]);
        const float u_env = kcfg.normalized_action ? __fdiv_rn(c.u, (float)kcfg.act_scale) : c.u;
        T applied[NU];
        if (B.blend < 0.0f) applied[0] = c.feasible != 0.0f ? u_env : act[0];
        else applied[0] = __fadd_rn(__fmul_rn(__fsub_rn(1.0f, B.blend), act[0]), __fmul_rn(B.blend, u_env));
        const size_t tn = (size_t)t * N + i;
        if (live) {
            f32x4 v;
            v.x = c.u0; v.y = c.u; v.z = c.s; v.w = c.feasible;
            *reinterpret_cast<f32x4*>(B.rows + 4 * tn) = v;
            B.applied[tn] = applied[0];
            B.ab[2 * tn] = o[0]; B.ab[2 * tn + 1] = o[1];
        }
        // ---- the control step (identical code to scg_step's kernel)
        const int32_t c0 = e.step;
        T noisy[NU];
        typename Ops::StepResult r = Ops::step(P, goal, e, applied, nullptr, key, i, st, noisy, seq_slot((T*)nullptr, 0), 0);
        if (live) store_step_row<NU, true>(A.act, A.logp, A.reward, A.done, A.flags, tn, act, logp, r);
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

constexpr int CBF_NN_LDS_LIMIT = 160 * 1024;
template <int G>
constexpr int cbf_nn_rollout_lds() {
    return (MlpRowsLds<CBF_NN_NX, CBF_NN_NOUT, G>::END + MlpLds<scg_make_spec_cfg<float>().nobs, SCG_POLICY_H, 1, 16>::END) * (int)sizeof(float);
}
constexpr bool CBF_NN_FITS_1 = cbf_nn_rollout_lds<1>() <= CBF_NN_LDS_LIMIT, CBF_NN_FITS_8 = cbf_nn_rollout_lds<8>() <= CBF_NN_LDS_LIMIT;

// Column tiles per workgroup: scg_actor_rollout_wide.h's rule (G = 1 up to 32 768 envs, G = 8 above; SCG_ROLLOUT_WIDE_TILES=1|8 overrides
// it for measurements); an actor whose image does not fit beside the G = 8 row-split image runs G = 1 at every N.
constexpr int CBF_NN_G1_MAX_ENVS = 32768;
static int cbf_nn_tiles(int num_envs) {
    int g = num_envs <= CBF_NN_G1_MAX_ENVS ? 1 : 8;
    if (const char* o = getenv("SCG_ROLLOUT_WIDE_TILES")) { if (atoi(o) == 1 || atoi(o) == 8) g = atoi(o); }
    return CBF_NN_FITS_8 ? g : 1;
}

static int cbf_nn_check_residual(const scg_cbf_residual* r, CbfNnResidual* R) {
    if (!r->d_params) return fail(SCG_ERR_INVALID, "scg_cbf_residual: d_params is NULL");
    if (r->hidden != SCG_CBF_NN_HIDDEN) return fail(SCG_ERR_INVALID, "scg_cbf_residual: the residual network served is 4 -> 256 -> 256 -> 2");
    if ((uintptr_t)r->d_params & 3) return fail(SCG_ERR_INVALID, "scg_cbf_residual: d_params must be 4-byte aligned");
    const scg_mlp_layout& m = r->mlp;
    if (m.W1 < 0 || m.b1 < 0 || m.W2 < 0 || m.b2 < 0 || m.W3 < 0 || m.b3 < 0)
        return fail(SCG_ERR_INVALID, "scg_cbf_residual: negative tensor offset");
    *R = CbfNnResidual{r->d_params, m.W1, m.b1, m.W2, m.b2, m.W3, m.b3};
    return SCG_OK;
}

// scg_rollout_cbf_nn after the NULL checks.  A template so that a geometry whose LDS need exceeds a CU's is not instantiated at all.
template <bool FITS1, bool FITS8>
static int cbf_nn_rollout(scg_env* env, const scg_actor_ptrs* actor, const scg_cbf_params* params, const scg_cbf_residual* residual,
                          const scg_cbf_nn_mode* mode, int k_steps, const scg_policy_rollout* out, float* d_filter_rows, float* d_applied,
                          float* d_ab, void* stream) {
    if constexpr (!FITS1) {
        (void)actor; (void)k_steps; (void)d_filter_rows; (void)d_applied; (void)d_ab; (void)stream;
        return fail(SCG_ERR_INVALID, "the actor's image and the residual's do not fit a CU's LDS together: no fused cbf_nn rollout for this actor shape");
    } else {
        if (k_steps <= 0) return fail(SCG_ERR_INVALID, "k_steps must be positive");
        if (!env->has_reset) return fail(SCG_ERR_STATE, "scg_reset (all envs) must be called before scg_rollout_cbf_nn");
        const bool uniform = mode->uniform != 0;
        if (!uniform && (!actor || !actor->W1 || !actor->b1 || !actor->W2 || !actor->b2 || !actor->W3 || !actor->b3 || !actor->logstd))
            return fail(SCG_ERR_INVALID, "the actor has a NULL parameter pointer");
        if (!(mode->blend <= 1.0f)) return fail(SCG_ERR_INVALID, "blend is negative (the evaluation rule) or a weight in [0, 1]");
        if (uniform && !(mode->act_low <= mode->act_high)) return fail(SCG_ERR_INVALID, "act_low must not exceed act_high");
        if (!d_filter_rows || !d_applied || !d_ab || !rollout_outputs_present(out, true))
            return fail(SCG_ERR_INVALID, "scg_rollout_cbf_nn needs d_filter_rows, d_applied, d_ab, d_obs, d_act, d_logp, d_reward, d_done and d_flags");
        if (!rollout_rows_aligned(out, (uintptr_t)d_filter_rows))
            return fail(SCG_ERR_INVALID, "row outputs and the filter rows must be 16-byte aligned");
        if (((uintptr_t)d_applied | (uintptr_t)d_ab) & 3) return fail(SCG_ERR_INVALID, "d_applied and d_ab must be 4-byte aligned");
        if (const int rc = cbf_check_params(params)) return rc;
        CbfNnArgs B;
        if (const int rc = cbf_nn_check_residual(residual, &B.res)) return rc;
        HIP_TRY(hipSetDevice(env->device));
        const PolicyArgs A = policy_args(out, k_steps, mode->deterministic ? 1 : 0);
        B.actor = uniform ? MlpWeights{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}
                          : MlpWeights{actor->W1, actor->b1, actor->W2, actor->b2, actor->W3, actor->b3};
        B.logstd = uniform ? nullptr : actor->logstd;
        B.p = *params; B.uniform = uniform ? 1 : 0; B.blend = mode->blend; B.low = mode->act_low; B.high = mode->act_high;
        B.rows = d_filter_rows; B.applied = d_applied; B.ab = d_ab;
        const InstParams<float> I = inst_of<float>(env);
        hipStream_t st = (hipStream_t)stream;
        static PerDeviceOnce attr;
        int attr_dev;
        if (attr.pending(&attr_dev)) {
            HIP_TRY(hipFuncSetAttribute((const void*)rollout_cbf_nn_kernel<1>, hipFuncAttributeMaxDynamicSharedMemorySize, cbf_nn_rollout_lds<1>()));
            if constexpr (FITS8)
                HIP_TRY(hipFuncSetAttribute((const void*)rollout_cbf_nn_kernel<8>, hipFuncAttributeMaxDynamicSharedMemorySize, cbf_nn_rollout_lds<8>()));
            attr.commit(attr_dev);
        }
        const int g = cbf_nn_tiles(env->cfg.num_envs), per_wg = 32 * g;
        const dim3 grid((env->cfg.num_envs + per_wg - 1) / per_wg), block(64 * MLP_ROWS_WAVES);
        if (g == 1) rollout_cbf_nn_kernel<1><<<grid, block, cbf_nn_rollout_lds<1>(), st>>>(I, A, B);
        else if constexpr (FITS8) rollout_cbf_nn_kernel<8><<<grid, block, cbf_nn_rollout_lds<8>(), st>>>(I, A, B);
        HIP_TRY(hipGetLastError());
        return SCG_OK;
    }
}

}  // namespace scg
#endif  // SCG_CBF_SERVED

extern "C" int scg_cbf_nn_shape(int32_t* hidden, int32_t* activation, int32_t* residual_hidden, int32_t* obs_dim, int32_t* act_dim) {
#ifdef SCG_CBF_SERVED
    if (hidden) *hidden = SCG_POLICY_H;
    if (activation) *activation = SCG_POLICY_ACT;
    if (residual_hidden) *residual_hidden = SCG_CBF_NN_HIDDEN;
    if (obs_dim) *obs_dim = scg::scg_make_spec_cfg<float>().nobs;
    if (act_dim) *act_dim = scg::Dims<SCG_SPEC_SYS>::NU;
#else
    if (hidden) *hidden = 0;
    if (activation) *activation = 0;
    if (residual_hidden) *residual_hidden = 0;
    if (obs_dim) *obs_dim = 0;
    if (act_dim) *act_dim = 0;
#endif
    return SCG_OK;
}

extern "C" int scg_cbf_nn_lds(int tiles, int32_t* lds_bytes) {
    if (!lds_bytes) return fail(SCG_ERR_INVALID, "scg_cbf_nn_lds needs lds_bytes");
    *lds_bytes = 0;
#ifdef SCG_CBF_SERVED
    if (tiles == 1) *lds_bytes = scg::cbf_nn_rollout_lds<1>();
    else if (tiles == 8) *lds_bytes = scg::cbf_nn_rollout_lds<8>();
    else return fail(SCG_ERR_INVALID, "tiles is 1 or 8");
#endif
    return SCG_OK;
}

extern "C" int scg_cbf_nn_certify(scg_env* env, const scg_cbf_params* params, const scg_cbf_residual* residual, const float* d_state,
                                  const float* d_action, float* d_certified, float* d_slack, uint8_t* d_feasible, float* d_ab, int n, void* stream) {
    if (!env || !params || !residual || !d_state || !d_action || !d_certified || !d_feasible)
        return fail(SCG_ERR_INVALID, "scg_cbf_nn_certify needs env, params, residual, d_state, d_action, d_certified and d_feasible");
#ifdef SCG_CBF_SERVED
    using namespace scg;
    if (n < 0) return fail(SCG_ERR_INVALID, "n must not be negative");
    if ((uintptr_t)d_state & 15) return fail(SCG_ERR_INVALID, "d_state must be 16-byte aligned");
    if (((uintptr_t)d_action | (uintptr_t)d_certified | (uintptr_t)d_slack | (uintptr_t)d_ab) & 3)
        return fail(SCG_ERR_INVALID, "d_action, d_certified, d_slack and d_ab must be 4-byte aligned");
    if (const int rc = cbf_check_params(params)) return rc;
    CbfNnResidual R;
    if (const int rc = cbf_nn_check_residual(residual, &R)) return rc;
    if (n == 0) return SCG_OK;
    HIP_TRY(hipSetDevice(env->device));
    constexpr int bytes = MlpRowsLds<CBF_NN_NX, CBF_NN_NOUT, CBF_NN_CERT_TILES>::END * (int)sizeof(float);
    static PerDeviceOnce attr;
    int attr_dev;
    if (attr.pending(&attr_dev)) {
        HIP_TRY(hipFuncSetAttribute((const void*)cbf_nn_certify_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
        attr.commit(attr_dev);
    }
    constexpr int per_wg = 32 * CBF_NN_CERT_TILES;
    const long long groups = ((long long)n + per_wg - 1) / per_wg;
    const dim3 grid((unsigned)(groups < CBF_NN_CERT_MAX_GROUPS ? groups : CBF_NN_CERT_MAX_GROUPS)), block(64 * MLP_ROWS_WAVES);
    cbf_nn_certify_kernel<<<grid, block, bytes, (hipStream_t)stream>>>(*params, R, d_state, d_action, d_certified, d_slack, d_feasible, d_ab, n);
    HIP_TRY(hipGetLastError());
    return SCG_OK;
#else
    (void)d_slack; (void)d_ab; (void)n; (void)stream;
    return fail(SCG_ERR_INVALID, "the cbf_nn filter serves float32 cartpole envs");
#endif
}

extern "C" int scg_rollout_cbf_nn(scg_env* env, const scg_actor_ptrs* actor, const scg_cbf_params* params, const scg_cbf_residual* residual,
                                  const scg_cbf_nn_mode* mode, int k_steps, const scg_policy_rollout* out, float* d_filter_rows, float* d_applied,
                                  float* d_ab, void* stream) {
    if (!env || !params || !residual || !mode || !out) return fail(SCG_ERR_INVALID, "NULL argument to scg_rollout_cbf_nn");
#ifdef SCG_CBF_SERVED
    using namespace scg;
    return cbf_nn_rollout<CBF_NN_FITS_1, CBF_NN_FITS_8>(env, actor, params, residual, mode, k_steps, out, d_filter_rows, d_applied, d_ab, stream);
#else
    (void)actor; (void)k_steps; (void)d_filter_rows; (void)d_applied; (void)d_ab; (void)stream;
    return fail(SCG_ERR_INVALID, "the cbf_nn filter serves float32 cartpole envs");
#endif
}

// scg_safe_pretrain.h — Safe-Explorer's pre-training phase (include/scg_safe_pretrain.h).  Included by scg_safe_explorer.hip after its own
// kernels, the way scg_pid.h rides in scg_ilqr.hip.
//   collect_constraints_kernel  rollout_random_kernel's loop (one thread = one env, the state in registers, the same EnvOps::step, auto-reset
//                               in the launch) that also writes the transition (obs, act, c, c_next) of every step to the caller's ring.
//   safety_update_kernel        n minibatches of SafetyLayer.update: workgroup i = constraint model i, its parameters, Adam moments and
//                               gradient in LDS for the whole launch.  Per chunk of RC minibatch rows: pass 1, one thread per row, runs the
//                               forward pass with the weights read from LDS (every lane the same address: a broadcast) and leaves the row's
//                               inputs and dL/dpred in LDS; pass 2, thread (hidden unit j, row slice s), re-forms unit j's pre-activation
//                               with the SAME fma chain and accumulates unit j's gradients over the rows r = s, s + SL, ... in registers.
//                               The SL slices of a unit are adjacent lanes: a butterfly sums them.  All of it on the vector ALU in exact
//                               float32: the work is a serial chain of small minibatches on C workgroups, where latency decides.
#ifndef SCG_CSRC_SAFE_PRETRAIN_H
#define SCG_CSRC_SAFE_PRETRAIN_H

#include "../../include/scg_safe_pretrain.h"
#include "scg_adam.h"

namespace scg {

struct CollectArgs {
    float* obs; float* act; float* c; float* c_next;
    int64_t pos, capacity;
    float low[4], high[4];
    float* c_carry; float* last_obs; float* ep_stats;
    int32_t k_steps;
};

template <int SYS, bool DIST>
__global__ __launch_bounds__(64) void collect_constraints_kernel(const InstParams<float> I, const CollectArgs A) {
    using T = float;
    using S = SafeShape;
    using Ops = EnvOps<SYS, T, DIST, SCG_SEQ_ST_AUX>;
    using D = Dims<SYS>;
    constexpr int NIN = S::NIN, NU = S::NU, NC = S::NC;
    static_assert(NIN == D::NX || NIN == 2 * D::NX, "single-row observations (goal horizon <= 1)");
    constexpr CfgParams<T> kcfg = scg_make_spec_cfg<T>();
    const PV<T> P{kcfg, I};
    const GoalTab<T> goal{nullptr, I.x_goal, false};
    const int i = I.env_first + blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= I.env_end) return;
    const int64_t N = I.num_envs;
    typename Ops::E e;
    Ops::load_state(P, i, e);
    Ops::load_params(P, i, e);
    const RngKey key{I.key0, I.key1};
    T ep[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (A.ep_stats) seq_slot(A.ep_stats, i, 4).template load_row<4>(ep);
    T st[D::NX], row[2 * D::NX];
    Ops::state_vector(e, st);
    {
        const bool fresh = e.step == 0;
        const int32_t c0 = e.step - 1;
        Ops::obs_row(P, goal, st, e, key, fresh ? 1 : c0 + 2, fresh ? 0u : (uint32_t)(c0 + 1), fresh ? 0 : c0, i, nullptr, row);
    }
    int rr = (int)((A.pos + i) % A.capacity);                 // ring row of (t, i); k_steps * N <= capacity: no two threads share one
    {
        float c[NC];
        seq_slot(A.c_carry, i, NC).template load_row<NC>(c);
        seq_slot(A.c, rr, NC).template store_row<NC>(c);
    }
    bool dirty = false;
    for (int t = 0; t < A.k_steps; ++t) {
        seq_slot(A.obs, rr, NIN).template store_row<NIN>(row);
        // actions ~ U(low, high): Philox channel 4, item 0, word j (rollout_random_kernel's draw)
        const U4 w = rng_words(key, e.gid, e.episode, (uint32_t)e.step, rng_tag(RNG_CH_RANDOM_ACTION, 0, 0));
        T act[NU], noisy[NU];
#pragma unroll
        for (int j = 0; j < NU; ++j) act[j] = A.low[j] + (A.high[j] - A.low[j]) * u01<T>(u4_get(w, j));
        seq_slot(A.act, rr, NU).template store_row<NU>(act);
        const int32_t c0 = e.step;
        const typename Ops::StepResult r = Ops::step(P, goal, e, act, nullptr, key, i, st, noisy, seq_slot((T*)nullptr, 0), 0);
        // c_next: the state rows of the post-step (where the episode ended: terminal) state
        Ops::constraints(P, st, act, seq_slot(A.c_next, rr, NC), 1, true);
        ep[0] += r.reward; ep[1] += 1.0f; ep[2] += (r.flags & FLAG_VIOLATION) ? 1.0f : 0.0f; ep[3] += r.mse;
        Ops::obs_row(P, goal, st, e, key, c0 + 2, (uint32_t)(c0 + 1), c0, i, nullptr, row);
        if (r.done) {
            ep[0] = ep[1] = ep[2] = ep[3] = 0.0f;
            if (P.c.auto_reset) {
                dirty = true;
                Ops::reset(P, i, e, key, st);
                Ops::obs_row(P, goal, st, e, key, 1, 0u, 0, i, nullptr, row);
            }
        }
        // the c of step t + 1: the state rows of whichever state the env now is in (the same values as c_next unless it was reset)
        const int rn = (int)((A.pos + (int64_t)(t + 1) * N + i) % A.capacity);
        if (t + 1 < A.k_steps) Ops::constraints(P, st, act, seq_slot(A.c, rn, NC), 1, true);
        else Ops::constraints(P, st, act, seq_slot(A.c_carry, i, NC), 1, true);
        rr = rn;
    }
    seq_slot(A.last_obs, i, NIN).template store_row<NIN>(row);
    if (A.ep_stats) seq_slot(A.ep_stats, i, 4).template store_row<4>(ep);
    Ops::store(P, i, e, dirty);
}

// row slices per hidden unit: the largest power of two <= 64 with hc * slices <= max_threads
constexpr int pretrain_slices(int hc, int max_threads) { int s = 1; while (s < 64 && hc * 2 * s <= max_threads) s *= 2; return s; }
// minibatch rows staged per chunk: 1024, halved while `fixed + rows * roww` words are over the LDS budget (32: not even 64 rows fit)
constexpr int pretrain_chunk(int fixed, int roww) {
    int rc = 1024;
    while (rc >= 64 && (fixed + rc * roww) * 4 > SAFE_LDS_BUDGET) rc /= 2;
    return rc;
}

// Compile-time shape of the update kernel.
struct PretrainShape {
    using S = SafeShape;
    static constexpr int NIN = S::NIN, NU = S::NU, NC = S::NC, HC = S::HC;
    static constexpr int P = HC * (NIN + 1 + NU) + NU, PP = (P + 3) / 4 * 4;
    static constexpr int OW1 = 0, OB1 = HC * NIN, OW2 = OB1 + HC, OB2 = OW2 + NU * HC;       // nn.Linear layout of one constraint model
    // pass 2 keeps 3 NIN values per thread (weights, their gradients, the row): wide observations run 512 threads (256 registers each)
    static constexpr int MAX_THREADS = NIN <= 12 ? 1024 : 512;
    static constexpr int SL = pretrain_slices(HC, MAX_THREADS);                     // row slices per hidden unit: a power of two <= 64 (adjacent lanes)
    static constexpr int THREADS = (HC * SL + 63) / 64 * 64, WAVES = THREADS / 64;
    static constexpr int ROWW = NIN + NU + 1;                  // one staged row: obs | act | dL/dpred
    static constexpr int FIXED = 4 * PP + 16;                  // params | m | v | grad | the waves' loss partials
    static constexpr int RC = pretrain_chunk(FIXED, ROWW);                 // minibatch rows per chunk (32: not even 64 rows fit -> not served)
    static constexpr int BYTES = (FIXED + RC * ROWW) * 4;
    static constexpr bool SERVED = RC >= 64;
};

// word `e` of `base`, written through (what a launch leaves for the next one; scg_wide.h's store_wt for single words)
__device__ __forceinline__ void pretrain_store_wt(float* base, int e, float x) { buf_st<17>(make_rsrc(base), (uint32_t)e * 4u, 0u, x); }

__global__ __launch_bounds__(PretrainShape::THREADS) void safety_update_kernel(const scg_safety_update_args a) {
    using Q = PretrainShape;
    constexpr int NIN = Q::NIN, NU = Q::NU, NC = Q::NC, HC = Q::HC, P = Q::P, PP = Q::PP, SL = Q::SL, TH = Q::THREADS, RC = Q::RC;
    extern __shared__ __align__(16) float lds[];
    float* const p = lds;
    float* const m = p + PP;
    float* const v = m + PP;
    float* const g = v + PP;
    float* const red = g + PP;
    float* const xs = red + 16;                                // [RC][NIN]
    float* const as = xs + RC * NIN;                           // [RC][NU]
    float* const es = as + RC * NU;                            // [RC]
    const int ci = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const bool train = a.train != 0;
    const size_t po = (size_t)ci * P;
    for (int e = tid; e < P; e += TH) {
        p[e] = a.d_params[po + e];
        if (train) { m[e] = a.d_m[po + e]; v[e] = a.d_v[po + e]; }
    }
    float step = train ? a.d_steps[ci] : 0.0f;
    __syncthreads();
    const int j = tid / SL, s = tid % SL;
    const bool unit = j < HC;
    const int B = a.batch;
    const float scale = 2.0f / (float)B;
    for (int mb = 0; mb < a.n_batches; ++mb) {
        const int32_t* rows = a.d_rows + (size_t)mb * B;
        float lsum = 0.0f;
        float w1[NIN], w2[NU], b1j = 0.0f, gw1[NIN], gw2[NU], gb2[NU], gb1 = 0.0f;
#pragma unroll
        for (int k = 0; k < NIN; ++k) { w1[k] = unit ? p[Q::OW1 + j * NIN + k] : 0.0f; gw1[k] = 0.0f; }
#pragma unroll
        for (int o = 0; o < NU; ++o) { w2[o] = unit ? p[Q::OW2 + o * HC + j] : 0.0f; gw2[o] = 0.0f; gb2[o] = 0.0f; }
        if (unit) b1j = p[Q::OB1 + j];
        for (int base = 0; base < B; base += RC) {
            const int nr = B - base < RC ? B - base : RC;
            // ---- pass 1: the forward pass of row r, its squared error and dL/dpred = 2 (pred - c_next) / B
            for (int r = tid; r < nr; r += TH) {
                const size_t row = (size_t)rows[base + r];
                float x[NIN], ac[NU], gg[NU];
#pragma unroll
                for (int k = 0; k < NIN; ++k) x[k] = a.d_obs[row * NIN + k];
#pragma unroll
                for (int o = 0; o < NU; ++o) { ac[o] = a.d_act[row * NU + o]; gg[o] = p[Q::OB2 + o]; }
                const float c = a.d_c[row * NC + ci], cn = a.d_c_next[row * NC + ci];
#pragma unroll 2
                for (int u = 0; u < HC; ++u) {
                    float pre = p[Q::OB1 + u];
#pragma unroll
                    for (int k = 0; k < NIN; ++k) pre = __builtin_fmaf(p[Q::OW1 + u * NIN + k], x[k], pre);
                    const float h = fmaxf(pre, 0.0f);
#pragma unroll
                    for (int o = 0; o < NU; ++o) gg[o] = __builtin_fmaf(p[Q::OW2 + o * HC + u], h, gg[o]);
                }
                float pred = c;
#pragma unroll
                for (int o = 0; o < NU; ++o) pred = __builtin_fmaf(gg[o], ac[o], pred);
                const float d = pred - cn;
                lsum = __builtin_fmaf(d, d, lsum);
                if (train) {
#pragma unroll
                    for (int k = 0; k < NIN; ++k) xs[r * NIN + k] = x[k];
#pragma unroll
                    for (int o = 0; o < NU; ++o) as[r * NU + o] = ac[o];
                    es[r] = __fmul_rn(d, scale);
                }
            }
            if (!train) continue;
            __syncthreads();
            // ---- pass 2: hidden unit j's gradients over the rows of slice s (the pre-activation by pass 1's fma chain: the same bits)
            if (unit) {
                for (int r = s; r < nr; r += SL) {
                    float x[NIN];
#pragma unroll
                    for (int k = 0; k < NIN; ++k) x[k] = xs[r * NIN + k];
                    const float e = es[r];
                    float pre = b1j;
#pragma unroll
                    for (int k = 0; k < NIN; ++k) pre = __builtin_fmaf(w1[k], x[k], pre);
                    const bool on = pre > 0.0f;
                    const float h = on ? pre : 0.0f;
                    float sa = 0.0f;
#pragma unroll
                    for (int o = 0; o < NU; ++o) {
                        const float dg = __fmul_rn(e, as[r * NU + o]);
                        gw2[o] = __builtin_fmaf(dg, h, gw2[o]);
                        sa = __builtin_fmaf(dg, w2[o], sa);
                        if (j == 0) gb2[o] += dg;
                    }
                    const float dh = on ? sa : 0.0f;
                    gb1 += dh;
#pragma unroll
                    for (int k = 0; k < NIN; ++k) gw1[k] = __builtin_fmaf(dh, x[k], gw1[k]);
                }
            }
            __syncthreads();
        }
        // ---- the minibatch's loss: a butterfly inside each wave, the wave partials in wave order
#pragma unroll
        for (int off = 1; off < 64; off *= 2) lsum += __shfl_xor(lsum, off, 64);
        if (lane == 0) red[tid >> 6] = lsum;
        __syncthreads();
        if (tid == 0) {
            float tot = 0.0f;
            for (int w = 0; w < Q::WAVES; ++w) tot += red[w];
            a.d_loss[(size_t)mb * NC + ci] = tot / (float)B;
        }
        if (train) {
            // ---- the slices of a unit are SL adjacent lanes: a butterfly leaves the full sums in each of them
#pragma unroll
            for (int off = 1; off < SL; off *= 2) {
#pragma unroll
                for (int k = 0; k < NIN; ++k) gw1[k] += __shfl_xor(gw1[k], off, 64);
#pragma unroll
                for (int o = 0; o < NU; ++o) { gw2[o] += __shfl_xor(gw2[o], off, 64); gb2[o] += __shfl_xor(gb2[o], off, 64); }
                gb1 += __shfl_xor(gb1, off, 64);
            }
            if (unit && s == 0) {
#pragma unroll
                for (int k = 0; k < NIN; ++k) g[Q::OW1 + j * NIN + k] = gw1[k];
                g[Q::OB1 + j] = gb1;
#pragma unroll
                for (int o = 0; o < NU; ++o) g[Q::OW2 + o * HC + j] = gw2[o];
                if (j == 0) {
#pragma unroll
                    for (int o = 0; o < NU; ++o) g[Q::OB2 + o] = gb2[o];
                }
            }
            __syncthreads();
            step += 1.0f;
            for (int e = tid; e < P; e += TH) adam_element(p[e], g[e], m[e], v[e], a.lr, step);
        }
        __syncthreads();
    }
    if (!train) return;
    for (int e = tid; e < P; e += TH) {
        pretrain_store_wt(a.d_params + po, e, p[e]);
        pretrain_store_wt(a.d_m + po, e, m[e]);
        pretrain_store_wt(a.d_v + po, e, v[e]);
        if (a.d_grad) pretrain_store_wt(a.d_grad + po, e, g[e]);
    }
    if (tid == 0) pretrain_store_wt(a.d_steps, ci, step);
}

}  // namespace scg

extern "C" int scg_safe_pretrain_lds(int32_t* bytes) {
    if (bytes) *bytes = scg::PretrainShape::BYTES;
    return SCG_OK;
}

extern "C" int scg_collect_constraints(scg_env* env, int k_steps, const scg_collect_io* io, void* stream) {
    using namespace scg;
    using S = SafeShape;
    if (!env || !io) return fail(SCG_ERR_INVALID, "NULL argument to scg_collect_constraints");
#if SCG_SPEC_DTYPE == 0
    if (k_steps <= 0) return fail(SCG_ERR_INVALID, "k_steps must be positive");
    if (!env->has_reset) return fail(SCG_ERR_STATE, "scg_reset (all envs) must be called before scg_collect_constraints");
    if (!io->d_obs || !io->d_act || !io->d_c || !io->d_c_next || !io->d_c_carry || !io->d_last_obs)
        return fail(SCG_ERR_INVALID, "scg_collect_constraints needs d_obs, d_act, d_c, d_c_next, d_c_carry and d_last_obs");
    if (((uintptr_t)io->d_obs | (uintptr_t)io->d_act | (uintptr_t)io->d_c | (uintptr_t)io->d_c_next | (uintptr_t)io->d_c_carry |
         (uintptr_t)io->d_last_obs | (uintptr_t)io->d_ep_stats) & 15)
        return fail(SCG_ERR_INVALID, "the ring arrays, d_c_carry, d_last_obs and d_ep_stats must be 16-byte aligned");
    const int64_t n = env->cfg.num_envs;
    if (io->capacity <= 0 || io->pos < 0 || io->pos >= io->capacity) return fail(SCG_ERR_INVALID, "scg_collect_constraints: 0 <= pos < capacity");
    if ((int64_t)k_steps * n > io->capacity)
        return fail(SCG_ERR_INVALID, "scg_collect_constraints: k_steps * num_envs exceeds the ring's capacity (two envs would write one row)");
    if (io->capacity * 4 * (int64_t)(S::NIN > S::NC ? S::NIN : S::NC) >= (int64_t)1 << 32)
        return fail(SCG_ERR_INVALID, "scg_collect_constraints: a ring array exceeds the 32-bit byte offsets");
    HIP_TRY(hipSetDevice(env->device));
    CollectArgs A;
    A.obs = io->d_obs; A.act = io->d_act; A.c = io->d_c; A.c_next = io->d_c_next;
    A.pos = io->pos; A.capacity = io->capacity;
    for (int j = 0; j < 4; ++j) { A.low[j] = io->low[j]; A.high[j] = io->high[j]; }
    A.c_carry = io->d_c_carry; A.last_obs = io->d_last_obs; A.ep_stats = io->d_ep_stats;
    A.k_steps = k_steps;
    const InstParams<float> I = inst_of<float>(env);
    const int grid = (env->cfg.num_envs + 63) / 64;
    collect_constraints_kernel<SCG_SPEC_SYS, SCG_SPEC_DIST != 0><<<dim3(grid), dim3(64), 0, (hipStream_t)stream>>>(I, A);
    HIP_TRY(hipGetLastError());
    return SCG_OK;
#else
    (void)k_steps; (void)stream;
    return fail(SCG_ERR_INVALID, "scg_collect_constraints serves float32 envs");
#endif
}

extern "C" int scg_safety_update(const scg_safety_update_args* args, void* stream) {
    using namespace scg;
    using Q = PretrainShape;
    if (!args) return fail(SCG_ERR_INVALID, "NULL argument to scg_safety_update");
#if SCG_SPEC_DTYPE == 0
    if constexpr (!Q::SERVED) {
        (void)stream;
        return fail(SCG_ERR_INVALID, "scg_safety_update: this safety-layer shape needs more than 163840 B of LDS per workgroup");
    } else {
        const scg_safety_update_args& a = *args;
        if (a.n_batches <= 0 || a.batch <= 0) return fail(SCG_ERR_INVALID, "scg_safety_update: n_batches and batch must be positive");
        if (!a.d_params || !a.d_obs || !a.d_act || !a.d_c || !a.d_c_next || !a.d_rows || !a.d_loss)
            return fail(SCG_ERR_INVALID, "scg_safety_update needs d_params, d_obs, d_act, d_c, d_c_next, d_rows and d_loss");
        if (a.train && (!a.d_m || !a.d_v || !a.d_steps)) return fail(SCG_ERR_INVALID, "scg_safety_update: training needs d_m, d_v and d_steps");
        if ((int64_t)Q::NC * Q::P * 4 >= (int64_t)1 << 32) return fail(SCG_ERR_INVALID, "scg_safety_update: the parameter buffer exceeds 32-bit offsets");
        static scg::PerDeviceOnce attr;
        int attr_dev;
        if (attr.pending(&attr_dev)) {
            HIP_TRY(hipFuncSetAttribute((const void*)safety_update_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, Q::BYTES));
            attr.commit(attr_dev);
        }
        safety_update_kernel<<<dim3(Q::NC), dim3(Q::THREADS), Q::BYTES, (hipStream_t)stream>>>(a);
        HIP_TRY(hipGetLastError());
        return SCG_OK;
    }
#else
    (void)stream;
    return fail(SCG_ERR_INVALID, "scg_safety_update serves float32 envs");
#endif
}

#endif  // SCG_CSRC_SAFE_PRETRAIN_H

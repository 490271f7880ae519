// scg_offpolicy_step.h — what the fused SAC and DDPG gradient steps share beyond the wide-tile passes of scg_wide.h: the critic kernel
// (a DDPG step is a SAC step with one critic, no log-prob and no temperature), the step's argument block, the fixed pairing that ends the sums of the
// reductions, the replay ring's bookkeeping and the host helpers of the two C ABIs.  What differs for good reasons stays in scg_sac.hip
// and scg_ddpg.hip: the actor kernels (tanh-Gaussian head against a plain tanh), the owners' bookkeeping in the reductions, the step
// sequences.  An edit here makes both libraries stale (_sac.DEPS, _ddpg.DEPS).
// Include after scg_wide.h and after the library's own fail() and HIP_TRY (they name the library in its error text).
#pragma once
#include <cstdint>
#include <string>

#include "scg_wide.h"

namespace scg {
namespace wide {

// ------------------------------------------------------------------ kernels
struct Common {
    const int32_t* idx; int batch; int n_part;
    const float* obs; const float* act; const float* rew; const float* next_obs; const float* mask;
    float low[4], high[4];
#ifdef SCG_STEP_TEMPERATURE                     // (defined by scg_sac.hip.  Not a null pointer in DDPG's blocks: every kernel's argument
    const float* log_alpha;                     //  bytes are fetched at its entry, and words nobody reads cost time — see ALG::Nets)
#endif                                          // device scalar (d_params + n_params)
    float gamma;
    uint32_t k0, k1; const uint32_t* counter;
};

// Q networks of algorithm ALG (scg_sac.hip: SacCritics, scg_ddpg.hip: DdpgCritic):
//   ALG::NCRIT    critics y = 0 .. NCRIT - 1 (2 or 1): q_out, qo, dqda and the stored tiles are [NCRIT][B]...; with one critic y is the constant 0
//   ALG::Nets     the critics' layouts, by value, and layout(Nets, y).  One layout per critic and no more: with DDPG's one layout passed
//                 twice and a null log_alpha in Common, every DDPG launch that takes them ran 40 - 160 ns longer behind its larger
//                 argument block (instruction streams equal but for the argument offsets), 0.7 % of a step
//   ALG::TgtArgs  what the target needs beyond reward and mask, by value (SAC: qt, logp_next; DDPG: qt)
//   ALG::Tgt      load(TgtArgs, r, B): the loads of batch row r;  init(Common): once, behind the first barrier;
//                 value(Common, rew, mask): the critic loss's target
//   MODE 0: forward only, blockIdx.y = y + NCRIT * online:
//             online = 0: TARGET network y at (next_obs[idx], a_in[row])          -> q_out[y][row]
//             online = 1: ONLINE network y at (obs[idx], act[idx])                -> qo[y][row] and the waves' h1 / h2 tiles, for MODE 2
//           (the second kind does not depend on the first: it is the forward half of the critic loss, run here next to the targets
//            instead of behind them)
//   MODE 1: online networks at (obs[idx], a_in[row]), data gradient       -> q_out[y][row], dqda[y][row][NU]; blockIdx.y = y
//   MODE 2: backward only, blockIdx.y = y: d mean (q - target)^2 / d(theta_y) into the workgroups' partials, q = qo[y][row] and the
//           stored tiles
// No barrier ends a tile of the forward-only loop: forward() has two.  A wave writes H1X of tile t + 1 only behind barrier 2 of tile t,
// which every reader of H1X of tile t has reached, and RED of tile t + 1 only behind barrier 1 of tile t + 1, which every reader of RED
// of tile t has reached.  backward()'s exchange buffers need the trailing barrier of MODE 1 and MODE 2.
struct QAct { float* qo; float* h1s; float* h2s; float* rew; float* mask; };     // [NCRIT][B], [NCRIT][B / 32 tiles][NT][1024] each, [B], [B]
template <int MODE, class ALG>
__global__ __launch_bounds__(64 * NT, MODE == 0 ? 2 : 1) void q_kernel(const float* __restrict__ params, const float* __restrict__ params_online,
                                                        const typename ALG::Nets nets, const Common Cm, const float* __restrict__ a_in, const typename ALG::TgtArgs TA,
                                                        float* __restrict__ q_out, float* __restrict__ dqda, const QAct QA,
                                                        float* __restrict__ partials) {
    using S = Small<1>;
    using G = Part<NQ, 1>;
    constexpr int L1Q = 4 * ((NQ + 7) / 8);
    constexpr bool TWO = ALG::NCRIT == 2;
    static_assert(ALG::NCRIT == 1 || ALG::NCRIT == 2, "one critic or two");
    extern __shared__ __align__(16) float lds[];
    const int y = TWO ? blockIdx.y & 1 : 0;
    const bool online = MODE == 0 && (TWO ? blockIdx.y >> 1 : blockIdx.y);
    const MlpWeights w = weights_of(online ? params_online : params, ALG::layout(nets, y));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 31, h = lane >> 5;
    const int n_tiles = Cm.batch / 32, B = Cm.batch;
    const int tile0 = blockIdx.x, r0 = tile0 * 32 + c;
    const int s0 = Cm.idx[r0];                                          // (gridDim.x <= n_tiles; unconditional: see actor_grad_kernel)
    SmallRegs<1> sr;
    small_load<1>(sr, w, threadIdx.x);
    float* const xch = lds + S::END;
    if constexpr (MODE == 2) {
        // ---- backward only.  Request order: row index, small block, the tiles and the row's values, the data-gradient operand
        float bt[NT][16];
        const float* const h1s = QA.h1s + (size_t)y * B * HID;
        const float* const h2s = QA.h2s + (size_t)y * B * HID;
        f32x16 h1, h2;
        float x[L1Q], v_rew = 0.0f, v_mask = 0.0f, v_q = 0.0f;
        typename ALG::Tgt T;
        // (reward and mask by BATCH row, left by q_kernel<0>'s online blocks: nothing the loss derivative needs waits for the row index)
        auto load_row = [&](int tile, int r) {
            act_load(h1s, tile, wave, lane, h1); act_load(h2s, tile, wave, lane, h2);
            v_q = QA.qo[(size_t)y * B + r]; T.load(TA, r, B);
            v_rew = QA.rew[r]; v_mask = QA.mask[r];
        };
        auto load_in = [&](int s) { load_x2<L1Q, NOBS, NU>(Cm.obs + (size_t)s * NOBS, Cm.act + (size_t)s * NU, h, x); };
        load_row(tile0, r0);
        load_bt(w.W2, wave, lane, bt);                                  // (see actor_grad_kernel)
        load_in(s0);
        small_store<1>(lds, sr, threadIdx.x);
        __syncthreads();
        float* const P = partials + ((size_t)y * Cm.n_part + blockIdx.x) * PSTRIDE;
        T.init(Cm);
        const float inv_b = 1.0f / (float)B;
        float st = 0.0f;
        bool first = true;
        for (int tile = tile0; tile < n_tiles; tile += gridDim.x) {
            const int r = tile * 32 + c;
            if (tile != tile0) { load_row(tile, r); load_in(Cm.idx[r]); }
            const float target = T.value(Cm, v_rew, v_mask);
            const float e = v_q - target;
            const float dout[1] = {2.0f * e * inv_b};
            if (wave == 0 && h == 0) st += e * e * inv_b;
            backward<NQ, 1, ACT, true, false>(lds, xch, bt, h1, h2, dout, wave, lane, P, first, nullptr, x);
            first = false;
            __syncthreads();                                            // the exchange buffers are free for the next tile
        }
        if (wave == 0) {                                                // (st lives in the lanes of half 0)
            const float v = row_sum32(xch + Xch::WAVE + TR_WORDS + 34 * 32, st, lane);
            if (lane == 0) { P[G::STAT] = v; P[G::STAT + 1] = 0.0f; }
        }
    } else {
        // request order (see small_load): the first tile's row index, the small block, the forward operands, the row's values;
        // the backward operand (bt) is requested behind the barrier and arrives under the forward pass
        float w1a[(NU * HID + 64 * NT - 1) / (64 * NT)];
        if constexpr (MODE == 1) {                                      // W1A[j][f] = W1[f][NOBS + j]
#pragma unroll
            for (int j = 0; j < (NU * HID + 64 * NT - 1) / (64 * NT); ++j) {
                const int k = threadIdx.x + j * 64 * NT;
                w1a[j] = k < NU * HID ? w.W1[(size_t)(k % HID) * NQ + NOBS + k / HID] : 0.0f;
            }
        }
        float a1[L1Q], a2[NT][16];
        load_a1<NQ, L1Q>(w.W1, wave, lane, a1);
        load_a2(w.W2, wave, lane, a2);
        float x[L1Q], v_rew = 0.0f, v_mask = 0.0f;
        auto load_row = [&](int r, int s) {
            if constexpr (MODE == 0) {
                if (online) {
                    load_x2<L1Q, NOBS, NU>(Cm.obs + (size_t)s * NOBS, Cm.act + (size_t)s * NU, h, x);
                    if (y == 0) { v_rew = Cm.rew[s]; v_mask = Cm.mask[s]; }
                } else load_x2<L1Q, NOBS, NU>(Cm.next_obs + (size_t)s * NOBS, a_in + (size_t)r * NU, h, x);
            } else {
                load_x2<L1Q, NOBS, NU>(Cm.obs + (size_t)s * NOBS, a_in + (size_t)r * NU, h, x);
            }
        };
        load_row(r0, s0);
        small_store<1>(lds, sr, threadIdx.x);
        if constexpr (MODE == 1) {
#pragma unroll
            for (int j = 0; j < (NU * HID + 64 * NT - 1) / (64 * NT); ++j) {
                const int k = threadIdx.x + j * 64 * NT;
                if (k < NU * HID) lds[S::W1A + k] = w1a[j];
            }
        }
        __syncthreads();
        float bt[MODE == 1 ? NT : 1][16];
        if constexpr (MODE == 1) load_bt(w.W2, wave, lane, bt);
        for (int tile = tile0; tile < n_tiles; tile += gridDim.x) {
            const int r = tile * 32 + c;
            if (tile != tile0) load_row(r, Cm.idx[r]);
            f32x16 h1, h2;
            float out[1];
            forward<NQ, 1, ACT>(lds, xch, a1, a2, x, wave, lane, h1, h2, out);
            if constexpr (MODE == 0) {
                if (online) {
                    act_store(QA.h1s + (size_t)y * B * HID, tile, wave, lane, h1);
                    act_store(QA.h2s + (size_t)y * B * HID, tile, wave, lane, h2);
                    if (wave == 0 && h == 0) QA.qo[(size_t)y * B + r] = out[0];
                    if (wave == 1 % NT && h == 0 && y == 0) { QA.rew[r] = v_rew; QA.mask[r] = v_mask; }
                } else if (wave == 0 && h == 0) {
                    q_out[(size_t)y * B + r] = out[0];
                }
            } else {
                const float dout[1] = {1.0f};
                float din[NU];
                backward<NQ, 1, ACT, false, true>(lds, xch, bt, h1, h2, dout, wave, lane, nullptr, true, din);
                if (wave == 0 && h == 0) {
                    q_out[(size_t)y * B + r] = out[0];
#pragma unroll
                    for (int j = 0; j < NU; ++j) dqda[((size_t)y * B + r) * NU + j] = din[j];
                }
                __syncthreads();                                        // the exchange buffers are free for the next tile
            }
        }
    }
}

}  // namespace wide

// ---- the reductions' sum of one partial word, in a fixed order (the bitwise contract of both steps): thread group g = 0 .. 3 sums
// partials g, g + 4, ... (the loop of each reduce_kernel), then the word's owner pairs the four sums, `stride` words apart at p.
__device__ __forceinline__ float pair_sum(const float* p, int stride) { return (p[0] + p[stride]) + (p[2 * stride] + p[3 * stride]); }

// The ring's write position, fill counts and counter word behind ring_push_kernel (scg_wide.h), whose every thread reads the
// position: one thread of a launch of its own.
__device__ __forceinline__ void ring_advance(const RingArgs& R, int n) {
    *R.pos = (*R.pos + n) % R.capacity;
    if (R.size_f) *R.size_f = fminf(*R.size_f + (float)n, (float)R.capacity);
    if (R.size_i) *R.size_i = min(*R.size_i + n, R.capacity);
    if (R.counter) *R.counter += 1u;
}

// ------------------------------------------------------------------ host side
static int n_part_of(int batch) { const int t = batch / 32; return t < 512 ? t : 512; }

template <typename K>
static int set_lds(K kernel, size_t bytes) {
    HIP_TRY(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return 0;
}

static size_t wide_lds_actor() { return (wide::Small<NA>::END + wide::Xch::END) * sizeof(float); }
static size_t wide_lds_q() { return (wide::Small<1>::END + wide::Xch::END) * sizeof(float); }
// forward-only launches need the small block, the h1 exchange and the output partials only: two workgroups per CU fit
static size_t wide_lds_actor_fwd() { return (wide::Small<NA>::END + wide::Xch::FWD_END) * sizeof(float); }
static size_t wide_lds_q_fwd() { return (wide::Small<1>::END + wide::Xch::FWD_END) * sizeof(float); }

// Args: scg_sac_args or scg_ddpg_args (the fields read here have the same names in both).
template <class Args>
static int check_step_args(const Args* a, const char* who) {
    if (!a || !a->d_params || !a->d_target || !a->d_grad || !a->d_m || !a->d_v || !a->d_steps || !a->d_obs || !a->d_act || !a->d_rew ||
        !a->d_next_obs || !a->d_mask || !a->d_counter || !a->d_workspace || !a->d_stats || (!a->d_ring_size && !a->d_idx_in))
        return fail(-1, std::string(who) + ": NULL argument");
    if (a->batch <= 0 || a->batch % 32) return fail(-1, std::string(who) + ": the batch size must be a positive multiple of 32");
    return 0;
}
template <class Args>
static void fill_common(wide::Common& Cm, const Args* a, const int32_t* idx, int n_part) {
    Cm.idx = idx; Cm.batch = a->batch; Cm.n_part = n_part; Cm.obs = a->d_obs; Cm.act = a->d_act; Cm.rew = a->d_rew; Cm.next_obs = a->d_next_obs;
    Cm.mask = a->d_mask; Cm.gamma = a->gamma;
    for (int j = 0; j < 4; ++j) { Cm.low[j] = a->act_low[j]; Cm.high[j] = a->act_high[j]; }
    Cm.k0 = (uint32_t)a->seed; Cm.k1 = (uint32_t)(a->seed >> 32); Cm.counter = a->d_counter;
}

// the first NU action bounds as the collector kernels take them (the rest zero)
static void pack_bounds(const float* act_low, const float* act_high, float4& l4, float4& h4) {
    float lo[4] = {0, 0, 0, 0}, hi[4] = {0, 0, 0, 0};
    for (int j = 0; j < NU; ++j) { lo[j] = act_low[j]; hi[j] = act_high[j]; }
    l4 = make_float4(lo[0], lo[1], lo[2], lo[3]); h4 = make_float4(hi[0], hi[1], hi[2], hi[3]);
}

// Ring: scg_sac_ring or scg_ddpg_ring (the same fields).
template <class Ring>
static RingArgs ring_args_of(const Ring* ring) {
    return RingArgs{ring->d_obs, ring->d_act, ring->d_rew, ring->d_next_obs, ring->d_mask, ring->capacity, (long long*)ring->d_pos, ring->d_size_f,
                    ring->d_size_i32, ring->d_counter};
}
// The argument check and the ring_push_kernel launch of the two *_push exports; R: the ring as the caller's one-thread launch behind it
// (scg_sac.hip: ring_advance_kernel; scg_ddpg.hip: bookkeeping_kernel, with the noise commit) takes it.
template <class Ring>
static int launch_ring_push(const Ring* ring, float* d_cur_obs, const float* d_act, const float* d_reward, const float* d_next_obs,
                            const float* d_terminal_obs, const uint8_t* d_done, const uint8_t* d_flags, int n, hipStream_t st, const char* who,
                            RingArgs& R) {
    if (!ring || !ring->d_obs || !ring->d_act || !ring->d_rew || !ring->d_next_obs || !ring->d_mask || !ring->d_pos || !d_cur_obs || !d_act ||
        !d_reward || !d_next_obs || !d_terminal_obs || !d_done || !d_flags)
        return fail(-1, std::string(who) + ": NULL argument");
    if (n <= 0 || ring->capacity < n) return fail(-1, std::string(who) + ": replay capacity smaller than one vectorised step");
    R = ring_args_of(ring);
    const int total = n * NOBS;
    ring_push_kernel<<<dim3((total + 255) / 256), dim3(256), 0, st>>>(R, d_cur_obs, d_act, d_reward, d_next_obs, d_terminal_obs, d_done, d_flags, n);
    return 0;
}

}  // namespace scg

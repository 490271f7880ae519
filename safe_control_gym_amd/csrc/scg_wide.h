// scg_wide.h — the wide-tile MLP passes of the fused off-policy gradient steps, and the collector kernels the off-policy agents
// share: the one home of the scheme, included by libscg_sac_* (scg_sac.hip) and libscg_ddpg_* (scg_ddpg.hip).  What differs between
// the algorithms — the actor kernels and loss heads, the reductions' bookkeeping, the step sequences — stays in the two .hip files;
// what the steps share on top of these passes (the critic kernel, the host helpers) is scg_offpolicy_step.h.  An edit here makes
// both libraries stale (_sac.DEPS, _ddpg.DEPS).
// Include AFTER defining the network constants: NOBS, HID, NU, ACT, NQ (= NOBS + NU), NA (actor head width), NT (= HID / 32),
// and SCG_S_STAMP (a no-op outside scg_sac.hip's timing builds).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/scg_learn.h"
#include "scg_mlp.h"
#include "scg_rng.h"

namespace scg {

__host__ __device__ static inline MlpWeights weights_of(const float* p, const scg_mlp_layout& L) {
    return MlpWeights{p + L.W1, p + L.b1, p + L.W2, p + L.b2, p + L.W3, p + L.b3};
}

// ------------------------------------------------------------------ partial gradient vector of one wave
template <int NIN, int NOUT>
struct Part {
    static constexpr int DW1 = 0;                           // [NIN + 1][H]: column NIN is db1
    static constexpr int DB2 = DW1 + (NIN + 1) * HID;
    static constexpr int DW3 = DB2 + HID;                   // [NOUT][H]
    static constexpr int DB3 = DW3 + NOUT * HID;            // [8]
    static constexpr int STAT = DB3 + 8;                    // [4]
    static constexpr int DW2 = STAT + 4;                    // [NT * NT tiles][4 g][64 lanes][4]: accumulator word q = 4 g + r of lane
    static constexpr int END = DW2 + HID * HID;
};
constexpr int PSTRIDE = (Part<NOBS, NA>::END > Part<NQ, 1>::END ? Part<NOBS, NA>::END : Part<NQ, 1>::END);

// (a branch on the wave-uniform `first`, not a select: the select form LOADS the partial word on every call — a global round trip per
//  output row in the dW3 phase of a workgroup's only tile, tools/sac_timeline.py)
__device__ __forceinline__ void padd(float* p, float v, bool first) {
    if (first) *p = v;
    else *p += v;
}

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// 16-byte store WRITTEN THROUGH (sc0 sc1, as scg_learn.hip's partial vectors): what a launch leaves for the NEXT launch — partial gradient
// vectors, activation tiles — is read there from other XCDs, so it has to reach the memory side before this kernel may retire; written
// back, that is one flush of megabytes behind the last workgroup's last store, written through it drains while the kernel still computes.
// `base` must be wave-uniform (it becomes the buffer resource); `word` = this lane's float offset from it.
#ifndef SCG_S_STORE_AUX
#define SCG_S_STORE_AUX 17
#endif
typedef unsigned int u32x4 __attribute__((vector_size(16)));
__device__ __forceinline__ void store_wt(float* base, uint32_t word, const f32x4 v) {
    const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, 0xffffffff, 0x00020000);
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), r, 4u * word, 0, SCG_S_STORE_AUX);
}

// Sum over lanes 0..31 of v, valid in lane 0: through 32 words of the wave's LDS (one 4-byte write per lane, eight 16-byte reads in lane 0,
// a fixed order) — a butterfly over the lanes is 5-6 dependent ds_bpermute round trips.
__device__ __forceinline__ float row_sum32(float* row, float v, int lane) {
    if (lane < 32) row[lane] = v;
    wave_sync();
    float s = 0.0f;
    if (lane == 0) {
#pragma unroll
        for (int g = 0; g < 8; ++g) {
            const f32x4 d4 = *reinterpret_cast<const f32x4*>(row + 4 * g);
            s += d4.x; s += d4.y; s += d4.z; s += d4.w;
        }
    }
    return s;
}

// x[q] = input feature row(q, h) of one sample, the input being [a [NA_] | b [NB_]] (rows >= NA_ + NB_ are zero)
template <int L1Q, int NA_, int NB_>
__device__ __forceinline__ void load_x2(const float* __restrict__ a, const float* __restrict__ b, int h, float* x) {
#pragma unroll
    for (int q = 0; q < L1Q; ++q) {
        const int f0 = d_row(q, 0), f1 = d_row(q, 1);           // compile-time after unrolling
        const float v0 = f0 < NA_ ? a[f0 < NA_ ? f0 : 0] : (f0 < NA_ + NB_ ? b[f0 < NA_ + NB_ && f0 >= NA_ ? f0 - NA_ : 0] : 0.0f);
        const float v1 = f1 < NA_ ? a[f1 < NA_ ? f1 : 0] : (f1 < NA_ + NB_ ? b[f1 < NA_ + NB_ && f1 >= NA_ ? f1 - NA_ : 0] : 0.0f);
        x[q] = h ? v1 : v0;
    }
}

// batch row r of this update: a replay-ring slot ~ U[0, ring size) (or the caller's, for tests)
__device__ __forceinline__ int sample_row(int r, const int32_t* __restrict__ ring_size, const int32_t* __restrict__ idx_in, uint32_t cnt,
                                          uint32_t k0, uint32_t k1) {
    if (idx_in) return idx_in[r];
    const uint32_t n = (uint32_t)max(*ring_size, 1);
    const U4 w = philox4x32_10(U4{cnt, (uint32_t)r, 0u, 0x5ac0u}, k0, k1);
    return (int32_t)int_below(w.x, n);
}

// N(0,1) draws for one batch row: Box-Muller on a Philox block (stream: 1 policy-loss action, 2 target action)
__device__ __forceinline__ void normal4(uint32_t cnt, uint32_t row, uint32_t stream, uint32_t k0, uint32_t k1, float* n) {
    const U4 w = philox4x32_10(U4{cnt, row, stream, 0x5ac1u}, k0, k1);
    const float r0 = sqrtf(-2.0f * __logf(u01<float>(w.x))), r1 = sqrtf(-2.0f * __logf(u01<float>(w.z)));
    float s0, c0, s1, c1;
    __sincosf(6.283185307179586f * u01<float>(w.y), &s0, &c0);
    __sincosf(6.283185307179586f * u01<float>(w.w), &s1, &c1);
    n[0] = r0 * c0; n[1] = r0 * s0; n[2] = r1 * c1; n[3] = r1 * s1;
}

// ================================================================== wide tiles
// A batch of 4096 is only 128 tiles.  The NT waves of a workgroup SHARE one tile: wave w owns the hidden features
// [32 w, 32 w + 32) of both layers, the activations cross an LDS exchange between the layers, and every wave's dependent MFMA
// chain is 1 / NT of the network's.  Each weight is then used by exactly one wave, once per tile: the MFMA operands are read from
// the parameter vector straight into registers (no LDS image, no fill) — only W3 and the biases sit in the LDS.
//   forward :  L1 (own 32 features) -> h1 tile to H1X -> barrier -> L2 (A = own rows of W2, B = all h1 tiles) -> own partial of the
//              output layer to RED -> barrier -> every wave sums the NT partials (fixed order)
//   backward:  dW3 / db2 / dz2 on the own tile; dz2 tile to DZX, own h1 tile transposed to H1T -> barrier ->
//              data gradient of the OWN input-feature tile (all dz2 tiles x own columns of W2; computed transposed when it feeds
//              dW1 — scg_learn.hip's trick — plain when it feeds dq/da), dW1 | db1 slice, the dW2 tiles [all tau][rho = w]
//              (A = H1T tiles, B = own dz2^T)
// Partial gradient vectors: one per workgroup, word order of Part<> (dW2 in the accumulator's [tile][lane][q] order).
namespace wide {
constexpr int XW = 20, XT = 64 * XW;                    // an exchanged tile: 16 words per lane, padded to 20 (conflict-free 16-byte access)
// LDS of a wide-tile kernel = [Small<NOUT> of each network it evaluates][Xch]: the per-network constants and ONE set of exchange
// buffers shared by the networks a workgroup walks through one after the other (workgroup barrier in between).
template <int NOUT>
struct Small {
    static constexpr int W3 = 0;                                        // [NOUT][H]
    static constexpr int B1 = W3 + NOUT * HID, B2 = B1 + HID, B3 = B2 + HID;   // b3: [8]
    static constexpr int W1A = B3 + 8;                                  // [4][H]    W1's action columns (Q networks, dq/da)
    static constexpr int END = W1A + 4 * HID;
    static_assert(NOUT <= 8 && (END % 4) == 0, "layout");
};
struct Xch {
    static constexpr int H1X = 0;                                       // [NT][XT]  h1 tiles, accumulator layout (lane = sample)
    static constexpr int RED = H1X + NT * XT;                           // [NT][8][32] per-wave partial outputs
    static constexpr int FWD_END = RED + NT * 8 * 32;
    static constexpr int DZX = FWD_END;                                 // [NT][XT]  dz2 tiles, accumulator layout
    static constexpr int H1T = DZX + NT * XT;                           // [NT][XT]  h1 tiles transposed (lane = feature)
    static constexpr int DIN = H1T + NT * XT;                           // [NT][4][32] per-wave partial input gradients
    static constexpr int WAVE = DIN + NT * 4 * 32;                      // per wave: scr | xs | dout_l
    static constexpr int WAVE_WORDS = TR_WORDS + 34 * 32 + 8 * 32;
    static constexpr int END = WAVE + NT * WAVE_WORDS;
};

// W3 and the biases of one network -> LDS (all threads; caller barriers), in two halves: the REQUESTS (small_load) go out first in a
// kernel, the LDS writes (small_store) after the other requests of the prologue have been issued — the memory counter retires in
// order, so the barrier behind the stores then waits for this handful of loads only, not for the ~150 operand loads behind them
// (tools/sac_timeline.py: 3.6 us from kernel entry to the first barrier when the small block was requested last).
template <int NOUT>
struct SmallRegs { float w3[(NOUT * HID + 64 * NT - 1) / (64 * NT)]; float b1, b2, b3; };
template <int NOUT>
__device__ __forceinline__ void small_load(SmallRegs<NOUT>& R, const MlpWeights& w, int tid) {
    constexpr int IT = (NOUT * HID + 64 * NT - 1) / (64 * NT);
#pragma unroll
    for (int j = 0; j < IT; ++j) { const int k = tid + j * 64 * NT; R.w3[j] = k < NOUT * HID ? w.W3[k] : 0.0f; }
    static_assert(HID <= 64 * NT * 2, "one bias word per thread and layer");
    R.b1 = tid < HID ? w.b1[tid] : 0.0f;
    R.b2 = tid < HID ? w.b2[tid] : 0.0f;
    R.b3 = tid < NOUT ? w.b3[tid] : 0.0f;
}
template <int NOUT>
__device__ __forceinline__ void small_store(float* lds, const SmallRegs<NOUT>& R, int tid) {     // lds = the network's Small<NOUT> block
    using S = Small<NOUT>;
    constexpr int IT = (NOUT * HID + 64 * NT - 1) / (64 * NT);
#pragma unroll
    for (int j = 0; j < IT; ++j) { const int k = tid + j * 64 * NT; if (k < NOUT * HID) lds[S::W3 + k] = R.w3[j]; }
    if (tid < HID) { lds[S::B1 + tid] = R.b1; lds[S::B2 + tid] = R.b2; }
    if (tid < 8) lds[S::B3 + tid] = R.b3;
}

// MFMA operands of wave `wave` from the torch-layout parameters:
//   a1[q]      = W1[32 wave + i][row(q, h)]                  A operand of layer 1            (i = lane & 31, h = lane >> 5)
//   a2[tau][q] = W2[32 wave + i][32 tau + row(q, h)]         A operand of layer 2
//   bt[rho][q] = W2[32 rho + row(q, h)][32 wave + i]         operand of the data gradient of the own input tile
template <int NIN, int L1Q>
__device__ __forceinline__ void load_a1(const float* __restrict__ W1, int wave, int lane, float* a1) {
    const int i = lane & 31, h = lane >> 5;
#pragma unroll
    for (int q = 0; q < L1Q; ++q) {
        const int f = d_row(q, 0) + 4 * h;
        a1[q] = f < NIN ? W1[(size_t)(32 * wave + i) * NIN + (f < NIN ? f : 0)] : 0.0f;
    }
}
__device__ __forceinline__ void load_a2(const float* __restrict__ W2, int wave, int lane, float (&a2)[NT][16]) {
    const int i = lane & 31, h = lane >> 5;
    const float* row = W2 + (size_t)(32 * wave + i) * HID + 4 * h;
    if ((reinterpret_cast<uintptr_t>(W2) & 15) == 0) {
#pragma unroll
        for (int tau = 0; tau < NT; ++tau)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(row + 32 * tau + 8 * g);
                a2[tau][4 * g] = v.x; a2[tau][4 * g + 1] = v.y; a2[tau][4 * g + 2] = v.z; a2[tau][4 * g + 3] = v.w;
            }
    } else {
#pragma unroll
        for (int tau = 0; tau < NT; ++tau)
#pragma unroll
            for (int q = 0; q < 16; ++q) a2[tau][q] = row[32 * tau + d_row(q, 0)];
    }
}
__device__ __forceinline__ void load_bt(const float* __restrict__ W2, int wave, int lane, float (&bt)[NT][16]) {
    const int i = lane & 31, h = lane >> 5;
#pragma unroll
    for (int rho = 0; rho < NT; ++rho)
#pragma unroll
        for (int q = 0; q < 16; ++q) bt[rho][q] = W2[(size_t)(32 * rho + d_row(q, h)) * HID + 32 * wave + i];
}

__device__ __forceinline__ void put_tile(float* slot, const f32x16& t) {          // slot = base + lane * XW
#pragma unroll
    for (int g = 0; g < 4; ++g) *reinterpret_cast<f32x4*>(slot + 4 * g) = (f32x4){t[4 * g], t[4 * g + 1], t[4 * g + 2], t[4 * g + 3]};
}
__device__ __forceinline__ void get_tile(const float* slot, float* t) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(slot + 4 * g);
        t[4 * g] = v.x; t[4 * g + 1] = v.y; t[4 * g + 2] = v.z; t[4 * g + 3] = v.w;
    }
}

// Forward pass of the workgroup's tile: h1, h2 = this wave's feature tile of each hidden layer (accumulator layout), out = the
// network outputs of this lane's sample (every wave, both lane halves).  Two workgroup barriers.
template <int NIN, int NOUT, int ACT2>
__device__ __forceinline__ void forward(const float* sm, float* xch, const float* a1, const float (&a2)[NT][16], const float* x, int wave, int lane,
                                        f32x16& h1, f32x16& h2, float* out) {
    using S = Small<NOUT>;
    using X = Xch;
    constexpr int L1Q = 4 * ((NIN + 7) / 8);
    const int c = lane & 31, h = lane >> 5;
    f32x16 acc;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const f32x4 b = *reinterpret_cast<const f32x4*>(sm + S::B1 + 32 * wave + 8 * g + 4 * h);
        acc[4 * g] = b.x; acc[4 * g + 1] = b.y; acc[4 * g + 2] = b.z; acc[4 * g + 3] = b.w;
    }
#pragma unroll
    for (int q = 0; q < L1Q; ++q) acc = mfma32(a1[q], x[q], acc);
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = mlp_act<ACT>(acc[q]);
    h1 = acc;
    put_tile(xch + X::H1X + wave * XT + lane * XW, h1);
    __syncthreads();
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const f32x4 b = *reinterpret_cast<const f32x4*>(sm + S::B2 + 32 * wave + 8 * g + 4 * h);
        acc[4 * g] = b.x; acc[4 * g + 1] = b.y; acc[4 * g + 2] = b.z; acc[4 * g + 3] = b.w;
    }
#pragma unroll
    for (int tau = 0; tau < NT; ++tau) {
        float hb[16];
        get_tile(xch + X::H1X + tau * XT + lane * XW, hb);
#pragma unroll
        for (int q = 0; q < 16; ++q) acc = mfma32(a2[tau][q], hb[q], acc);
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = mlp_act<ACT2>(acc[q]);
    h2 = acc;
    // (all outputs' partial sums first, then the NOUT lane-half exchanges back to back: written per output — sum, exchange, store — the
    //  exchanges were NOUT dependent LDS round trips in a row, 8 for the actor's head)
    float so[NOUT];
#pragma unroll
    for (int o = 0; o < NOUT; ++o) {
        float s = 0.0f;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 w = *reinterpret_cast<const f32x4*>(sm + S::W3 + o * HID + 32 * wave + 8 * g + 4 * h);
            s = __builtin_fmaf(w.x, h2[4 * g], s); s = __builtin_fmaf(w.y, h2[4 * g + 1], s);
            s = __builtin_fmaf(w.z, h2[4 * g + 2], s); s = __builtin_fmaf(w.w, h2[4 * g + 3], s);
        }
        so[o] = s;
    }
    float sx[NOUT];
#pragma unroll
    for (int o = 0; o < NOUT; ++o) sx[o] = __shfl_xor(so[o], 32, 64);
    if (h == 0) {
#pragma unroll
        for (int o = 0; o < NOUT; ++o) xch[X::RED + (wave * 8 + o) * 32 + c] = so[o] + sx[o];
    }
    __syncthreads();
#pragma unroll
    for (int o = 0; o < NOUT; ++o) {
        float s = sm[S::B3 + o];
#pragma unroll
        for (int w = 0; w < NT; ++w) s += xch[X::RED + (w * 8 + o) * 32 + c];
        out[o] = s;
    }
}

// the wave's own sample cache for the dW1 product: xs[column][sample], a ones row and a zeros row behind the inputs
template <int NIN, int L1Q>
__device__ __forceinline__ void cache_x(float* xs, const float* x, int c, int h) {
#pragma unroll
    for (int q = 0; q < L1Q; ++q) {
        const int f = d_row(q, 0);
        if (f + 4 < NIN) xs[(f + 4 * h) * 32 + c] = x[q];
        else if (f < NIN) { if (h == 0) xs[f * 32 + c] = x[q]; }
    }
    if (h == 0) { xs[NIN * 32 + c] = 1.0f; xs[(NIN + 1) * 32 + c] = 0.0f; }
}

// Backward pass of the workgroup's tile (see the scheme above).  h1, h2: this wave's tiles from forward(); dout: d loss / d out of
// this lane's sample (identical in every wave).  WGRAD: this wave's slices of the weight / bias gradients into the workgroup's
// partial vector P;  DIN: din[j] = d loss / d input[NIN - NU + j] of this lane's sample (every wave).  One workgroup barrier
// (two with DIN); the caller barriers before the next tile's forward().
template <int NIN, int NOUT, int ACT2, bool WGRAD, bool DIN, int TL = -1>
__device__ __forceinline__ void backward(const float* sm, float* xch, const float (&bt)[NT][16], f32x16& h1, f32x16& h2,
                                         const float* dout, int wave, int lane, float* P, bool first, float* din, const float* xin = nullptr) {
    using S = Small<NOUT>;
    using X = Xch;
    using G = Part<NIN, NOUT>;
    const int c = lane & 31, h = lane >> 5;
    float* const wl = xch + X::WAVE + wave * X::WAVE_WORDS;
    float* const scr = wl; float* const xs = wl + TR_WORDS; float* const dout_l = xs + 34 * 32;
    float zt[16];                                                       // dz2^T of the own tile (WGRAD)
    if constexpr (WGRAD) {
        if (h == 0) {
#pragma unroll
            for (int o = 0; o < NOUT; ++o) dout_l[o * 32 + c] = dout[o];
        }
        wave_sync();
        // db3: lane o of the LAST wave sums row o of the LDS copy (8 x 16-byte reads, a fixed order).  (As a butterfly over the lanes it was
        // 5 dependent ds_bpermute round trips per output, and the branches of the stores in between kept the compiler from overlapping the
        // outputs' chains: 40 in a row for the actor's head — ~2 us in front of the workgroup barrier, tools/sac_timeline.py.)
        if (wave == NT - 1 && lane < NOUT) {
            float v = 0.0f;
#pragma unroll
            for (int g = 0; g < 8; ++g) {
                const f32x4 d4 = *reinterpret_cast<const f32x4*>(dout_l + lane * 32 + 4 * g);
                v += d4.x; v += d4.y; v += d4.z; v += d4.w;
            }
            padd(P + G::DB3 + lane, v, first);
        }
        float t[16];
        tile_transpose(scr, h2, t, lane);                               // t[q] = h2[feature 32 wave + c][sample row(q, h)]
        float a3[NOUT];                                                 // dW3[o][f] = sum_s h2[f][s] dout[o][s]: all outputs, then the exchanges
#pragma unroll
        for (int o = 0; o < NOUT; ++o) {
            float acc = 0.0f;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 dv = *reinterpret_cast<const f32x4*>(dout_l + o * 32 + 8 * g + 4 * h);
                acc = __builtin_fmaf(t[4 * g], dv.x, acc); acc = __builtin_fmaf(t[4 * g + 1], dv.y, acc);
                acc = __builtin_fmaf(t[4 * g + 2], dv.z, acc); acc = __builtin_fmaf(t[4 * g + 3], dv.w, acc);
            }
            a3[o] = acc;
        }
        float x3[NOUT];
#pragma unroll
        for (int o = 0; o < NOUT; ++o) x3[o] = __shfl_xor(a3[o], 32, 64);
        if (h == 0) {
            float* const p3 = P + G::DW3 + 32 * wave + c;
            if (first) {
#pragma unroll
                for (int o = 0; o < NOUT; ++o) p3[o * HID] = a3[o] + x3[o];
            } else {
#pragma unroll
                for (int o = 0; o < NOUT; ++o) p3[o * HID] += a3[o] + x3[o];
            }
        }
    }
    if constexpr (TL >= 0) SCG_S_STAMP(TL, 4);
    // dz2 = (W3^T dout) * act2'(h2), in place
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        float dh[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int o = 0; o < NOUT; ++o) {
            const f32x4 wv = *reinterpret_cast<const f32x4*>(sm + S::W3 + o * HID + 32 * wave + 8 * g + 4 * h);
            dh[0] = __builtin_fmaf(wv.x, dout[o], dh[0]); dh[1] = __builtin_fmaf(wv.y, dout[o], dh[1]);
            dh[2] = __builtin_fmaf(wv.z, dout[o], dh[2]); dh[3] = __builtin_fmaf(wv.w, dout[o], dh[3]);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) h2[4 * g + r] = dh[r] * mlp_dact<ACT2>(h2[4 * g + r]);
    }
    put_tile(xch + X::DZX + wave * XT + lane * XW, h2);
    if constexpr (WGRAD) {
        tile_transpose(scr, h2, zt, lane);                              // dz2[out 32 wave + c][sample row(q, h)]
        float sb = 0.0f;
#pragma unroll
        for (int q = 0; q < 16; ++q) sb += zt[q];
        sb += __shfl_xor(sb, 32, 64);
        if (h == 0) padd(P + G::DB2 + 32 * wave + c, sb, first);
        tile_transpose_inplace(scr, h1, lane);                          // h1[in 32 wave + c][sample row(q, h)]
        put_tile(xch + X::H1T + wave * XT + lane * XW, h1);
    }
    if constexpr (WGRAD) {
        // the tile's input rows -> the wave's sample cache (dW1's operand).  Here, not at the top of the tile: the rows are an index -> row
        // gather, two dependent memory round trips that nothing in front of this point has to wait for
        constexpr int L1Q = 4 * ((NIN + 7) / 8);
        cache_x<NIN, L1Q>(xs, xin, c, h);
    }
    if constexpr (TL >= 0) SCG_S_STAMP(TL, 5);
    __syncthreads();
    if constexpr (TL >= 0) SCG_S_STAMP(TL, 6);
    // data gradient of the own input tile: dh1[32 wave + .] = sum over rho of W2[32 rho + ., 32 wave + .]^T dz2[rho]
    f32x16 acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
#pragma unroll
    for (int rho = 0; rho < NT; ++rho) {
        float za[16];
        get_tile(xch + X::DZX + rho * XT + lane * XW, za);
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            if constexpr (WGRAD) acc = mfma32(za[q], bt[rho][q], acc);  // transposed: [sample row(q', h)][feature 32 wave + c]
            else acc = mfma32(bt[rho][q], za[q], acc);                  // plain:      [feature row(q', h)][sample c]
        }
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] *= mlp_dact<ACT>(h1[q]);       // h1 is transposed exactly when acc is
    if constexpr (TL >= 0) SCG_S_STAMP(TL, 7);
    if constexpr (DIN) {
        // d loss / d (action inputs): this wave's 32 features, then the waves' partials through the LDS
        static_assert(!WGRAD, "the input gradient is taken from the plain data gradient");
        float sj[NU], xj[NU];
#pragma unroll
        for (int j = 0; j < NU; ++j) {
            float s = 0.0f;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 wv = *reinterpret_cast<const f32x4*>(sm + S::W1A + j * HID + 32 * wave + 8 * g + 4 * h);
                s = __builtin_fmaf(wv.x, acc[4 * g], s); s = __builtin_fmaf(wv.y, acc[4 * g + 1], s);
                s = __builtin_fmaf(wv.z, acc[4 * g + 2], s); s = __builtin_fmaf(wv.w, acc[4 * g + 3], s);
            }
            sj[j] = s;
        }
#pragma unroll
        for (int j = 0; j < NU; ++j) xj[j] = __shfl_xor(sj[j], 32, 64);
        if (h == 0) {
#pragma unroll
            for (int j = 0; j < NU; ++j) xch[X::DIN + (wave * 4 + j) * 32 + c] = sj[j] + xj[j];
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NU; ++j) {
            float s = 0.0f;
#pragma unroll
            for (int w = 0; w < NT; ++w) s += xch[X::DIN + (w * 4 + j) * 32 + c];
            din[j] = s;
        }
    }
    if constexpr (WGRAD) {
        // dW1 | db1 slice: [dz1 tile (own 32 features x 32 samples)] x [x | 1]; D[feature row(q', h)][column c]
        {
            const float* const xrow = xs + (c < NIN + 1 ? c : NIN + 1) * 32 + 4 * h;
            float xb[16];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(xrow + 8 * g);
                xb[4 * g] = v.x; xb[4 * g + 1] = v.y; xb[4 * g + 2] = v.z; xb[4 * g + 3] = v.w;
            }
            f32x16 g1;
#pragma unroll
            for (int q = 0; q < 16; ++q) g1[q] = 0.0f;
#pragma unroll
            for (int q = 0; q < 16; ++q) g1 = mfma32(acc[q], xb[q], g1);
            if (c <= NIN) {
                const uint32_t dw = G::DW1 + c * HID + 32 * wave + 4 * h;
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    f32x4 v = {g1[4 * g], g1[4 * g + 1], g1[4 * g + 2], g1[4 * g + 3]};
                    if (!first) v += *reinterpret_cast<const f32x4*>(P + dw + 8 * g);
                    store_wt(P, dw + 8 * g, v);
                }
            }
        }
        if constexpr (TL >= 0) SCG_S_STAMP(TL, 8);
        // dW2 tiles (in 32 tau.., out 32 wave..) = h1^T[tau] x dz2^T[own] over this tile's samples
#pragma unroll
        for (int tau = 0; tau < NT; ++tau) {
            float ta[16];
            get_tile(xch + X::H1T + tau * XT + lane * XW, ta);
            f32x16 d2;
#pragma unroll
            for (int q = 0; q < 16; ++q) d2[q] = 0.0f;
#pragma unroll
            for (int q = 0; q < 16; ++q) d2 = mfma32(ta[q], zt[q], d2);
            const uint32_t dw = G::DW2 + ((tau * NT + wave) * 4 * 64 + lane) * 4;        // [tile][g][lane][4]: 1 KB of consecutive addresses per store
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f32x4 v = {d2[4 * g], d2[4 * g + 1], d2[4 * g + 2], d2[4 * g + 3]};
                if (!first) v += *reinterpret_cast<const f32x4*>(P + dw + 256 * g);
                store_wt(P, dw + 256 * g, v);
            }
        }
    }
}

// ---- a wave's activation tiles across launches.  The forward pass that FEEDS a gradient kernel runs in the launch before it (the actor
// at obs: actor_fwd_kernel; the critics at (obs, act): q_kernel<0>'s online blocks), which leaves every wave's h1 / h2 tile — accumulator
// layout, read back by the same (tile, wave, lane) — in the workspace: [tile][wave][g][lane][4], 16-byte accesses, 1 KB per instruction.
// The gradient kernels then START at the loss derivatives: no operand loads for the forward products, no forward pass, no tanh-Gaussian
// algebra on their critical path (round 6's timeline of actor_grad_kernel: 4.8 + 1.5 of the 18.9 us a wave lived).
__device__ __forceinline__ void act_store(float* __restrict__ base, int tile, int wave, int lane, const f32x16& t) {
    const uint32_t word = (uint32_t)((tile * NT + wave) * 4 * 64 + lane) * 4u;
#pragma unroll
    for (int g = 0; g < 4; ++g) store_wt(base, word + 256u * g, (f32x4){t[4 * g], t[4 * g + 1], t[4 * g + 2], t[4 * g + 3]});
}
__device__ __forceinline__ void act_load(const float* __restrict__ base, int tile, int wave, int lane, f32x16& t) {
    const float* const p = base + (((size_t)tile * NT + wave) * 4 * 64 + lane) * 4;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(p + g * 256);
        t[4 * g] = v.x; t[4 * g + 1] = v.y; t[4 * g + 2] = v.z; t[4 * g + 3] = v.w;
    }
}
}  // namespace wide

// Word k of a partial vector (Part<NIN, NOUT>) -> its element of the flat gradient (torch parameter order); -1: padding,
// -2 - j: statistics word j.  The reduction launches sum the workgroups' partials through it.
template <int NIN, int NOUT>
__device__ __forceinline__ int dest_of(int k, const scg_mlp_layout& lay) {
    using G = Part<NIN, NOUT>;
    if (k < G::DB2) { const int in = k / HID, o = k % HID; return in < NIN ? lay.W1 + o * NIN + in : lay.b1 + o; }
    if (k < G::DW3) return lay.b2 + (k - G::DB2);
    if (k < G::DB3) return lay.W3 + (k - G::DW3);
    if (k < G::STAT) return (k - G::DB3) < NOUT ? lay.b3 + (k - G::DB3) : -1;
    if (k < G::DW2) return -2 - (k - G::STAT);
    const int p = k - G::DW2;                               // [tile][g][lane][4]
    const int q = 4 * ((p >> 8) & 3) + (p & 3), lane = (p >> 2) & 63, tr = p >> 10;
    const int tau = tr / NT, rho = tr % NT;
    return lay.W2 + (32 * rho + (lane & 31)) * HID + 32 * tau + d_row(q, lane >> 5);
}

// ================================================================== collector (the agents' env-facing half)
// warm-up actions: action_space.sample() per env (sac.py:276-277), a ~ U[low, high) per dimension.  `pending` (nullable): DDPG's count
// of envs whose exploration noise awaits its commit — a uniform action draws none.
__global__ __launch_bounds__(256) void uniform_action_kernel(int m, float4 low, float4 high, uint32_t k0, uint32_t k1,
                                                              const uint32_t* __restrict__ counter, int32_t* __restrict__ pending,
                                                              float* __restrict__ a_out) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (pending && s == 0) *pending = 0;
    if (s >= m) return;
    const float lo[4] = {low.x, low.y, low.z, low.w}, hi[4] = {high.x, high.y, high.z, high.w};
    const U4 w = philox4x32_10(U4{counter ? *counter : 0u, (uint32_t)s, 4u, 0x5ac1u}, k0, k1);
    const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
    for (int j = 0; j < NU; ++j) a_out[(size_t)s * NU + j] = lo[j] + (hi[j] - lo[j]) * u01<float>(ww[j]);
}

// One vectorised env step into the replay ring (SACBuffer.push with the time-limit fix-up of sac.py:287-305, ddpg.py:293-311): row
// pos + i (mod capacity) <- (obs the action was taken at, action, reward, next observation — the TERMINAL observation where the episode
// was truncated by the time limit —, mask = 1 if truncated else 1 - done); the persistent current-observation batch becomes the
// step's observation.  One thread per (env, observation element).  The write position is read here by everybody and advanced by the
// one-thread launch behind it (scg_sac.hip: ring_advance_kernel; scg_ddpg.hip: bookkeeping_kernel, with the noise commit).
struct RingArgs {
    float* obs; float* act; float* rew; float* next_obs; float* mask; int capacity;
    long long* pos; float* size_f; int32_t* size_i; uint32_t* counter;
};
__global__ __launch_bounds__(256) void ring_push_kernel(const RingArgs R, float* __restrict__ cur_obs, const float* __restrict__ act,
                                                         const float* __restrict__ rew, const float* __restrict__ next,
                                                         const float* __restrict__ term, const uint8_t* __restrict__ done,
                                                         const uint8_t* __restrict__ flags, int n) {
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= n * NOBS) return;
    const int i = gid / NOBS, e = gid - i * NOBS;
    const size_t slot = (size_t)((*R.pos + i) % R.capacity);
    const bool dn = done[i] != 0, trunc = dn && (flags[i] & 1);
    const float nv = next[gid];
    R.obs[slot * NOBS + e] = cur_obs[gid];
    R.next_obs[slot * NOBS + e] = trunc ? term[gid] : nv;
    cur_obs[gid] = nv;
    for (int j = e; j < NU; j += NOBS) R.act[slot * NU + j] = act[(size_t)i * NU + j];     // every action column, also when NOBS < NU
    if (e == 0) { R.rew[slot] = rew[i]; R.mask[slot] = trunc ? 1.0f : (dn ? 0.0f : 1.0f); }
}

}  // namespace scg

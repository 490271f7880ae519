// scg_mlp_rows.h — the forward pass of a two-hidden-layer MLP of hidden width 256 on the CDNA4 matrix cores, exact float32, for callers
// whose workgroup is 8 waves.  Nothing here knows about envs or rollouts: a caller hands in the B operands of 32-sample column tiles
// and gets the NOUT outputs of each sample back.
//
// Why another layout than scg_mlp.h's: MlpLds<NIN, 256, NOUT, 16> keeps layer 2 as 64 tiles x 64 lanes x 16 words x 4 B = 256 KiB in
// LDS, and a CU has 160 KiB.  Here layer 2 lives in REGISTERS, split by output rows over the waves of the workgroup:
//   wave w owns rows 32 w .. 32 w + 31 of W2: 8 (rho = w, tau) tiles x 16 operands = 128 registers per lane, read ONCE (mlp_rows_load_w2)
//   from the flat parameter vector in the operand layout load_w2_tile reads (Wf[rho][tau][lane (i, h)][q] = W2[32 rho + i][32 tau +
//   row(q, h)]) and kept for as long as the caller keeps the array alive.
// A 32-sample column tile g is then computed by all 8 waves together (mlp_rows_forward):
//   layer 1   wave w forms h1 tile w (L1Q MFMAs, bias, activation) and writes it to LDS in D layout (4 KiB per tile, the four 16-byte
//             pieces of a lane swizzled against bank conflicts);
//   barrier;
//   layer 2   every wave reads the 8 h1 tiles as B operands (register q of a D tile is the B operand of step (tile, q), scg_mlp.h) and
//             accumulates its own 32 rows of h2 over tau = 0..7, q = 0..15 (128 MFMAs), then bias and ACT2;
//   layer 3   each wave's partial dot products of its 32 features with W3 (one fmaf chain over q = 0..15 per lane half, the halves
//             added with __shfl_xor(., 32)), written to LDS;
//   barrier (one for all G tiles);
//   the wave that owns tile g sums its 8 partials in the fixed order w = 0..7 and adds b3.
// The arithmetic per sample does not depend on G (the number of column tiles a workgroup serves) or on which tile a sample sits in.
// The h1 exchange buffer is double-buffered over g, so a tile costs one barrier; with the barrier after the inputs are published and
// the one before the sums a call is G + 2 barriers.  EVERY thread of the 512 must make the call: barriers inside.
// W1 (its Wf image), W3 and the biases stay in LDS (a few KiB); nothing of W2 is.
#pragma once
#include "scg_mlp.h"

namespace scg {

constexpr int MLP_ROWS_H = 256, MLP_ROWS_WAVES = 8;

// LDS image (float words) for G column tiles per workgroup.
template <int NIN, int NOUT, int G>
struct MlpRowsLds {
    static constexpr int H = MLP_ROWS_H, NT = H / 32;
    static constexpr int L1Q = 4 * ((NIN + 7) / 8);
    static constexpr int W1F = 0;                               // [NT][L1Q][64]
    static constexpr int W3 = W1F + NT * L1Q * 64;              // [NOUT][H]
    static constexpr int B1 = W3 + NOUT * H;
    static constexpr int B2 = B1 + H;
    static constexpr int B3 = B2 + H;
    static constexpr int X = (B3 + NOUT + 3) / 4 * 4;           // [G][L1Q][64]: the column tiles' layer-1 B operands
    static constexpr int H1 = X + G * L1Q * 64;                 // [2][NT][64 lanes][16]: the h1 exchange, double-buffered over g
    static constexpr int PART = H1 + 2 * NT * 1024;             // [G][8 waves][32 samples][NOUT]: layer-3 partials
    static constexpr int END = (PART + G * MLP_ROWS_WAVES * 32 * NOUT + 3) / 4 * 4;
    static_assert(NT == MLP_ROWS_WAVES, "one wave per 32 rows of W2");
    static_assert(NIN <= 32 && NOUT <= 8 && G >= 1 && G <= MLP_ROWS_WAVES, "unsupported MLP shape");
    static_assert(END * 4 <= 160 * 1024, "the image must fit a CU's LDS");
};

// Cooperative fill of W1's Wf image, W3 and the biases (all 512 threads; caller barriers after).
template <int NIN, int NOUT, int G>
__device__ __forceinline__ void mlp_rows_fill_lds(float* lds, const MlpWeights& w, int tid) {
    using L = MlpRowsLds<NIN, NOUT, G>;
    constexpr int NTHR = 64 * MLP_ROWS_WAVES;
    // W1F[rho][q][lane (i, h)] = W1[32 rho + i][row(q, h)], zero past NIN (mlp_fill_lds's image)
    constexpr int N1 = L::NT * L::L1Q * 64;
    for (int k = tid; k < N1; k += NTHR) {
        const int lane = k & 63, q = (k >> 6) % L::L1Q, rho = (k >> 6) / L::L1Q;
        const int in = d_row(q, lane >> 5);
        lds[L::W1F + k] = in < NIN ? w.W1[(32 * rho + (lane & 31)) * NIN + in] : 0.0f;
    }
    for (int k = tid; k < NOUT * L::H; k += NTHR) lds[L::W3 + k] = w.W3[k];
    if (tid < L::H) { lds[L::B1 + tid] = w.b1[tid]; lds[L::B2 + tid] = w.b2[tid]; }
    if (tid < NOUT) lds[L::B3 + tid] = w.b3[tid];
}

// The wave's 32 rows of W2 as MFMA A operands: w2[tau][q] = W2[32 wave + i][32 tau + row(q, h)] for lane (i, h).  Plain 4-byte loads:
// the flat vector's offsets carry no alignment promise, and this runs once per launch.
__device__ __forceinline__ void mlp_rows_load_w2(const float* __restrict__ W2, int wave, int lane, float (&w2)[MLP_ROWS_WAVES][16]) {
    const float* const p = W2 + (size_t)(32 * wave + (lane & 31)) * MLP_ROWS_H + 4 * (lane >> 5);
#pragma unroll
    for (int tau = 0; tau < MLP_ROWS_WAVES; ++tau) {
#pragma unroll
        for (int q = 0; q < 16; ++q) w2[tau][q] = p[32 * tau + d_row(q, 0)];
    }
}

// Forward pass of G column tiles.  x[q] (q < L1Q): input feature row(q, h) of this lane's sample in tile `wave`, read from waves < G;
// out[NOUT]: the outputs of that sample (identical in both lane halves), written for waves < G.
template <int NIN, int NOUT, int ACT, int ACT2, int G>
__device__ __forceinline__ void mlp_rows_forward(float* lds, const float (&w2)[MLP_ROWS_WAVES][16], const float* x, float* out, int wave, int lane) {
    using L = MlpRowsLds<NIN, NOUT, G>;
    const int h = lane >> 5;
    // The h1 exchange holds a lane's 16 values as four 16-byte pieces in 64 bytes.  At that lane stride lanes l, l + 4, l + 8, l + 12 of
    // a 16-lane group would meet in the same banks on every 16-byte access, so piece j of lane l sits at slot j ^ sw (sw = bits 2..3 of
    // l): the 16 lanes of a group then cover 64 distinct bank words.  Writer and reader are the same lane, so the values do not move.
    const int sw = (lane >> 2) & 3;
    if (wave < G) {
#pragma unroll
        for (int q = 0; q < L::L1Q; ++q) lds[L::X + (wave * L::L1Q + q) * 64 + lane] = x[q];
    }
    __syncthreads();
#pragma unroll 1
    for (int g = 0; g < G; ++g) {
        float* const hx = lds + L::H1 + (g & 1) * (L::NT * 1024);
        // ---- layer 1: h1 tile `wave` of column tile g
        {
            f32x16 acc;
#pragma unroll
            for (int j = 0; j < 4; ++j) {                               // bias: rows 8 j + 4 h + (0..3)
                const f32x4 b = *reinterpret_cast<const f32x4*>(lds + L::B1 + 32 * wave + 8 * j + 4 * h);
                acc[4 * j + 0] = b.x; acc[4 * j + 1] = b.y; acc[4 * j + 2] = b.z; acc[4 * j + 3] = b.w;
            }
#pragma unroll
            for (int q = 0; q < L::L1Q; ++q)
                acc = mfma32(lds[L::W1F + (wave * L::L1Q + q) * 64 + lane], lds[L::X + (g * L::L1Q + q) * 64 + lane], acc);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                f32x4 v;
                v.x = mlp_act<ACT>(acc[4 * j + 0]); v.y = mlp_act<ACT>(acc[4 * j + 1]);
                v.z = mlp_act<ACT>(acc[4 * j + 2]); v.w = mlp_act<ACT>(acc[4 * j + 3]);
                *reinterpret_cast<f32x4*>(hx + wave * 1024 + lane * 16 + 4 * (j ^ sw)) = v;
            }
        }
        __syncthreads();
        // ---- layer 2: my 32 rows of h2 over all 8 h1 tiles
        f32x16 acc;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const f32x4 b = *reinterpret_cast<const f32x4*>(lds + L::B2 + 32 * wave + 8 * j + 4 * h);
            acc[4 * j + 0] = b.x; acc[4 * j + 1] = b.y; acc[4 * j + 2] = b.z; acc[4 * j + 3] = b.w;
        }
#pragma unroll
        for (int tau = 0; tau < L::NT; ++tau) {
            float b[16];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(hx + tau * 1024 + lane * 16 + 4 * (j ^ sw));
                b[4 * j + 0] = v.x; b[4 * j + 1] = v.y; b[4 * j + 2] = v.z; b[4 * j + 3] = v.w;
            }
#pragma unroll
            for (int q = 0; q < 16; ++q) acc = mfma32(w2[tau][q], b[q], acc);
            __builtin_amdgcn_sched_barrier(0);                          // keep the scheduler from hoisting every tile's operand loads
        }
        // ---- layer 3: partial dot products of my 32 features
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[q] = mlp_act<ACT2>(acc[q]);
#pragma unroll
        for (int o = 0; o < NOUT; ++o) {
            float s = 0.0f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const f32x4 w = *reinterpret_cast<const f32x4*>(lds + L::W3 + o * L::H + 32 * wave + 8 * j + 4 * h);
                s = __builtin_fmaf(w.x, acc[4 * j + 0], s); s = __builtin_fmaf(w.y, acc[4 * j + 1], s);
                s = __builtin_fmaf(w.z, acc[4 * j + 2], s); s = __builtin_fmaf(w.w, acc[4 * j + 3], s);
            }
            s += __shfl_xor(s, 32, 64);
            if (h == 0) lds[L::PART + ((g * MLP_ROWS_WAVES + wave) * 32 + lane) * NOUT + o] = s;
        }
    }
    __syncthreads();
    if (wave < G) {
#pragma unroll
        for (int o = 0; o < NOUT; ++o) {
            float s = lds[L::PART + ((wave * MLP_ROWS_WAVES + 0) * 32 + (lane & 31)) * NOUT + o];
#pragma unroll
            for (int w = 1; w < MLP_ROWS_WAVES; ++w) s += lds[L::PART + ((wave * MLP_ROWS_WAVES + w) * 32 + (lane & 31)) * NOUT + o];
            out[o] = s + lds[L::B3 + o];
        }
    }
}

}  // namespace scg

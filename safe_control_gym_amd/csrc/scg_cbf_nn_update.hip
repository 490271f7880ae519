// scg_cbf_nn_update.hip — the Adam steps of the cbf_nn filter's residual network, MLP(4 -> 256 -> 256 -> 2) with relu
// (safety_filters/cbf/cbf_nn.py:227-264: compute_loss / update), every minibatch of a training episode enqueued by one call:
//     hipcc --offload-arch=gfx950 -> libscg_resupd_256.so       (C ABI, contracts and summation orders: include/scg_cbf_nn_update.h)
//
// Parameters and both Adam moments are 3 x 67 586 words = 811 KB: they do not fit a CU's LDS (scg_safety_update's plan), so the step
// is split over the chip and crosses workgroups at a KERNEL BOUNDARY, per minibatch:
//   phase_a  one workgroup (256 threads, 4 waves) per tile of TR = 4 batch rows: gather, forward, error, backward to d1.  W2 is read
//            twice per workgroup (256 KB each): the forward pass wants thread j to walk row j (stride 1 KB between lanes), so 32-column
//            chunks go through a padded LDS tile, the next chunk's loads in flight in registers under the current chunk's FMAs; the
//            backward pass wants thread k to walk column k, which is coalesced as it lies.  A batch of 64 is 16 workgroups.
//   phase_b  64 workgroups own four rows of W2 each (thread k: 4 sums over the batch rows, h1[r][k] loaded once for the four), 9 more
//            own W1 | b1 and b2 | W3 | b3 one element per thread.  Gradient sum, adam_element, plain stores.  No LDS, no barrier.
// Vector ALU throughout: a step is 13 MFLOP against ~20 us of launch and memory latency, and v_mfma_f32_32x32x2_f32 issues exact
// float32 at the vector rate, so the matrix cores would change the operand plumbing (LDS images of W2 in two orientations, rebuilt
// after every step) and not the time.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "../../include/scg_cbf_nn_update.h"
#include "scg_adam.h"

using namespace scg;

constexpr int NX = SCG_CBF_NN_UPDATE_NX, H = SCG_CBF_NN_UPDATE_HIDDEN, NOUT = SCG_CBF_NN_UPDATE_NOUT;
constexpr int NPARAMS = SCG_CBF_NN_UPDATE_PARAMS, MAX_BATCH = SCG_CBF_NN_UPDATE_MAX_BATCH;
constexpr int O_W1 = 0, O_B1 = O_W1 + H * NX, O_W2 = O_B1 + H, O_B2 = O_W2 + H * H, O_W3 = O_B2 + H, O_B3 = O_W3 + NOUT * H;
static_assert(O_B3 + NOUT == NPARAMS && NX == 4 && H == 256 && NOUT == 2, "the kernels are written for 4 -> 256 -> 256 -> 2");
constexpr int THREADS = 256;                  // = H: thread t owns hidden unit t
constexpr int TR = 4;                         // rows per phase-A tile = waves per workgroup (the output layer: one row per wave)
constexpr int KC = 32, KPAD = KC + 1;         // W2 columns per LDS chunk; the pad makes lane j's walk of row j conflict-free
// d_work: per batch row  x [4] | h1 [256] | h2 [256] | d1 [256] | d2 [256] | g (e' act, e') [2] | pad [2], then the tiles' partial losses
constexpr int R_X = 0, R_H1 = 4, R_H2 = R_H1 + H, R_D1 = R_H2 + H, R_D2 = R_D1 + H, R_G = R_D2 + H, ROW = R_G + 4;
static_assert(ROW % 4 == 0 && R_D2 % 4 == 0, "float4 reads of a work row");
constexpr int W2_ROWS_PER_GROUP = 4;
constexpr int B_W2_GROUPS = H / W2_ROWS_PER_GROUP;                       // 64
constexpr int N_SMALL = NPARAMS - H * H;                                 // W1 | b1 and b2 | W3 | b3: 2050 elements
constexpr int B_SMALL_GROUPS = (N_SMALL + THREADS - 1) / THREADS;        // 9

static thread_local std::string g_err;
static int fail(int code, const std::string& m) { g_err = m; return code; }
extern "C" const char* scg_cbf_nn_update_last_error(void) { return g_err.c_str(); }
#ifndef SCG_SRC_HASH
#define SCG_SRC_HASH 0ULL
#endif
#define SCG_STR2(x) #x
#define SCG_STR(x) SCG_STR2(x)
extern "C" const char* scg_cbf_nn_update_source_hash_tag(void) { return "SCG_SRC_HASH:" SCG_STR(SCG_SRC_HASH); }

__device__ __forceinline__ float sum4(const float (&s)[4]) { return (s[0] + s[1]) + (s[2] + s[3]); }
__device__ __forceinline__ int tiles_of(int batch) { return (batch + TR - 1) / TR; }

struct PhaseA {
    const float* params;
    const float* state;
    const float* act;
    const double* bd;
    const double* bda;
    const int32_t* rows;        // this minibatch's [batch]
    int32_t batch, train;
    float* step;
    float* work;
};

__global__ __launch_bounds__(THREADS) void phase_a(PhaseA a) {
    __shared__ float wt[H * KPAD];                                       // W2[:, k0 : k0 + KC], row j at j * KPAD
    __shared__ __attribute__((aligned(16))) float h1s[TR][H], h2s[TR][H], d2s[TR][H];
    __shared__ __attribute__((aligned(16))) float xs[TR][NX];
    __shared__ float acts[TR], tgt[TR][2], gs[TR][2], sq[TR];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int row0 = blockIdx.x * TR;
    const float* P = a.params;
    float* tile_loss = a.work + (size_t)a.batch * ROW;

    if (blockIdx.x == 0 && t == 0 && a.train) a.step[0] = a.step[0] + 1.0f;        // (phase B of this minibatch reads it back: Adam's t)
    // the first W2 chunk is on its way while the rows are gathered
    float4 pre[H * KC / 4 / THREADS];                                    // 8 float4 per thread
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int f = t + THREADS * i;
        pre[i] = *reinterpret_cast<const float4*>(P + O_W2 + (f >> 3) * H + 4 * (f & 7));
    }
    if (t < TR) {
        const int r = min(row0 + t, a.batch - 1);                        // a masked tail row reads the minibatch's last row
        const int ring = a.rows[r];
        *reinterpret_cast<float4*>(xs[t]) = *reinterpret_cast<const float4*>(a.state + (size_t)ring * NX);
        acts[t] = a.act[ring];
        tgt[t][0] = (float)a.bd[ring];
        tgt[t][1] = (float)a.bda[ring];
    }
    __syncthreads();

    // layer 1: thread t = unit t
    {
        const float4 w = *reinterpret_cast<const float4*>(P + O_W1 + t * NX);
        const float b = P[O_B1 + t];
#pragma unroll
        for (int r = 0; r < TR; ++r) {
            const float s = __builtin_fmaf(xs[r][3], w.w, __builtin_fmaf(xs[r][2], w.z, __builtin_fmaf(xs[r][1], w.y, xs[r][0] * w.x))) + b;
            h1s[r][t] = fmaxf(s, 0.0f);
        }
    }
    // layer 2: thread t = unit t, W2 through the LDS chunk
    float acc[TR][4];
#pragma unroll
    for (int r = 0; r < TR; ++r)
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[r][q] = 0.0f;
    for (int c = 0; c < H / KC; ++c) {
        __syncthreads();                                                 // h1s written (c = 0); the previous chunk's reads are done
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int f = t + THREADS * i;
            float* dst = wt + (f >> 3) * KPAD + 4 * (f & 7);
            dst[0] = pre[i].x; dst[1] = pre[i].y; dst[2] = pre[i].z; dst[3] = pre[i].w;
        }
        __syncthreads();
        if (c + 1 < H / KC) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int f = t + THREADS * i;
                pre[i] = *reinterpret_cast<const float4*>(P + O_W2 + (f >> 3) * H + KC * (c + 1) + 4 * (f & 7));
            }
        }
        const float* wrow = wt + t * KPAD;
#pragma unroll
        for (int kk = 0; kk < KC; kk += 4) {
            const float w0 = wrow[kk], w1 = wrow[kk + 1], w2 = wrow[kk + 2], w3 = wrow[kk + 3];
#pragma unroll
            for (int r = 0; r < TR; ++r) {
                const float4 h = *reinterpret_cast<const float4*>(&h1s[r][KC * c + kk]);
                acc[r][0] = __builtin_fmaf(w0, h.x, acc[r][0]);
                acc[r][1] = __builtin_fmaf(w1, h.y, acc[r][1]);
                acc[r][2] = __builtin_fmaf(w2, h.z, acc[r][2]);
                acc[r][3] = __builtin_fmaf(w3, h.w, acc[r][3]);
            }
        }
    }
    {
        const float b = P[O_B2 + t];
#pragma unroll
        for (int r = 0; r < TR; ++r) h2s[r][t] = fmaxf(sum4(acc[r]) + b, 0.0f);
    }
    __syncthreads();

    // output layer, error and loss derivative: wave w = row w; lane l takes inputs 4 l .. 4 l + 3, then a butterfly over the lanes
    {
        const int r = wave;
        const float4 h = *reinterpret_cast<const float4*>(&h2s[r][4 * lane]);
        float o[NOUT];
#pragma unroll
        for (int y = 0; y < NOUT; ++y) {
            const float4 w = *reinterpret_cast<const float4*>(P + O_W3 + y * H + 4 * lane);
            float s = __builtin_fmaf(w.w, h.w, __builtin_fmaf(w.z, h.z, __builtin_fmaf(w.y, h.y, w.x * h.x)));
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
            o[y] = s + P[O_B3 + y];
        }
        if (lane == 0) {
            const bool live = row0 + r < a.batch;
            const float err = ((tgt[r][0] + o[0] * acts[r]) + o[1]) - tgt[r][1];
            const float e = live ? 2.0f * err / (float)a.batch : 0.0f;
            gs[r][0] = e * acts[r];
            gs[r][1] = e;
            sq[r] = live ? err * err : 0.0f;
        }
    }
    __syncthreads();
    if (t == 0) {
        float s = 0.0f;
#pragma unroll
        for (int r = 0; r < TR; ++r) s += sq[r];
        tile_loss[blockIdx.x] = s;
    }
    // d2 = (W3^T g) * [h2 > 0]: thread t = unit t
    {
        const float wa = P[O_W3 + t], wb = P[O_W3 + H + t];
#pragma unroll
        for (int r = 0; r < TR; ++r) d2s[r][t] = h2s[r][t] > 0.0f ? __builtin_fmaf(wa, gs[r][0], wb * gs[r][1]) : 0.0f;
    }
    __syncthreads();
    // d1 = (d2 W2) * [h1 > 0]: thread t = column t of W2, coalesced as it lies
    float d1[TR];
    {
#pragma unroll
        for (int r = 0; r < TR; ++r)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[r][q] = 0.0f;
        const float* col = P + O_W2 + t;
#pragma unroll 4
        for (int j = 0; j < H; j += 4) {
            const float w0 = col[j * H], w1 = col[(j + 1) * H], w2 = col[(j + 2) * H], w3 = col[(j + 3) * H];
#pragma unroll
            for (int r = 0; r < TR; ++r) {
                const float4 d = *reinterpret_cast<const float4*>(&d2s[r][j]);
                acc[r][0] = __builtin_fmaf(d.x, w0, acc[r][0]);
                acc[r][1] = __builtin_fmaf(d.y, w1, acc[r][1]);
                acc[r][2] = __builtin_fmaf(d.z, w2, acc[r][2]);
                acc[r][3] = __builtin_fmaf(d.w, w3, acc[r][3]);
            }
        }
#pragma unroll
        for (int r = 0; r < TR; ++r) d1[r] = h1s[r][t] > 0.0f ? sum4(acc[r]) : 0.0f;
    }
    // what phase B sums over: the live rows only
#pragma unroll
    for (int r = 0; r < TR; ++r) {
        if (row0 + r < a.batch) {
            float* w = a.work + (size_t)(row0 + r) * ROW;
            w[R_H1 + t] = h1s[r][t];
            w[R_H2 + t] = h2s[r][t];
            w[R_D1 + t] = d1[r];
            w[R_D2 + t] = d2s[r][t];
            if (t < NX) w[R_X + t] = xs[r][t];
            if (t < 2) w[R_G + t] = gs[r][t];
        }
    }
}

struct PhaseB {
    float* params;
    float* m;
    float* v;
    const float* step;
    const float* work;
    int32_t batch, train;
    float lr;
    float* loss;                // this minibatch's element of d_loss
    float* grad;                // nullable
};

// sum over the batch rows of u[r] * v[r] (v = nullptr: of u[r]); su, sv: the strides between rows
__device__ __forceinline__ float batch_sum(const float* u, const float* v, int batch) {
    float s[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    int r = 0;
    for (; r + 3 < batch; r += 4) {
#pragma unroll
        for (int q = 0; q < 4; ++q) s[q] = __builtin_fmaf(u[(size_t)(r + q) * ROW], v ? v[(size_t)(r + q) * ROW] : 1.0f, s[q]);
    }
    for (; r < batch; ++r) s[0] = __builtin_fmaf(u[(size_t)r * ROW], v ? v[(size_t)r * ROW] : 1.0f, s[0]);
    return sum4(s);
}

__device__ __forceinline__ void apply(const PhaseB& b, int idx, float g, float t_adam) {
    if (b.grad) b.grad[idx] = g;
    if (b.train) {
        float p = b.params[idx], m = b.m[idx], v = b.v[idx];
        adam_element(p, g, m, v, b.lr, t_adam);
        b.params[idx] = p;
        b.m[idx] = m;
        b.v[idx] = v;
    }
}

__global__ __launch_bounds__(THREADS) void phase_b(PhaseB b) {
    const int t = threadIdx.x, g = blockIdx.x;
    if (g == 0 && t == 0) {                                              // the loss: tiles in order
        const float* tile_loss = b.work + (size_t)b.batch * ROW;
        float s = 0.0f;
        for (int i = 0; i < tiles_of(b.batch); ++i) s += tile_loss[i];
        b.loss[0] = s / (float)b.batch;
    }
    if (!b.train && !b.grad) return;                                     // (uniform; the kernel has no barrier)
    const float t_adam = b.step[0];
    if (g < B_W2_GROUPS) {
        // rows j0 .. j0 + 3 of W2, thread t = column t:  dW2[j][t] = sum_r d2[r][j] h1[r][t]
        const int j0 = g * W2_ROWS_PER_GROUP;
        float s[W2_ROWS_PER_GROUP][4];
#pragma unroll
        for (int y = 0; y < W2_ROWS_PER_GROUP; ++y)
#pragma unroll
            for (int q = 0; q < 4; ++q) s[y][q] = 0.0f;
        const float* h1 = b.work + R_H1 + t;
        const float* d2 = b.work + R_D2 + j0;
        int r = 0;
        for (; r + 3 < b.batch; r += 4) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float h = h1[(size_t)(r + q) * ROW];
                const float4 d = *reinterpret_cast<const float4*>(d2 + (size_t)(r + q) * ROW);
                s[0][q] = __builtin_fmaf(d.x, h, s[0][q]);
                s[1][q] = __builtin_fmaf(d.y, h, s[1][q]);
                s[2][q] = __builtin_fmaf(d.z, h, s[2][q]);
                s[3][q] = __builtin_fmaf(d.w, h, s[3][q]);
            }
        }
        for (; r < b.batch; ++r) {
            const float h = h1[(size_t)r * ROW];
            const float4 d = *reinterpret_cast<const float4*>(d2 + (size_t)r * ROW);
            s[0][0] = __builtin_fmaf(d.x, h, s[0][0]);
            s[1][0] = __builtin_fmaf(d.y, h, s[1][0]);
            s[2][0] = __builtin_fmaf(d.z, h, s[2][0]);
            s[3][0] = __builtin_fmaf(d.w, h, s[3][0]);
        }
#pragma unroll
        for (int y = 0; y < W2_ROWS_PER_GROUP; ++y) apply(b, O_W2 + (j0 + y) * H + t, sum4(s[y]), t_adam);
        return;
    }
    // W1 | b1 and b2 | W3 | b3: one element per thread
    const int e = (g - B_W2_GROUPS) * THREADS + t;
    if (e >= N_SMALL) return;
    const int idx = e < O_W2 ? e : e - O_W2 + O_B2;
    const float* w = b.work;
    float grad;
    if (idx < O_B1) grad = batch_sum(w + R_D1 + idx / NX, w + R_X + idx % NX, b.batch);             // dW1[k][i] = sum_r d1[r][k] x[r][i]
    else if (idx < O_W2) grad = batch_sum(w + R_D1 + (idx - O_B1), nullptr, b.batch);               // db1[k]
    else if (idx < O_W3) grad = batch_sum(w + R_D2 + (idx - O_B2), nullptr, b.batch);               // db2[j]
    else if (idx < O_B3) grad = batch_sum(w + R_G + (idx - O_W3) / H, w + R_H2 + (idx - O_W3) % H, b.batch);   // dW3[y][j] = sum_r g[r][y] h2[r][j]
    else grad = batch_sum(w + R_G + (idx - O_B3), nullptr, b.batch);                                // db3[y]
    apply(b, idx, grad, t_adam);
}

static bool served(int32_t batch) { return batch >= 1 && batch <= MAX_BATCH; }

extern "C" int scg_cbf_nn_update_shape(int32_t* nx, int32_t* hidden, int32_t* nout, int32_t* max_batch) {
    *nx = NX; *hidden = H; *nout = NOUT; *max_batch = MAX_BATCH;
    return 0;
}

extern "C" int scg_cbf_nn_update_work_bytes(int32_t batch, int64_t* bytes) {
    if (!served(batch) || !bytes) return fail(-1, "batch outside [1, SCG_CBF_NN_UPDATE_MAX_BATCH]");
    const int64_t tiles = (batch + TR - 1) / TR;
    *bytes = ((int64_t)batch * ROW + (tiles + 3) / 4 * 4) * (int64_t)sizeof(float);
    return 0;
}

extern "C" int scg_cbf_nn_update(const scg_cbf_nn_update_args* a, void* stream) {
    if (!a) return fail(-1, "null arguments");
    if (!a->d_params || !a->d_m || !a->d_v || !a->d_step || !a->d_state || !a->d_act || !a->d_barrier_dot || !a->d_barrier_dot_approx ||
        !a->d_rows || !a->d_loss || !a->d_work)
        return fail(-1, "a null pointer (only d_grad may be null)");
    if (a->n_batches < 1 || !served(a->batch)) return fail(-1, "n_batches < 1 or batch outside [1, SCG_CBF_NN_UPDATE_MAX_BATCH]");
    if (((uintptr_t)a->d_state | (uintptr_t)a->d_work | (uintptr_t)a->d_params) & 15) return fail(-1, "d_params, d_state and d_work must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int tiles = (a->batch + TR - 1) / TR;
    for (int i = 0; i < a->n_batches; ++i) {
        PhaseA pa{a->d_params, a->d_state, a->d_act, a->d_barrier_dot, a->d_barrier_dot_approx, a->d_rows + (size_t)i * a->batch, a->batch, a->train,
                  a->d_step, a->d_work};
        hipLaunchKernelGGL(phase_a, dim3(tiles), dim3(THREADS), 0, st, pa);
        PhaseB pb{a->d_params, a->d_m, a->d_v, a->d_step, a->d_work, a->batch, a->train, a->lr, a->d_loss + i,
                  i == a->n_batches - 1 ? a->d_grad : nullptr};
        hipLaunchKernelGGL(phase_b, dim3(B_W2_GROUPS + B_SMALL_GROUPS), dim3(THREADS), 0, st, pb);
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(-2, std::string("launch: ") + hipGetErrorString(e));
    return 0;
}

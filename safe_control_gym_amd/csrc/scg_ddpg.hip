// scg_ddpg.hip — ONE gradient step of the reference's DDPGAgent.update (controllers/ddpg/ddpg_utils.py:16-121) as a fixed
// sequence of MI355X kernels, plus the DDPG collector's noisy action and ring push, compiled per network shape:
//     hipcc -DSCG_D_NOBS=<obs_dim> -DSCG_D_H=<hidden> -DSCG_D_NU=<act_dim> -DSCG_D_ACT=<0 tanh|1 relu|2 leaky>
//     -> libscg_ddpg_<nobs>_<h>_<nu>_<act>.so       (C ABI: include/scg_ddpg.h)
//
// A DDPG step is a strict subset of a SAC step (deterministic actor, one critic, no log-prob, no temperature), so it runs on the
// same wide-tile scheme (scg_wide.h; measured for this launch shape in scg_sac.hip's notes): 32-sample column tiles, one tile per
// workgroup, the hidden features split over the workgroup's waves, the activation tiles of a forward pass that feeds a gradient
// kernel stored write-through for it, one partial gradient vector per workgroup summed in a fixed order by the reduction launch
// (which also runs Adam and the Polyak update of each parameter it owns).  q_kernel, the pairing of the reduction's group sums and
// the host helpers are SAC's own, from scg_offpolicy_step.h; this file keeps the deterministic actor's kernels, the reduction's group
// sums and bookkeeping, and the collector.
//   actor_fwd_kernel  rows ~ U[0, ring size); a = actor(obs) + its h1 / h2 tiles and tanh outputs          compute_policy_loss
//   q_kernel<1>       q(obs, a), dq/da
//   actor_grad_kernel d(-mean q)/d(actor) from the stored pass
//   reduce_kernel     actor: sum, Adam, Polyak
//   actor_fwd_kernel  a' = actor(next_obs) with the updated actor [update_n: + the next step's first job]    compute_q_loss
//   q_kernel<0>       target critic at (next_obs, a') | online critic at (obs, act) (blockIdx.y), tiles stored
//   q_kernel<2>       d mean (q - y)^2 / d(q) from the stored pass
//   reduce_kernel     critic: sum, Adam, Polyak, step counters, loss statistics
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/scg_ddpg.h"
#include "scg_adam.h"
#include "scg_mlp.h"
#include "scg_once.h"
#include "scg_rng.h"

#ifndef SCG_D_NOBS
#error "compile with -DSCG_D_NOBS= -DSCG_D_H= -DSCG_D_NU= -DSCG_D_ACT="
#endif

constexpr int NOBS = SCG_D_NOBS, HID = SCG_D_H, NU = SCG_D_NU, ACT = SCG_D_ACT;
constexpr int NQ = NOBS + NU;                 // critic input: (obs, act)
constexpr int NA = NU;                        // actor head: the action (before tanh)
constexpr int NT = HID / 32;
constexpr int WAVES = 4;
static_assert(NU >= 1 && NU <= 4 && NQ < 32 && HID % 32 == 0 && HID <= 128, "unsupported DDPG shape");
#define SCG_S_STAMP(which, k) do {} while (0)

#include "scg_wide.h"

using namespace scg;

static thread_local std::string g_err;
static int fail(int code, const std::string& m) { g_err = m; return code; }
extern "C" const char* scg_ddpg_last_error(void) { return g_err.c_str(); }
extern "C" void scg_ddpg_shape(int32_t* nobs, int32_t* hidden, int32_t* nu, int32_t* act) { *nobs = NOBS; *hidden = HID; *nu = NU; *act = ACT; }
#ifndef SCG_SRC_HASH
#define SCG_SRC_HASH 0ULL
#endif
#define SCG_STR2(x) #x
#define SCG_STR(x) SCG_STR2(x)
extern "C" const char* scg_ddpg_source_hash_tag(void) { return "SCG_SRC_HASH:" SCG_STR(SCG_SRC_HASH); }
#define HIP_TRY(e) do { hipError_t _e = (e); if (_e != hipSuccess) return fail(-2, std::string(#e) + ": " + hipGetErrorString(_e)); } while (0)

#include "scg_offpolicy_step.h"

// ================================================================== gradient step
namespace scg {
namespace wide {

// One actor forward job: rows `idx` (or, with idx_out, drawn here and kept for the later launches) of `src`; the action per batch
// row; optionally (th / h1s / h2s) what actor_grad_kernel needs of this pass.
struct AfJob {
    const float* src;
    const int32_t* idx; int32_t* idx_out; const int32_t* ring_size; const int32_t* idx_in;
    uint32_t cnt_add;
    float* a_out;
    float* th; float* h1s; float* h2s;          // nullable: tanh(out) [j][B], the waves' tiles
};
__global__ __launch_bounds__(64 * NT, 2) void actor_fwd_kernel(const float* __restrict__ params, const scg_mlp_layout lay, const Common Cm,
                                                                const AfJob J0, const AfJob J1) {
    constexpr int L1Q = 4 * ((NOBS + 7) / 8);
    extern __shared__ __align__(16) float lds[];
    const AfJob& J = blockIdx.y ? J1 : J0;
    const MlpWeights w = weights_of(params, lay);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 31, h = lane >> 5;
    const int n_tiles = Cm.batch / 32, B = Cm.batch;
    int32_t* const idx_out = J.idx_out;
    const uint32_t cnt = *Cm.counter + J.cnt_add;
    const int tile0 = blockIdx.x, r0 = tile0 * 32 + c;
    int s0 = 0;
    if (!idx_out) s0 = J.idx[r0];
    SmallRegs<NA> sr;
    small_load<NA>(sr, w, threadIdx.x);
    float a1[L1Q], a2[NT][16];
    load_a1<NOBS, L1Q>(w.W1, wave, lane, a1);
    load_a2(w.W2, wave, lane, a2);
    if (idx_out) s0 = sample_row(r0, J.ring_size, J.idx_in, cnt, Cm.k0, Cm.k1);
    float x[L1Q];
    load_x2<L1Q, NOBS, 0>(J.src + (size_t)s0 * NOBS, nullptr, h, x);
    small_store<NA>(lds, sr, threadIdx.x);
    float* const xch = lds + Small<NA>::END;
    __syncthreads();
    for (int tile = tile0; tile < n_tiles; tile += gridDim.x) {
        const int r = tile * 32 + c;
        int s = s0;
        if (tile != tile0) {
            s = idx_out ? sample_row(r, J.ring_size, J.idx_in, cnt, Cm.k0, Cm.k1) : J.idx[r];
            load_x2<L1Q, NOBS, 0>(J.src + (size_t)s * NOBS, nullptr, h, x);
        }
        if (idx_out && wave == 0 && h == 0) idx_out[r] = s;
        f32x16 h1, h2;
        float out[NA];
        forward<NOBS, NA, ACT>(lds, xch, a1, a2, x, wave, lane, h1, h2, out);
        if (J.h1s) { act_store(J.h1s, tile, wave, lane, h1); act_store(J.h2s, tile, wave, lane, h2); }
        if (wave == 0 && h == 0) {
#pragma unroll
            for (int j = 0; j < NU; ++j) {
                const float th = tanhf(out[j]);
                J.a_out[(size_t)r * NU + j] = Cm.low[j] + 0.5f * (th + 1.0f) * (Cm.high[j] - Cm.low[j]);
                if (J.th) J.th[(size_t)j * B + r] = th;
            }
        }
        // (no barrier here: forward()'s two keep a tile's exchange buffers from the next tile's writes — the argument stands above
        //  QAct in scg_offpolicy_step.h)
    }
}

// The critic's side of q_kernel (scg_offpolicy_step.h): one of them, target = rew + gamma mask q_targ[row].
struct DdpgCritic {
    static constexpr int NCRIT = 1;
    struct Nets { scg_mlp_layout lay; };
    static __device__ __forceinline__ const scg_mlp_layout& layout(const Nets& N, int) { return N.lay; }
    struct TgtArgs { const float* __restrict__ qt; };                           // [B]
    struct Tgt {
        float qt = 0.0f;
        __device__ __forceinline__ void load(const TgtArgs& A, int r, int) { qt = A.qt[r]; }
        __device__ __forceinline__ void init(const Common&) {}
        __device__ __forceinline__ float value(const Common& Cm, float v_rew, float v_mask) const { return v_rew + Cm.gamma * v_mask * qt; }
    };
};

// actor gradient of policy_loss = -mean q(obs, actor(obs)), from the pass actor_fwd_kernel left behind (tiles, tanh outputs) and
// q_kernel<1>'s q and dq/da:  d loss / d out_j = -(1/B) dq/da_j 0.5 (high_j - low_j)(1 - tanh^2)
__global__ __launch_bounds__(64 * NT, 1) void actor_grad_kernel(const float* __restrict__ params, const scg_mlp_layout lay, const Common Cm,
                                                                 const float* __restrict__ qpi, const float* __restrict__ dqda,
                                                                 const float* __restrict__ th_all, const float* __restrict__ h1s,
                                                                 const float* __restrict__ h2s, float* __restrict__ partials) {
    using S = Small<NA>;
    using G = Part<NOBS, NA>;
    constexpr int L1Q = 4 * ((NOBS + 7) / 8);
    extern __shared__ __align__(16) float lds[];
    const MlpWeights w = weights_of(params, lay);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = lane & 31, h = lane >> 5;
    const int n_tiles = Cm.batch / 32, B = Cm.batch;
    const int tile0 = blockIdx.x, r0 = tile0 * 32 + c;
    const int s0 = Cm.idx[r0];
    SmallRegs<NA> sr;
    small_load<NA>(sr, w, threadIdx.x);
    float bt[NT][16];
    f32x16 h1, h2;
    float x[L1Q], th[NU], dq[NU], q = 0.0f;
    auto load_row = [&](int tile, int r) {
        act_load(h1s, tile, wave, lane, h1); act_load(h2s, tile, wave, lane, h2);
#pragma unroll
        for (int j = 0; j < NU; ++j) { th[j] = th_all[(size_t)j * B + r]; dq[j] = dqda[(size_t)r * NU + j]; }
        q = qpi[r];
    };
    auto load_in = [&](int s) { load_x2<L1Q, NOBS, 0>(Cm.obs + (size_t)s * NOBS, nullptr, h, x); };
    load_row(tile0, r0);
    load_bt(w.W2, wave, lane, bt);
    load_in(s0);
    small_store<NA>(lds, sr, threadIdx.x);
    __syncthreads();
    float* const xch = lds + S::END;
    float* const P = partials + (size_t)blockIdx.x * PSTRIDE;
    const float inv_b = 1.0f / (float)B;
    float st_loss = 0.0f;
    bool first = true;
    for (int tile = tile0; tile < n_tiles; tile += gridDim.x) {
        const int r = tile * 32 + c;
        if (tile != tile0) { load_row(tile, r); load_in(Cm.idx[r]); }
        float dout[NA];
#pragma unroll
        for (int j = 0; j < NU; ++j) dout[j] = -inv_b * (dq[j] * 0.5f * (Cm.high[j] - Cm.low[j]) * (1.0f - th[j] * th[j]));
        if (wave == 0 && h == 0) st_loss += -q * inv_b;
        backward<NOBS, NA, ACT, true, false>(lds, xch, bt, h1, h2, dout, wave, lane, P, first, nullptr, x);
        first = false;
        __syncthreads();
    }
    if (wave == 0) {
        const float v = row_sum32(xch + Xch::WAVE + TR_WORDS + 34 * 32, st_loss, lane);
        if (lane == 0) { P[G::STAT] = v; P[G::STAT + 1] = 0.0f; }
    }
}

}  // namespace wide
}  // namespace scg

// Sum of the workgroups' partials -> flat gradient (torch parameter order: dest_of, scg_wide.h) of one network.
// Each parameter is written by exactly one thread of one launch: its sum over the partials (four groups of every fourth partial,
// then a fixed pairing), its torch.optim.Adam step and its soft update.  The step's bookkeeping rides here as well, every word
// touched by one thread of a launch in which nobody else reads it:
//   actor's launch   the statistics word's owner writes the policy loss and pre-increments steps[1] (read by the critic's launch only)
//   critic's launch  Adam's t is steps[1] as it stands; the statistics word's owner advances steps[0] and the Philox counter and
//                    writes the step's statistics
struct ReduceArgs {
    const float* partials; int n_part; scg_mlp_layout lay; float* grad;
    float* p; float* m; float* v; float lr; float* steps; int critic; float* target; float tau;
    float* stat;                // [2] workspace: the policy loss, written by the actor's launch
    uint32_t* counter; float* stats; float* stats_acc;
};
template <int NIN, int NOUT>
__global__ __launch_bounds__(256) void reduce_kernel(const ReduceArgs R) {
    __shared__ float part[4][64];
    const int kl = threadIdx.x & 63, grp = threadIdx.x >> 6;
    const int k = blockIdx.x * 64 + kl;
    constexpr int words = Part<NIN, NOUT>::END;
    const bool owner = grp == 0 && k < words;
    int d = -1;
    float o_p = 0.0f, o_m = 0.0f, o_v = 0.0f, o_t = 0.0f, o_s0 = 0.0f, o_s1 = 0.0f, o_pl = 0.0f, o_acc[2] = {0.0f, 0.0f};
    uint32_t o_cnt = 0u;
    if (owner) {
        d = dest_of<NIN, NOUT>(k, R.lay);
        if (d >= 0) {
            o_p = R.p[d]; o_m = R.m[d]; o_v = R.v[d]; o_t = R.target[d]; o_s0 = R.steps[R.critic];
        } else if (d == -2) {
            o_s0 = R.steps[0]; o_s1 = R.steps[1];
            if (R.critic) {
                o_cnt = *R.counter; o_pl = R.stat[0];
                if (R.stats_acc) { o_acc[0] = R.stats_acc[0]; o_acc[1] = R.stats_acc[1]; }
            }
        }
    }
    // (this loop is word for word scg_sac.hip's reduce_kernel's and must stay so — the order is the bitwise contract; why it is not a
    //  shared device function is said there.  The pairing behind the barrier is pair_sum, scg_offpolicy_step.h.)
    float s = 0.0f;
    if (k < words) {
        const float* const src = R.partials + (size_t)grp * PSTRIDE + k;          // partials grp, grp + 4, ...
        const int mine = (R.n_part - grp + 3) / 4;
        for (int g0 = 0; g0 < mine; g0 += 32) {
            float v[32];
#pragma unroll
            for (int j = 0; j < 32; ++j) v[j] = g0 + j < mine ? src[(size_t)(g0 + j) * 4 * PSTRIDE] : 0.0f;
#pragma unroll
            for (int j = 0; j < 32; ++j) { if (g0 + j < mine) s += v[j]; }
        }
    }
    part[grp][kl] = s;
    __syncthreads();
    if (!owner) return;
    s = pair_sum(&part[0][kl], sizeof part[0] / sizeof part[0][0]);
    if (d >= 0) {
        R.grad[d] = s;
        adam_element(o_p, s, o_m, o_v, R.lr, R.critic ? o_s0 : o_s0 + 1.0f);
        R.p[d] = o_p; R.m[d] = o_m; R.v[d] = o_v;
        R.target[d] = polyak(o_t, o_p, R.tau);
    } else if (d == -2) {
        if (!R.critic) {
            R.stat[0] = s;
            R.steps[1] = o_s1 + 1.0f;
        } else {
            R.steps[0] = o_s0 + 1.0f;
            *R.counter = o_cnt + 1u;
            R.stats[0] = o_pl; R.stats[1] = s;
            if (R.stats_acc) { R.stats_acc[0] = o_acc[0] + o_pl; R.stats_acc[1] = o_acc[1] + s; }
        }
    }
}

// ------------------------------------------------------------------ host side of the step (with the helpers of scg_offpolicy_step.h)
using QC = wide::DdpgCritic;
struct Ws {      // workspace carve-up (floats)
    size_t idx[2], a_pi, th, ah1, ah2, qpi, dqda, a_next, qt, qo, qh1, qh2, qrew, qmask, stat, partials, total;
};
static Ws carve(int B, int n_part) {
    Ws w; size_t o = 0;
    auto take = [&](size_t n) { size_t at = o; o += (n + 63) / 64 * 64; return at; };
    // (two copies of the minibatch rows: scg_ddpg_update_n draws step k + 1's while step k still reads its own)
    w.idx[0] = take(B); w.idx[1] = take(B); w.a_pi = take((size_t)B * NU); w.th = take((size_t)B * NU);
    w.ah1 = take((size_t)B * HID); w.ah2 = take((size_t)B * HID); w.qpi = take(B); w.dqda = take((size_t)B * NU);
    w.a_next = take((size_t)B * NU); w.qt = take(B); w.qo = take(B); w.qh1 = take((size_t)B * HID); w.qh2 = take((size_t)B * HID);
    w.qrew = take(B); w.qmask = take(B); w.stat = take(8);
    w.partials = take((size_t)n_part * PSTRIDE);
    w.total = o;
    return w;
}

extern "C" size_t scg_ddpg_workspace_bytes(int batch) {
    if (batch <= 0 || batch % 32) return 0;
    return carve(batch, n_part_of(batch)).total * sizeof(float);
}

// ================================================================== collector: noisy action, ring push
constexpr int NCHUNK = 256;                     // envs per workgroup of the noisy-action launch (one per thread)
struct NoiseDev {
    int kind; double theta, dt, sqrt_dt, a, std_start, std_end, std_inc; int window;
    const double* x_prev; double* x_next; const int64_t* calls; int32_t* pending;
};
__device__ __forceinline__ double sched_std(const NoiseDev& N, int64_t c) {   // LinearSchedule after c calls
    const double v = N.std_start + (double)c * N.std_inc;
    return N.std_end > N.std_start ? fmin(v, N.std_end) : fmax(v, N.std_end);
}
__device__ __forceinline__ void env_eps(int i, const float* __restrict__ eps_in, uint32_t cnt, uint32_t k0, uint32_t k1, float* e) {
    if (eps_in) {
#pragma unroll
        for (int j = 0; j < NU; ++j) e[j] = eps_in[(size_t)i * NU + j];
    } else {
        normal4(cnt, (uint32_t)i, 3u, k0, k1, e);
    }
}
static size_t lds_noisy_bytes() { return MlpLds<NOBS, HID, NA>::END * sizeof(float) + (size_t)NCHUNK * 4 * sizeof(double) * 2 + NCHUNK * sizeof(double); }

// Workgroup g: envs [256 g, 256 g + 256).  (1) the noise of its envs: OU — every thread folds a contiguous piece of [window start, chunk
// end) into an affine map x -> A x + B (A = a^len, a = 1 - theta dt), thread 0 composes the 256 maps in order starting from the carry in
// front of the window, every thread re-walks its piece from its own carry-in and keeps the x of the chunk's envs; Gaussian — std eps per
// env.  (2) the deterministic actor on the chunk's 8 tiles (LDS image, one wave per tile), plus the noise, rounded to float32 once.
__global__ __launch_bounds__(64 * WAVES, 1) void noisy_act_kernel(const float* __restrict__ params, const scg_mlp_layout lay,
                                                                   const float* __restrict__ obs, int m, float4 low, float4 high,
                                                                   uint32_t k0, uint32_t k1, const uint32_t* __restrict__ counter,
                                                                   const NoiseDev N, const float* __restrict__ eps_in, float* __restrict__ a_out) {
    using L = MlpLds<NOBS, HID, NA>;
    extern __shared__ __align__(16) float lds[];
    double* const noise = reinterpret_cast<double*>(lds + L::END);      // [NCHUNK][4]
    double* const aggB = noise + NCHUNK * 4;                            // [NCHUNK][4]: B of each thread's map, then its carry-in
    double* const aggA = aggB + NCHUNK * 4;                             // [NCHUNK]
    const int tid = threadIdx.x;
    mlp_fill_lds<NOBS, HID, NA>(lds, weights_of(params, lay), tid);
    const int E0 = blockIdx.x * NCHUNK, E1 = min(m, E0 + NCHUNK);
    const uint32_t cnt = counter ? *counter : 0u;
    if (N.kind != SCG_DDPG_NOISE_NONE && blockIdx.x == 0 && tid == 0) *N.pending = m;
    if (N.kind == SCG_DDPG_NOISE_GAUSSIAN) {
        const int i = E0 + tid;
        if (i < E1) {
            float e[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            env_eps(i, eps_in, cnt, k0, k1, e);
            const double sd = sched_std(N, *N.calls + i);
#pragma unroll
            for (int j = 0; j < NU; ++j) noise[tid * 4 + j] = (double)e[j] * sd;
        }
    } else if (N.kind == SCG_DDPG_NOISE_OU) {
        const int64_t c0 = *N.calls;
        const int W0 = E0 > N.window ? E0 - N.window : 0;
        const int len = E1 - W0, per = (len + NCHUNK - 1) / NCHUNK;
        const int i0 = min(W0 + tid * per, E1), i1 = min(i0 + per, E1);
        // (a) this thread's piece as an affine map
        double A = 1.0, Bm[4] = {0.0, 0.0, 0.0, 0.0};
        for (int i = i0; i < i1; ++i) {
            float e[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            env_eps(i, eps_in, cnt, k0, k1, e);
            const double b = sched_std(N, c0 + i) * N.sqrt_dt;
#pragma unroll
            for (int j = 0; j < NU; ++j) Bm[j] = fma(N.a, Bm[j], b * (double)e[j]);
            A *= N.a;
        }
        aggA[tid] = A;
#pragma unroll
        for (int j = 0; j < NU; ++j) aggB[tid * 4 + j] = Bm[j];
        __syncthreads();
        // (b) compose in order: aggB[t] becomes the carry-in of thread t's piece
        if (tid == 0) {
            double x[4];
            const double aw = W0 > 0 ? pow(N.a, (double)W0) : 1.0;          // the carry's own decay over the envs left out in front
#pragma unroll
            for (int j = 0; j < NU; ++j) x[j] = aw * N.x_prev[j];
            for (int t = 0; t < NCHUNK; ++t) {
                const double At = aggA[t];
#pragma unroll
                for (int j = 0; j < NU; ++j) { const double b = aggB[t * 4 + j]; aggB[t * 4 + j] = x[j]; x[j] = fma(At, x[j], b); }
            }
        }
        __syncthreads();
        // (c) re-walk with the reference's own update, keeping the chunk's values
        double x[4];
#pragma unroll
        for (int j = 0; j < NU; ++j) x[j] = aggB[tid * 4 + j];
        for (int i = i0; i < i1; ++i) {
            float e[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            env_eps(i, eps_in, cnt, k0, k1, e);
            const double b = sched_std(N, c0 + i) * N.sqrt_dt;
#pragma unroll
            for (int j = 0; j < NU; ++j) x[j] = x[j] + N.theta * (0.0 - x[j]) * N.dt + b * (double)e[j];
            if (i >= E0) {
#pragma unroll
                for (int j = 0; j < NU; ++j) noise[(i - E0) * 4 + j] = x[j];
            }
            if (i == m - 1) {
#pragma unroll
                for (int j = 0; j < NU; ++j) N.x_next[j] = x[j];
            }
        }
    }
    __syncthreads();                                                    // LDS image + the chunk's noise
    const int lane = tid & 63, wave = tid >> 6, c = lane & 31, h = lane >> 5;
    const float lo[4] = {low.x, low.y, low.z, low.w}, hi[4] = {high.x, high.y, high.z, high.w};
    for (int tile = E0 / 32 + wave; tile * 32 < E1; tile += WAVES) {
        int s = tile * 32 + c;
        const bool live = s < m;
        s = live ? s : m - 1;
        float x[L::L1Q];
        load_x2<L::L1Q, NOBS, 0>(obs + (size_t)s * NOBS, nullptr, h, x);
        f32x16 h1[NT], h2[NT];
        float out[NA];
        mlp_forward_tile<NOBS, HID, NA, ACT>(lds, x, h1, h2, out, lane);
        if (live && h == 0) {
#pragma unroll
            for (int j = 0; j < NU; ++j) {
                const float a = lo[j] + 0.5f * (tanhf(out[j]) + 1.0f) * (hi[j] - lo[j]);
                a_out[(size_t)s * NU + j] = N.kind == SCG_DDPG_NOISE_NONE ? a : (float)((double)a + noise[(s - E0) * 4 + j]);
            }
        }
    }
}

// (uniform_action_kernel, RingArgs and ring_push_kernel: scg_wide.h.)  Behind a push: the ring's write position and the commit of the
// exploration noise the step's actions drew, one thread.
struct CommitArgs { double* x_prev; const double* x_next; int64_t* calls; int32_t* pending; int kind; };
__global__ void bookkeeping_kernel(const RingArgs R, int with_ring, int n, const CommitArgs Cn) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (with_ring) ring_advance(R, n);
    if (Cn.pending) {
        const int p = *Cn.pending;
        if (p > 0) {
            if (Cn.kind == SCG_DDPG_NOISE_OU) {
                for (int j = 0; j < NU; ++j) Cn.x_prev[j] = Cn.x_next[j];
            }
            *Cn.calls += p;
        }
        *Cn.pending = 0;
    }
}

// One-time kernel attributes (dynamic LDS above 64 KB).
extern "C" int scg_ddpg_prepare(void) {
    static scg::PerDeviceOnce once;
    int dev;
    if (!once.pending(&dev)) return 0;
    if (lds_noisy_bytes() > 160 * 1024 || wide_lds_actor() > 160 * 1024 || wide_lds_q() > 160 * 1024)
        return fail(-1, "scg_ddpg: network image does not fit the LDS");
    if (set_lds(noisy_act_kernel, lds_noisy_bytes())) return -2;
    if (set_lds(wide::actor_fwd_kernel, wide_lds_actor_fwd()) || set_lds(wide::actor_grad_kernel, wide_lds_actor()) ||
        set_lds(wide::q_kernel<0, QC>, wide_lds_q_fwd()) || set_lds(wide::q_kernel<1, QC>, wide_lds_q()) || set_lds(wide::q_kernel<2, QC>, wide_lds_q())) return -2;
    once.commit(dev);
    return 0;
}

// One gradient step.  parity: which copy of the minibatch rows the step uses; have_first: the step's first launch already ran as the
// second job of the previous step's target-action launch; with_next: this step's target-action launch carries that job for the next step.
static int enqueue_step(const scg_ddpg_args* a, hipStream_t st, int parity, bool have_first, bool with_next) {
    const int B = a->batch, n_part = n_part_of(B);
    const Ws w = carve(B, n_part);
    float* W = (float*)a->d_workspace;
    int32_t* idx = (int32_t*)(W + w.idx[parity]);
    int32_t* idx_next = (int32_t*)(W + w.idx[parity ^ 1]);
    wide::Common Cm;
    fill_common(Cm, a, idx, n_part);
    float* stat = W + w.stat;
    auto policy_job = [&](int32_t* rows, uint32_t cnt_add) {
        return wide::AfJob{a->d_obs, nullptr, rows, a->d_ring_size, a->d_idx_in, cnt_add, W + w.a_pi, W + w.th, W + w.ah1, W + w.ah2};
    };
    const wide::QAct QA{W + w.qo, W + w.qh1, W + w.qh2, W + w.qrew, W + w.qmask};
    auto reduce_args = [&](const scg_mlp_layout& lay, float lr, int critic) {
        ReduceArgs R;
        R.partials = W + w.partials; R.n_part = n_part; R.lay = lay; R.grad = a->d_grad; R.p = a->d_params; R.m = a->d_m; R.v = a->d_v;
        R.lr = lr; R.steps = a->d_steps; R.critic = critic; R.target = a->d_target; R.tau = a->tau; R.stat = stat;
        R.counter = a->d_counter; R.stats = a->d_stats; R.stats_acc = a->d_stats_acc;
        return R;
    };
    // 1. minibatch rows, a = actor(obs) and its tiles
    if (!have_first) {
        const wide::AfJob J = policy_job(idx, 0u);
        wide::actor_fwd_kernel<<<dim3(n_part, 1), dim3(64 * NT), wide_lds_actor_fwd(), st>>>(a->d_params, a->actor, Cm, J, J);
    }
    // 2. q and dq/da at (obs, a)
    wide::q_kernel<1, QC><<<dim3(n_part, 1), dim3(64 * NT), wide_lds_q(), st>>>(a->d_params, nullptr, QC::Nets{a->q}, Cm, W + w.a_pi, QC::TgtArgs{}, W + w.qpi,
                                                                                W + w.dqda, QA, nullptr);
    // 3. actor gradient
    wide::actor_grad_kernel<<<dim3(n_part), dim3(64 * NT), wide_lds_actor(), st>>>(a->d_params, a->actor, Cm, W + w.qpi, W + w.dqda, W + w.th,
                                                                                   W + w.ah1, W + w.ah2, W + w.partials);
    // 4. its sum, the actor's Adam step, the soft update of the actor's target copy
    reduce_kernel<NOBS, NA><<<dim3((Part<NOBS, NA>::END + 63) / 64), dim3(256), 0, st>>>(reduce_args(a->actor, a->actor_lr, 0));
    // 5. a' = actor(next_obs) with the updated actor [+ the next step's launch 1: same actor, the counter word one ahead]
    {
        const wide::AfJob J{a->d_next_obs, idx, nullptr, nullptr, nullptr, 0u, W + w.a_next, nullptr, nullptr, nullptr};
        const wide::AfJob Jn = with_next ? policy_job(idx_next, 1u) : J;
        wide::actor_fwd_kernel<<<dim3(n_part, with_next ? 2 : 1), dim3(64 * NT), wide_lds_actor_fwd(), st>>>(a->d_params, a->actor, Cm, J, Jn);
    }
    // 6. target critic at (next_obs, a'); beside it the online critic's forward pass at (obs, act)
    wide::q_kernel<0, QC><<<dim3(n_part, 2), dim3(64 * NT), wide_lds_q_fwd(), st>>>(a->d_target, a->d_params, QC::Nets{a->q}, Cm, W + w.a_next, QC::TgtArgs{},
                                                                                    W + w.qt, nullptr, QA, nullptr);
    // 7. critic gradient
    wide::q_kernel<2, QC><<<dim3(n_part, 1), dim3(64 * NT), wide_lds_q(), st>>>(a->d_params, nullptr, QC::Nets{a->q}, Cm, nullptr, QC::TgtArgs{W + w.qt}, nullptr,
                                                                                nullptr, QA, W + w.partials);
    // 8. its sum, the critic's Adam step, the soft update of the critic's target copy, the step's bookkeeping
    reduce_kernel<NQ, 1><<<dim3((Part<NQ, 1>::END + 63) / 64), dim3(256), 0, st>>>(reduce_args(a->q, a->critic_lr, 1));
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int scg_ddpg_update(const scg_ddpg_args* a, void* stream) {
    if (int rc = check_step_args(a, "scg_ddpg_update")) return rc;
    if (int rc = scg_ddpg_prepare()) return rc;
    return enqueue_step(a, (hipStream_t)stream, 0, false, false);
}

extern "C" int scg_ddpg_update_n(const scg_ddpg_args* a, int n_steps, void* stream) {
    if (int rc = check_step_args(a, "scg_ddpg_update_n")) return rc;
    if (n_steps <= 0) return fail(-1, "scg_ddpg_update_n: n_steps must be positive");
    if (int rc = scg_ddpg_prepare()) return rc;
    for (int k = 0; k < n_steps; ++k)
        if (int rc = enqueue_step(a, (hipStream_t)stream, k & 1, k > 0, k + 1 < n_steps)) return rc;
    return 0;
}

static NoiseDev noise_dev(const scg_ddpg_noise* nz) {
    NoiseDev N{};
    N.kind = nz ? nz->kind : SCG_DDPG_NOISE_NONE;
    if (N.kind == SCG_DDPG_NOISE_NONE) return N;
    N.theta = nz->theta; N.dt = nz->dt; N.sqrt_dt = std::sqrt(nz->dt); N.a = 1.0 - nz->theta * nz->dt;
    N.std_start = nz->std_start; N.std_end = nz->std_end; N.std_inc = nz->std_inc;
    N.x_prev = nz->d_x_prev; N.x_next = nz->d_x_next; N.calls = nz->d_calls; N.pending = nz->d_pending;
    // envs in front of a chunk whose terms still weigh more than 2^-50 in its first x (all of them when the process does not contract)
    const double aa = std::fabs(N.a);
    N.window = aa == 0.0 ? 0 : (aa < 1.0 ? (int)std::min(std::ceil(50.0 * std::log(2.0) / -std::log(aa)), (double)INT_MAX) : INT_MAX);
    return N;
}

static int launch_noisy(const float* d_params, const scg_mlp_layout* actor, const float* act_low, const float* act_high, const float* d_obs,
                        int m, uint64_t seed, const uint32_t* d_counter, int uniform, const scg_ddpg_noise* noise, const float* d_eps_in,
                        float* d_act_out, hipStream_t st, const char* who) {
    if (!act_low || !act_high || !d_act_out || m <= 0 || (!uniform && (!d_params || !actor || !d_obs))) return fail(-1, std::string(who) + ": bad argument");
    if (noise && noise->kind != SCG_DDPG_NOISE_NONE &&
        (!noise->d_calls || !noise->d_pending || (noise->kind == SCG_DDPG_NOISE_OU && (!noise->d_x_prev || !noise->d_x_next))))
        return fail(-1, std::string(who) + ": noise state pointers missing");
    float4 l4, h4;
    pack_bounds(act_low, act_high, l4, h4);
    if (uniform) {
        uniform_action_kernel<<<dim3((m + 255) / 256), dim3(256), 0, st>>>(m, l4, h4, (uint32_t)seed, (uint32_t)(seed >> 32), d_counter,
                                                                          noise ? noise->d_pending : nullptr, d_act_out);
    } else {
        if (int rc = scg_ddpg_prepare()) return rc;
        noisy_act_kernel<<<dim3((m + NCHUNK - 1) / NCHUNK), dim3(64 * WAVES), lds_noisy_bytes(), st>>>(
            d_params, *actor, d_obs, m, l4, h4, (uint32_t)seed, (uint32_t)(seed >> 32), d_counter, noise_dev(noise), d_eps_in, d_act_out);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int scg_ddpg_noisy_act(const float* d_params, const scg_mlp_layout* actor, const float* act_low, const float* act_high, const float* d_obs,
                                  int m, uint64_t seed, const uint32_t* d_counter, int uniform, const scg_ddpg_noise* noise, const float* d_eps_in,
                                  float* d_act_out, void* stream) {
    return launch_noisy(d_params, actor, act_low, act_high, d_obs, m, seed, d_counter, uniform, noise, d_eps_in, d_act_out, (hipStream_t)stream,
                        "scg_ddpg_noisy_act");
}

extern "C" int scg_ddpg_act(const float* d_params, const scg_mlp_layout* actor, const float* act_low, const float* act_high, const float* d_obs,
                            int m, float* d_act_out, void* stream) {
    return launch_noisy(d_params, actor, act_low, act_high, d_obs, m, 0, nullptr, 0, nullptr, nullptr, d_act_out, (hipStream_t)stream, "scg_ddpg_act");
}

static CommitArgs commit_args(const scg_ddpg_noise* nz) {
    if (!nz || nz->kind == SCG_DDPG_NOISE_NONE || !nz->d_pending) return CommitArgs{nullptr, nullptr, nullptr, nullptr, 0};
    return CommitArgs{nz->d_x_prev, nz->d_x_next, nz->d_calls, nz->d_pending, nz->kind};
}

extern "C" int scg_ddpg_noise_commit(const scg_ddpg_noise* noise, void* stream) {
    const RingArgs R{};
    bookkeeping_kernel<<<dim3(1), dim3(64), 0, (hipStream_t)stream>>>(R, 0, 0, commit_args(noise));
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int scg_ddpg_push(const scg_ddpg_ring* ring, const scg_ddpg_noise* noise, float* d_cur_obs, const float* d_act, const float* d_reward,
                             const float* d_next_obs, const float* d_terminal_obs, const uint8_t* d_done, const uint8_t* d_flags, int n, void* stream) {
    RingArgs R;
    if (int rc = launch_ring_push(ring, d_cur_obs, d_act, d_reward, d_next_obs, d_terminal_obs, d_done, d_flags, n, (hipStream_t)stream, "scg_ddpg_push", R))
        return rc;
    bookkeeping_kernel<<<dim3(1), dim3(64), 0, (hipStream_t)stream>>>(R, 1, n, commit_args(noise));
    HIP_TRY(hipGetLastError());
    return 0;
}

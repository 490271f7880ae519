/* scg_safe_pretrain.h — Safe-Explorer's PRE-TRAINING phase (safe_ppo.py:281-297: random-action transitions, then a regression of the
 * constraint models on them) as two launches per epoch.  Both entry points live in libscg_saferoll_<spechash>_<H>_<act>_<Hc>.so
 * (include/scg_safe_explorer.h): observation width, action width, the number of state-constraint rows C and the safety layer's hidden
 * width Hc are that library's compile-time constants (scg_safe_explorer_shape).  float32 envs only.
 *
 * (a) scg_collect_constraints: K control steps with uniform random actions, one thread per env, the state in registers, auto-reset
 *     inside the launch.  Per step t and env i the transition (obs, act, c, c_next) goes to row (pos + t*N + i) % capacity of the
 *     caller's ring arrays:
 *       obs     the observation the env shows before the step (recomputed from the state at launch entry; the fresh one after a reset)
 *       act     low_j + (high_j - low_j) * u01(word j) of Philox channel 4, item 0, block 0, counter (env id, episode, step in episode):
 *               scg_rollout_random's draw
 *       c       the state-constraint rows of the current state (t = 0: d_c_carry as passed in)
 *       c_next  the state rows of this step's constraint values: the terminal, pre-reset values where the episode ended
 *     The c carried to step t + 1 is c_next, or the rows of the fresh state where the env was reset.
 *
 * (b) scg_safety_update: n_batches minibatches of SafetyLayer.update (safe_explorer_utils.py:86-118) in one launch:
 *       g = W2 relu(W1 obs + b1) + b2,  pred = c_i + g.act,  loss_i = mean((c_next_i - pred)^2),  one Adam step per constraint model
 *       (betas 0.9 / 0.999, eps 1e-8).
 *     Workgroup i owns constraint model i: its parameters, both Adam moments and the gradient sit in LDS for the whole launch; nothing
 *     crosses workgroups, there are no atomics, every sum has a fixed order.  Exact float32 on the vector ALU; bit-reproducible; n
 *     minibatches in one launch equal n launches of one bit for bit; constraint i's results do not depend on constraint j's parameters.
 */
#ifndef SCG_SAFE_PRETRAIN_H
#define SCG_SAFE_PRETRAIN_H

#include <stdint.h>

#include "scg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct scg_collect_io {
    float* d_obs;           /* [capacity][obs_dim]  ring arrays, row-major float32, 16-byte aligned */
    float* d_act;           /* [capacity][nu] */
    float* d_c;             /* [capacity][C] */
    float* d_c_next;        /* [capacity][C] */
    int64_t pos;            /* ring row of (t = 0, env 0); 0 <= pos < capacity */
    int64_t capacity;       /* k_steps * N <= capacity, capacity * 4 * max(obs_dim, C) < 2^32 */
    float low[4], high[4];  /* action bounds (spec.action_space); entries >= nu are ignored */
    float* d_c_carry;       /* [N][C] in/out: the constraint values of the current state */
    float* d_last_obs;      /* [N][obs_dim] out: the observation after the last step */
    float* d_ep_stats;      /* nullable [N][4]: the env's running episode totals, advanced as under scg_step */
} scg_collect_io;

/* SCG_ERR_INVALID (nothing launched, nothing written) when k_steps * N > capacity: two threads would write one row. */
int scg_collect_constraints(scg_env* env, int k_steps, const scg_collect_io* io, void* stream);

typedef struct scg_safety_update_args {
    float* d_params;        /* [C][P], per constraint: W1 [Hc][obs] | b1 [Hc] | W2 [A][Hc] | b2 [A]  (nn.Linear layout), P = Hc*(obs+1+A)+A */
    float* d_m; float* d_v; /* [C][P] Adam moments */
    float* d_steps;         /* [C] Adam step counts, advanced by n_batches when train != 0 */
    const float *d_obs, *d_act, *d_c, *d_c_next;     /* the ring arrays of (a) */
    const int32_t* d_rows;  /* [n_batches][batch] ring rows of each minibatch (the caller's permutation); every entry a valid ring row */
    int32_t n_batches, batch;                         /* batch >= 1, ANY value: tail rows are masked */
    float lr;
    int32_t train;          /* 0: losses only, nothing else is written */
    float* d_loss;          /* [n_batches][C] mean squared error of each minibatch, under the parameters BEFORE its update */
    float* d_grad;          /* nullable [C][P]: the gradient of the LAST minibatch (tests) */
} scg_safety_update_args;

/* Launches on the current device. */
int scg_safety_update(const scg_safety_update_args* args, void* stream);

/* LDS bytes per workgroup of scg_safety_update for this library's shape; more than 163840 (160 KiB): the shape is not served and
 * scg_safety_update returns SCG_ERR_INVALID. */
int scg_safe_pretrain_lds(int32_t* bytes);

#ifdef __cplusplus
}
#endif

#endif /* SCG_SAFE_PRETRAIN_H */

/* scg_cbf_nn_update.h — the Adam steps of the cbf_nn safety filter's residual network (safety_filters/cbf/cbf_nn.py:227-264:
 * CBF_NN.compute_loss / update) with every minibatch of a training episode enqueued by ONE library call.  The library
 * (libscg_resupd_256.so, csrc/scg_cbf_nn_update.hip) serves one network shape, MLP(4 -> 256 -> 256 -> 2) with relu on both hidden
 * layers, and needs no env handle and no task config: the four ring arrays are the caller's (DeviceCBFBuffer's).
 *
 *     (a, b) = mlp(state),   loss = mean((barrier_dot + a act + b - barrier_dot_approx)^2)  over the `batch` rows given,
 *     then one torch.optim.Adam step (betas 0.9 / 0.999, eps 1e-8: csrc/scg_adam.h's adam_element).
 *
 * Per minibatch the call enqueues two kernels on the stream; the kernel boundary is the only synchronisation between workgroups
 * (no flags, no grid sync, no atomics):
 *   phase A  one workgroup per tile of 4 rows: gather by index, forward pass, per-row error, d2 = (W3^T e') * [h2 > 0],
 *            d1 = (d2 W2) * [h1 > 0]; x, h1, h2, d1, d2, e' of each row and the tile's partial loss go to d_work.
 *   phase B  every workgroup owns a contiguous slice of the parameter vector: its gradient is the sum over the batch rows
 *            (dW2[j, :] = sum_r d2[r, j] h1[r, :], ...), then adam_element in place; one thread finishes d_loss[i].
 * Exact float32 on the vector ALU (the step is bound by launch and memory latency, not by its 13 MFLOP).
 *
 * Summation orders (all fixed): a dot product over 256 inputs runs in four interleaved partial sums (input k goes to sum k mod 4,
 * ascending k), combined (s0 + s1) + (s2 + s3); the output layer's two dot products: four consecutive inputs per lane, then a
 * butterfly over the 64 lanes; a sum over the batch rows: four interleaved partial sums (row r to sum r mod 4, the last batch mod 4
 * rows to sum 0), combined the same way; the loss: rows of a tile in order, tiles in order, then / batch.
 *
 * Contracts:
 *   - the result is bit-reproducible from run to run;
 *   - n minibatches in one call equal n calls of one, bit for bit;
 *   - a row's contribution does not depend on its position in the batch beyond the fixed summation order (the position permutes the
 *     order of the sum); a row index that occurs twice counts twice;
 *   - a parameter whose gradient is exactly zero (a dead relu unit) and whose moments are zero keeps its bits;
 *   - train = 0 writes d_loss (and d_grad if given) and nothing else (d_work is scratch);
 *   - masked tail rows of the last tile read a valid row (the minibatch's last) and contribute nothing.
 * Not served: other hidden widths, float32 barrier columns, batches above SCG_CBF_NN_UPDATE_MAX_BATCH.  The library does not know
 * the ring's capacity: every entry of d_rows must be a valid ring row (the Python facade checks before the call).
 */
#ifndef SCG_CBF_NN_UPDATE_H
#define SCG_CBF_NN_UPDATE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCG_CBF_NN_UPDATE_NX 4
#define SCG_CBF_NN_UPDATE_HIDDEN 256
#define SCG_CBF_NN_UPDATE_NOUT 2
#define SCG_CBF_NN_UPDATE_PARAMS 67586      /* 256*4 + 256 + 256*256 + 256 + 2*256 + 2 */
#define SCG_CBF_NN_UPDATE_MAX_BATCH 256

typedef struct scg_cbf_nn_update_args {
    float* d_params;            /* flat float32 [67586]: W1 [256][4] | b1 | W2 [256][256] | b2 | W3 [2][256] | b3   (scg_cbf_residual's packing) */
    float* d_m; float* d_v;     /* Adam moments, same packing */
    float* d_step;              /* [1] Adam step count, advanced by n_batches when train != 0 */
    const float*  d_state;      /* ring [capacity][4]  float32 */
    const float*  d_act;        /* ring [capacity]     float32 */
    const double* d_barrier_dot;        /* ring [capacity] float64 (DeviceCBFBuffer's dtype); rounded to float32 on read, as .to(float32) */
    const double* d_barrier_dot_approx; /* ring [capacity] float64, likewise */
    const int32_t* d_rows;      /* [n_batches][batch] ring rows of each minibatch; duplicates allowed and counted as often as they occur */
    int32_t n_batches, batch;   /* 1 <= batch <= SCG_CBF_NN_UPDATE_MAX_BATCH; ANY value in that range, tail rows masked */
    float lr;
    int32_t train;              /* 0: losses only, nothing else is written */
    float* d_loss;              /* [n_batches]  compute_loss under the parameters BEFORE that minibatch's step */
    float* d_grad;              /* nullable [67586]: the gradient of the LAST minibatch (tests) */
    float* d_work;              /* scratch of scg_cbf_nn_update_work_bytes(batch) bytes, 16-byte aligned */
} scg_cbf_nn_update_args;

/* Enqueues 2 * n_batches kernels on `stream` of the current device.  0 on success; -1 (SCG_ERR_INVALID) for an argument it does
 * not serve (a null pointer other than d_grad, n_batches < 1, batch outside [1, MAX_BATCH], a d_state or d_work that is not 16-byte
 * aligned), with nothing launched and nothing written; -2 (SCG_ERR_HIP) when a launch fails. */
int scg_cbf_nn_update(const scg_cbf_nn_update_args* args, void* stream);

/* Bytes of d_work for minibatches of `batch` rows; -1 for a batch that is not served. */
int scg_cbf_nn_update_work_bytes(int32_t batch, int64_t* bytes);

/* The network shape and the largest batch this library serves. */
int scg_cbf_nn_update_shape(int32_t* nx, int32_t* hidden, int32_t* nout, int32_t* max_batch);

const char* scg_cbf_nn_update_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* SCG_CBF_NN_UPDATE_H */

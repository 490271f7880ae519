"""Float64 NumPy restatement of the cbf_nn residual network's training step (safety_filters/cbf/cbf_nn.py:227-264: compute_loss, then
one torch.optim.Adam step, betas 0.9 / 0.999, eps 1e-8): loss, gradient and the optimiser, next to tests/cbf_nn_model.py (the forward
pass and the filter).  tests/test_cbf_nn_update_cpu.py pins this file to the reference-generated fixture (tests/golden/cbf_nn.npz:
train/*); the GPU tests of scg_cbf_nn_update (tests/test_gpu_cbf_nn_update.py) lean on it."""
import os

import numpy as np

KEYS = ('fcs.0.weight', 'fcs.0.bias', 'fcs.1.weight', 'fcs.1.bias', 'fcs.2.weight', 'fcs.2.bias')
SIZES = (1024, 256, 65536, 256, 512, 2)
SHAPES = ((256, 4), (256,), (256, 256), (256,), (2, 256), (2,))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
LR = 0.001                      # safety_filters/cbf/cbf_nn.yaml: learning_rate
B1, B2, EPS = 0.9, 0.999, 1e-8


def fixture():
    """(initial weights, the recorded batch, the weights after three updates, loss, loss_after) of tests/golden/cbf_nn.npz."""
    G = np.load(os.path.join(GOLDEN, 'cbf_nn.npz'))
    w0 = [np.asarray(G['mlp/' + k]) for k in KEYS]
    batch = {k: np.asarray(G['train/batch/' + k]) for k in ('state', 'act', 'barrier_dot', 'barrier_dot_approx')}
    after = {k: np.asarray(G['train/after/' + k]) for k in KEYS if k != 'fcs.1.weight'}
    after['fcs.1.weight/rows'] = np.asarray(G['train/after/fcs.1.weight/rows'])
    after['fcs.1.weight/sums'] = np.asarray(G['train/after/fcs.1.weight/sums'])
    return w0, batch, after, float(G['train/loss']), float(G['train/loss_after']), np.asarray(G['states'])


def loss_and_grad(weights, state, act, barrier_dot, barrier_dot_approx):
    """(loss, [dW1, db1, dW2, db2, dW3, db3]) in float64; a row that occurs twice counts twice."""
    W1, b1, W2, b2, W3, b3 = (np.asarray(w, dtype=np.float64) for w in weights)
    x = np.asarray(state, dtype=np.float64).reshape(-1, 4)
    u = np.asarray(act, dtype=np.float64).reshape(-1)
    n = x.shape[0]
    z1 = x @ W1.T + b1
    h1 = np.maximum(z1, 0.0)
    z2 = h1 @ W2.T + b2
    h2 = np.maximum(z2, 0.0)
    out = h2 @ W3.T + b3
    err = np.asarray(barrier_dot, dtype=np.float64).reshape(-1) + out[:, 0] * u + out[:, 1] - np.asarray(barrier_dot_approx, dtype=np.float64).reshape(-1)
    e = 2.0 * err / n
    g = np.stack([e * u, e], axis=1)                       # d loss / d out
    d2 = (g @ W3) * (z2 > 0)
    d1 = (d2 @ W2) * (z1 > 0)
    return float((err * err).mean()), [d1.T @ x, d1.sum(0), d2.T @ h1, d2.sum(0), g.T @ h2, g.sum(0)]


class Adam:
    """torch.optim.Adam on a list of float64 arrays (no weight decay, no amsgrad)."""

    def __init__(self, weights, lr=LR):
        self.w = [np.array(w, dtype=np.float64) for w in weights]
        self.m = [np.zeros_like(w) for w in self.w]
        self.v = [np.zeros_like(w) for w in self.w]
        self.t, self.lr = 0, lr

    def step(self, grads):
        self.t += 1
        bc1, bc2 = 1.0 - B1 ** self.t, 1.0 - B2 ** self.t
        for w, m, v, g in zip(self.w, self.m, self.v, grads):
            m *= B1
            m += (1.0 - B1) * g
            v *= B2
            v += (1.0 - B2) * g * g
            w -= (self.lr / bc1) * m / (np.sqrt(v) / np.sqrt(bc2) + EPS)


def train(weights, batches, lr=LR):
    """Adam steps on a sequence of (state, act, barrier_dot, barrier_dot_approx) batches from zero moments: (final weights, the loss
    before each step, the gradients of each step)."""
    opt = Adam(weights, lr)
    losses, grads = [], []
    for b in batches:
        lo, g = loss_and_grad(opt.w, *b)
        losses.append(lo)
        grads.append(g)
        opt.step(g)
    return opt.w, losses, grads


def pack(weights, dtype=np.float32):
    """The flat vector of scg_cbf_residual's packing."""
    return np.concatenate([np.asarray(w, dtype=dtype).reshape(-1) for w in weights])


def unpack(flat):
    out, off = [], 0
    for n, shp in zip(SIZES, SHAPES):
        out.append(np.asarray(flat[off:off + n]).reshape(shp))
        off += n
    return out


def ulp(x):
    """The float32 spacing at magnitude x."""
    return float(np.spacing(np.float32(abs(x))))

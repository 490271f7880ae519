"""NumPy float64 restatement of scg_safety_update (include/scg_safe_pretrain.h; SafetyLayer.update, safe_explorer_utils.py:86-118) and the
ring-row rule of scg_collect_constraints, plus the loader of tests/golden/safety_pretrain.npz.

Flat layout of one constraint model (nn.Linear layout, the optimisers' parameter order):  W1 [Hc][obs] | b1 [Hc] | W2 [A][Hc] | b2 [A]."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'safety_pretrain.npz')
CASES = ('cartpole_stab', 'quadrotor_2D_track')


def ring_rows(pos, k_steps, n_envs, capacity):
    """[k_steps, n_envs] ring row of step t, env i: (pos + t * N + i) % capacity."""
    t = np.arange(k_steps, dtype=np.int64)[:, None]
    i = np.arange(n_envs, dtype=np.int64)[None, :]
    return (int(pos) + t * int(n_envs) + i) % int(capacity)


def split(flat, obs, A, Hc):
    """(W1 [.., Hc, obs], b1 [.., Hc], W2 [.., A, Hc], b2 [.., A]) views of flat [.., P]."""
    lead = flat.shape[:-1]
    o = 0
    out = []
    for shp in ((Hc, obs), (Hc,), (A, Hc), (A,)):
        k = int(np.prod(shp))
        out.append(flat[..., o:o + k].reshape(lead + shp))
        o += k
    assert o == flat.shape[-1]
    return out


def loss_and_grad(flat, obs, act, c, c_next):
    """Per-constraint loss [C] and gradient [C, P] of one minibatch: g = W2 relu(W1 obs + b1) + b2, pred = c_i + g.act,
    loss_i = mean((c_next_i - pred)^2).  flat [C, P]; obs [B, obs], act [B, A], c / c_next [B, C]."""
    C = flat.shape[0]
    B, nobs = obs.shape
    A = act.shape[1]
    Hc = (flat.shape[1] - A) // (nobs + 1 + A)
    W1, b1, W2, b2 = split(flat, nobs, A, Hc)
    pre = np.einsum('chk,bk->cbh', W1, obs) + b1[:, None, :]                 # [C, B, Hc]
    h = np.maximum(pre, 0.0)
    g = np.einsum('cah,cbh->cba', W2, h) + b2[:, None, :]                    # [C, B, A]
    pred = c.T + (g * act[None]).sum(-1)                                     # [C, B]
    d = pred - c_next.T
    loss = (d * d).mean(1)
    e = 2.0 * d / B                                                          # dL/dpred
    dg = e[:, :, None] * act[None]                                           # [C, B, A]
    gW2 = np.einsum('cba,cbh->cah', dg, h)
    gb2 = dg.sum(1)
    dh = np.einsum('cba,cah->cbh', dg, W2) * (pre > 0)
    gW1 = np.einsum('cbh,bk->chk', dh, obs)
    gb1 = dh.sum(1)
    grad = np.concatenate([gW1.reshape(C, -1), gb1, gW2.reshape(C, -1), gb2], axis=1)
    return loss, grad


def adam(p, g, m, v, t, lr, b1=0.9, b2=0.999, eps=1e-8):
    """torch.optim.Adam's step t (1-based) on arrays of any shape; returns (p, m, v)."""
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    p = p - (lr / (1 - b1 ** t)) * m / (np.sqrt(v) / np.sqrt(1 - b2 ** t) + eps)
    return p, m, v


def run(flat, data, rows, lr, m=None, v=None, steps=0, train=True):
    """The minibatches rows[k] one after the other.  Returns dict(loss [n, C], final, m, v, grad (the last minibatch's), steps)."""
    p = np.array(flat, dtype=np.float64)
    m = np.zeros_like(p) if m is None else np.array(m, dtype=np.float64)
    v = np.zeros_like(p) if v is None else np.array(v, dtype=np.float64)
    d = {k: np.asarray(x, dtype=np.float64) for k, x in data.items()}
    losses, grad = [], None
    for idx in rows:
        loss, grad = loss_and_grad(p, d['obs'][idx], d['act'][idx], d['c'][idx], d['c_next'][idx])
        losses.append(loss)
        if train:
            steps += 1
            p, m, v = adam(p, grad, m, v, steps, lr)
    return {'loss': np.array(losses), 'final': p, 'm': m, 'v': v, 'grad': grad, 'steps': steps}


def load_case(name, path=GOLDEN):
    """One case of the fixture: dims, lr, init, the ring, rows, and the reference's float64 (`*64`) and float32 (`*32`) results."""
    G = np.load(path)
    g = {k[len(name) + 1:]: G[k] for k in G.files if k.startswith(name + '/')}
    obs, A, C, Hc, batch, nb, cap = (int(x) for x in g['dims'])
    out = {'obs_dim': obs, 'act_dim': A, 'C': C, 'Hc': Hc, 'batch': batch, 'n_batches': nb, 'capacity': cap, 'lr': float(g['lr']),
           'init': g['init'], 'rows': g['rows'], 'data': {k: g[k] for k in ('obs', 'act', 'c', 'c_next')}, 'loss32': g['loss32'],
           'loss64': g['loss64']}
    for k in ('final', 'm', 'v', 'grad'):
        out[k + '64'] = g[k + '64']
        # the float32 run is stored as the int32 bit-pattern difference to float32(float64 result) (make_safety_pretrain.py)
        with np.errstate(over='ignore'):
            out[k + '32'] = (g[k + '64'].astype(np.float32).view(np.int32) + g[k + '32_d']).view(np.float32)
    return out

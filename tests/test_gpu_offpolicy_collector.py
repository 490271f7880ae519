"""The SAC and DDPG collector kernels (csrc/scg_sac.hip, csrc/scg_ddpg.hip) at every network shape build() prebuilds for the two
libraries, against plain float64 references of the same operations:
  (a) deterministic actions   scg_sac_act, scg_ddpg_act, scg_ddpg_noisy_act without noise
  (b) SAC sampled actions     scg_sac_sample with the caller's eps, with the in-kernel Philox draw, and the uniform warm-up
  (c) DDPG exploration noise  scg_ddpg_noisy_act + scg_ddpg_noise_commit: Gaussian and Ornstein-Uhlenbeck, the uniform warm-up
  (d) ring push               scg_sac_push, scg_ddpg_push (+ the noise commit of its bookkeeping launch)
The reference actor is the agent's own, copied and cast to float64; the in-kernel draws are pinned to tests/philox_model.py.

Deterministic tolerance, per element (u64 the float64 pre-squash value, S = |b3| + sum |W3| |h2| the magnitude of the head's
dot-product terms, in float64):
    |a - a64| <= 0.5 (high - low) (sech^2(u64) TAU S + 2^-22) + ulp32(max(|low|, |high|)),   TAU = 1e-5
(TAU: the float32 forward pass; 2^-22: tanhf and the squash's roundings; the ulp: the final `low + ...`).  A column with low == high
returns low exactly.  Each test prints its worst error / bound ratio ([ratio] lines)."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch
from scipy.signal import lfilter

from safe_control_gym_amd import _ddpg, _sac, ddpg
from safe_control_gym_amd.sac import SACAgent, SACConfig
from tests import philox_model as pm

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# every shape build() prebuilds, plus one per library with fewer observation elements than action columns
SAC_SHAPES = [(24, 128, 4, 'relu'), (6, 32, 2, 'relu'), (12, 64, 2, 'relu'), (7, 96, 1, 'relu'), (17, 96, 2, 'tanh'), (27, 64, 4, 'leaky_relu'),
              (1, 32, 1, 'tanh'), (29, 128, 2, 'relu'), (3, 32, 3, 'relu'), (4, 32, 1, 'tanh'), (12, 64, 4, 'relu'), (2, 64, 3, 'leaky_relu')]
DDPG_SHAPES = [(24, 128, 4, 'relu'), (6, 32, 1, 'tanh'), (10, 64, 4, 'relu'), (12, 128, 2, 'relu'), (1, 32, 1, 'tanh'), (7, 96, 1, 'relu'),
               (17, 96, 3, 'tanh'), (27, 64, 4, 'leaky_relu'), (12, 32, 2, 'relu'), (1, 32, 4, 'tanh')]
SIZES = (1, 31, 33, 1000, 32768 + 135)          # one row, ragged tiles, a second grid pass of scg_sac_act / _sample (256 x 4 x 32 rows)
REGIMES = ('default', 'saturating', 'zero_rows')
TAU = 1e-5
# |eps_kernel - eps64| <= D_EPS (1 + |eps|) + D_LOG / r (r = the Box-Muller radius of the column's pair): the kernel's __sincosf and
# __logf; an absolute error dL of ln u moves r = sqrt(-2 ln u) by dL / r, which dominates near u = 1.  Measured over 2^21 rows x 4
# columns (test_in_kernel_draw_readout): 2.3e-6 and 3.0e-8; the constants leave a margin of ~2
D_EPS, D_LOG = 4e-6, 6e-8
SEED = (0x5DEECE66 << 32) | 0x1234ABCD          # the key's high word is non-zero
# (low, high) per column: one wide range, one degenerate column, two asymmetric ones (dyadic: high - low is exact in float32);
# the second set rotates them so that a one-column network meets both the wide and the degenerate column
BOUNDS = [(-40.0, 60.0), (0.5, 0.5), (-1.25, 0.75), (-0.375, 2.5)]
BOUND_SETS = (BOUNDS, BOUNDS[1:] + BOUNDS[:1])


def sid(shape):
    return '_'.join(str(v) for v in shape)


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)


class Bounds:
    def __init__(self, cols, nu):
        self.lo = np.array([c[0] for c in cols[:nu]], np.float64)
        self.hi = np.array([c[1] for c in cols[:nu]], np.float64)
        pad = [0.0] * (4 - nu)
        self.c_lo, self.c_hi = (C.c_float * 4)(*self.lo.tolist(), *pad), (C.c_float * 4)(*self.hi.tolist(), *pad)
        self.t_lo, self.t_hi = (torch.as_tensor(v, device=DEV) for v in (self.lo, self.hi))
        self.half = 0.5 * (self.t_hi - self.t_lo)
        self.ulp = torch.as_tensor(ulp32(np.maximum(np.abs(self.lo), np.abs(self.hi))), device=DEV)
        self.degenerate = [j for j in range(nu) if self.lo[j] == self.hi[j]]

    def squash(self, u):
        return self.t_lo + 0.5 * (torch.tanh(u) + 1.0) * (self.t_hi - self.t_lo)

    def bound(self, u, S, extra=0.0):
        """The deterministic tolerance at pre-squash value u64 with term magnitude S; `extra` is added inside 0.5 (high - low) sech^2."""
        sech2 = torch.cosh(u).pow(-2)
        return self.half * (sech2 * (TAU * S + extra) + 2.0 ** -22) + self.ulp


def draws(c, m, nu):
    """normal4 of rows 0..m-1 at counter c (first nu columns) and the allowed |eps_kernel - eps64| of each."""
    e = pm.normal4(SEED, c, np.arange(m))
    r = np.repeat(np.stack([np.hypot(e[:, 0], e[:, 1]), np.hypot(e[:, 2], e[:, 3])], axis=1), 2, axis=1)
    tol = D_EPS * (1.0 + np.abs(e)) + D_LOG / r
    return e[:, :nu], tol[:, :nu]


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return None if t is None else t.data_ptr()


def canary(m, nu):
    return torch.full(((m + 64) * nu,), float('nan'), device=DEV)


def check_out(out, m, nu, want, bound, B, tag, worst):
    """Canary rows untouched, degenerate columns exactly low, |out - want| <= bound; records the worst ratio."""
    assert bool(torch.isnan(out[m * nu:]).all()), f'{tag}: wrote past row {m}'
    got = out[:m * nu].view(m, nu)
    assert bool(torch.isfinite(got).all()), f'{tag}: non-finite action'
    for j in B.degenerate:
        assert bool((got[:, j] == float(np.float32(B.lo[j]))).all()), f'{tag}: degenerate column {j} is not low'
    ratio = float(((got.double() - want).abs() / bound).max())
    worst[0] = max(worst[0], ratio)
    assert ratio <= 1.0, f'{tag}: error / bound = {ratio:.3g}'
    return got


# ---------------------------------------------------------------------------------------------------------------- networks
_agents = {}


def sac_agent(shape):
    if ('sac', shape) not in _agents:
        obs, hid, nu, act = shape
        torch.manual_seed(17 + obs + 31 * nu)
        ag = SACAgent(obs, nu, -torch.ones(nu, device=DEV), torch.ones(nu, device=DEV), SACConfig(hidden_dim=hid, activation=act), DEV)
        assert ag.use_fused
        _agents['sac', shape] = (ag, _sac.lib(*shape))
    return _agents['sac', shape]


def ddpg_agent(shape):
    if ('ddpg', shape) not in _agents:
        obs, hid, nu, act = shape
        torch.manual_seed(23 + obs + 31 * nu)
        ag = ddpg.DDPGAgent(obs, nu, -np.ones(nu), np.ones(nu), ddpg.DDPGConfig(hidden_dim=hid, activation=act), DEV)
        assert ag.use_fused
        _agents['ddpg', shape] = (ag, _ddpg.lib(*shape))
    return _agents['ddpg', shape]


def head_terms(layer, h):
    """float64 (layer(h), |b| + |h| |W|^T)."""
    return layer(h), layer.bias.abs() + h.abs() @ layer.weight.abs().T


@torch.no_grad()
def sac_ref(ag, x):
    """float64 (mu, S_mu, log_std before the clamp, S_ls) of the agent's actor."""
    a = copy.deepcopy(ag.ac.actor).double()
    h = a.net(x.double())
    return (*head_terms(a.mu_layer, h), *head_terms(a.log_std_layer, h))


@torch.no_grad()
def ddpg_ref(ag, x):
    """float64 (pre-squash action, S) of the agent's actor."""
    net = copy.deepcopy(ag.ac.actor.net).double()
    h = x.double()
    for fc in net.fcs[:-1]:
        h = net.act(fc(h))
    return head_terms(net.fcs[-1], h)


class Regime:
    """Inputs and head parameters of one weight / input regime; the agent's parameters are restored on exit.
      default     the agent's init, N(0, 1) observations
      saturating  observations x 30, the action head's weights x 4 and biases +-6 (moved further out where a column's largest |u|
                  stays below 9.5): some tanh values round to +-1 in float32
      zero_rows   every third observation row all zero
    With ls_head (SAC sampling), the log_std biases alternate +10 / -40 (saturating) or -40 / +10 (zero_rows): the clamp bites at
    both ends."""

    def __init__(self, ag, name, heads, ls_head=None, pre=None):
        self.ag, self.name, self.heads, self.ls_head, self.pre = ag, name, heads, ls_head, pre

    def __enter__(self):
        self.saved = self.ag._flat['p'].clone()
        with torch.no_grad():
            if self.name == 'saturating':
                b = self.heads.bias
                self.heads.weight.mul_(4.0)
                sign = torch.tensor([1.0 if j % 2 == 0 else -1.0 for j in range(b.numel())], device=DEV)
                b.copy_(6.0 * sign)
                if self.pre is not None:        # a column whose largest |u| stays below 9.5 (one-observation tanh nets) is shifted there
                    x = self.inputs(4096, self.ag.obs_dim, torch.Generator().manual_seed(99))
                    top = (self.pre(self.ag, x) * sign).max(0).values
                    b.add_(sign * (9.5 - top).clamp(min=0.0).float())
            if self.ls_head is not None and self.name != 'default':
                b = self.ls_head.bias
                pat = (10.0, -40.0) if self.name == 'saturating' else (-40.0, 10.0)
                b.copy_(torch.tensor([pat[j % 2] for j in range(b.numel())], device=DEV))
        return self

    def inputs(self, m, nobs, gen):
        x = torch.randn(m, nobs, generator=gen).to(DEV)
        if self.name == 'saturating':
            x *= 30.0
        elif self.name == 'zero_rows':
            x[::3] = 0.0
        return x.contiguous()

    def __exit__(self, *exc):
        self.ag._flat['p'].copy_(self.saved)


def report(group, shape, worst, extra=''):
    print(f'[ratio] {group} {sid(shape)} worst error/bound {worst[0]:.4f}{extra}')


# ---------------------------------------------------------------------------------------------------------------- (a) deterministic
def sac_act(ag, D, B, x, out):
    fl = ag._flat
    _sac.check(D, D.scg_sac_act(ptr(fl['p']), C.byref(fl['actor']), B.c_lo, B.c_hi, ptr(x), x.shape[0], ptr(out), stream()))


def ddpg_act(ag, D, B, x, out):
    fl = ag._flat
    _ddpg.check(D, D.scg_ddpg_act(ptr(fl['p']), C.byref(fl['actor']), B.c_lo, B.c_hi, ptr(x), x.shape[0], ptr(out), stream()))


def ddpg_noisy_none(ag, D, B, x, out):
    fl = ag._flat
    _ddpg.check(D, D.scg_ddpg_noisy_act(ptr(fl['p']), C.byref(fl['actor']), B.c_lo, B.c_hi, ptr(x), x.shape[0], SEED, None, 0, None, None,
                                        ptr(out), stream()))


def deterministic_case(shape, family):
    nobs, _, nu, _ = shape
    ag, D = sac_agent(shape) if family == 'sac' else ddpg_agent(shape)
    calls = (('scg_sac_act', sac_act),) if family == 'sac' else (('scg_ddpg_act', ddpg_act), ('scg_ddpg_noisy_act/none', ddpg_noisy_none))
    heads = ag.ac.actor.mu_layer if family == 'sac' else ag.ac.actor.net.fcs[-1]
    pre = (lambda a, x: sac_ref(a, x)[0]) if family == 'sac' else (lambda a, x: ddpg_ref(a, x)[0])
    gen = torch.Generator().manual_seed(5)
    worst, saturated, old = [0.0], 0, []
    for regime in REGIMES:
        with Regime(ag, regime, heads, pre=pre) as R:
            for m in SIZES:
                x = R.inputs(m, nobs, gen)
                if family == 'sac':
                    u, S, _, _ = sac_ref(ag, x)
                else:
                    u, S = ddpg_ref(ag, x)
                if regime == 'saturating':
                    saturated += int((u.abs() > 9.1).sum())        # tanh rounds to +-1 in float32
                perm = torch.randperm(m, generator=gen).to(DEV)
                for cols in BOUND_SETS:
                    B = Bounds(cols, nu)
                    want, bound = B.squash(u), B.bound(u, S)
                    nar = [j for j in range(nu) if max(abs(B.lo[j]), abs(B.hi[j])) <= 2.5 and B.lo[j] != B.hi[j]]
                    if regime == 'default' and nar:  # never looser than the float32 checks' rtol 1e-5, atol 2e-6 on the narrow columns
                        old.append(float((bound[:, nar] / (1e-5 * want[:, nar].abs() + 2e-6)).median()))
                        bound[:, nar] = torch.minimum(bound[:, nar], 1e-5 * want[:, nar].abs() + 2e-6)
                    for name, fn in calls:
                        tag = f'{name} {sid(shape)} {regime} m={m} bounds={B.lo.tolist()}'
                        out = canary(m, nu)
                        fn(ag, D, B, x, out)
                        torch.cuda.synchronize()
                        got = check_out(out, m, nu, want, bound, B, tag, worst)
                        # row independence: a permuted batch permutes the outputs bit for bit
                        out_p = canary(m, nu)
                        fn(ag, D, B, x[perm].contiguous(), out_p)
                        torch.cuda.synchronize()
                        assert torch.equal(out_p[:m * nu].view(m, nu), got[perm]), f'{tag}: not row-independent'
    assert saturated > 0, 'the saturating regime never reaches tanh = +-1'
    report(f'a/{family}', shape, worst, f'; default regime, narrow columns: median uncapped bound / (1e-5 |a| + 2e-6) = '
           f'{np.median(old) if old else float("nan"):.3f}')


@pytest.mark.parametrize('shape', SAC_SHAPES, ids=sid)
def test_sac_deterministic_action(shape):
    """scg_sac_act == low + 0.5 (tanh(mu64) + 1)(high - low) within the module's deterministic tolerance (TAU = 1e-5; in the default
    regime capped at the float32 checks' 1e-5 |a| + 2e-6 on the narrow columns), at every batch size / regime / bound set; the rows
    past m stay untouched; a permuted batch permutes the outputs bit for bit."""
    deterministic_case(shape, 'sac')


@pytest.mark.parametrize('shape', DDPG_SHAPES, ids=sid)
def test_ddpg_deterministic_action(shape):
    """scg_ddpg_act and scg_ddpg_noisy_act without noise == the float64 squashed actor, tolerance as for SAC (TAU = 1e-5, capped)."""
    deterministic_case(shape, 'ddpg')


# ---------------------------------------------------------------------------------------------------------------- (b) SAC sampling
def sac_sample(ag, D, B, x, m, cnt, eps, out, uniform=0):
    fl = ag._flat
    if uniform:
        rc = D.scg_sac_sample(None, None, B.c_lo, B.c_hi, None, m, SEED, ptr(cnt), 1, None, ptr(out), stream())
    else:
        rc = D.scg_sac_sample(ptr(fl['p']), C.byref(fl['actor']), B.c_lo, B.c_hi, ptr(x), m, SEED, ptr(cnt), 0, ptr(eps), ptr(out), stream())
    _sac.check(D, rc)


def sampled_terms(mu, S_mu, ls, S_ls, eps):
    """u64 and its term magnitude: S_mu + sigma |eps| (1 + S_ls where the clamp is not active — the float32 sigma carries the
    log_std head's rounding there; a clamped log_std is exact)."""
    lsc = ls.clamp(-20.0, 2.0)
    sig = lsc.exp()
    free = ((ls > -20.0) & (ls < 2.0)).double()
    return mu + sig * eps, S_mu + sig * eps.abs() * (1.0 + free * S_ls), sig


@pytest.mark.parametrize('shape', SAC_SHAPES, ids=sid)
def test_sac_sample_with_caller_eps(shape):
    """scg_sac_sample with d_eps_in: u64 = mu64 + exp(clamp(ls64, -20, 2)) eps, tolerance of the deterministic case with
    S = S_mu + sigma |eps| (1 + S_ls where unclamped); the log_std biases +10 / -40 make the clamp bite at both ends."""
    nobs, _, nu, _ = shape
    ag, D = sac_agent(shape)
    gen = torch.Generator().manual_seed(6)
    cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
    worst, lo_hit, hi_hit = [0.0], 0, 0
    for regime in REGIMES:
        with Regime(ag, regime, ag.ac.actor.mu_layer, ag.ac.actor.log_std_layer) as R:
            for m in SIZES:
                x = R.inputs(m, nobs, gen)
                eps = torch.randn(m, nu, generator=gen).to(DEV)
                mu, S_mu, ls, S_ls = sac_ref(ag, x)
                lo_hit, hi_hit = lo_hit + int((ls < -20).sum()), hi_hit + int((ls > 2).sum())
                u, S, _ = sampled_terms(mu, S_mu, ls, S_ls, eps.double())
                perm = torch.randperm(m, generator=gen).to(DEV)
                for cols in BOUND_SETS:
                    B = Bounds(cols, nu)
                    tag = f'scg_sac_sample/eps_in {sid(shape)} {regime} m={m} bounds={B.lo.tolist()}'
                    out = canary(m, nu)
                    sac_sample(ag, D, B, x, m, cnt, eps, out)
                    torch.cuda.synchronize()
                    got = check_out(out, m, nu, B.squash(u), B.bound(u, S), B, tag, worst)
                    out_p = canary(m, nu)
                    sac_sample(ag, D, B, x[perm].contiguous(), m, cnt, eps[perm].contiguous(), out_p)
                    torch.cuda.synchronize()
                    assert torch.equal(out_p[:m * nu].view(m, nu), got[perm]), f'{tag}: not row-independent'
    assert lo_hit > 0 and hi_hit > 0, 'the log_std clamp did not bite at both ends'
    report('b/sac_eps_in', shape, worst)


@pytest.mark.parametrize('shape', SAC_SHAPES, ids=sid)
def test_sac_sample_in_kernel_draw(shape):
    """scg_sac_sample without d_eps_in: eps is tests/philox_model.normal4 at counter (*d_counter, row, 3, 0x5ac1), key (seed lo, seed hi).
    Tolerance: the eps_in case's, plus 0.5 (high - low) sech^2(u64) sigma (D_EPS (1 + |eps|) + D_LOG / r) for the kernel's __logf /
    __sincosf.
    65 536 rows at two counter words (one above 2^31)."""
    nobs, _, nu, _ = shape
    ag, D = sac_agent(shape)
    gen = torch.Generator().manual_seed(7)
    m = 65536
    x = torch.randn(m, nobs, generator=gen).to(DEV)
    mu, S_mu, ls, S_ls = sac_ref(ag, x)
    cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
    worst = [0.0]
    for k, c in enumerate((7, 0x80000001)):
        cnt.fill_(int(np.uint32(c).view(np.int32)))
        eps, tol = (torch.as_tensor(v, device=DEV) for v in draws(c, m, nu))
        u, S, sig = sampled_terms(mu, S_mu, ls, S_ls, eps)
        B = Bounds(BOUND_SETS[k], nu)
        out = canary(m, nu)
        sac_sample(ag, D, B, x, m, cnt, None, out)
        torch.cuda.synchronize()
        check_out(out, m, nu, B.squash(u), B.bound(u, S, sig * tol), B, f'scg_sac_sample/philox {sid(shape)} counter={c}', worst)
    report('b/sac_philox', shape, worst)


def uniform_bound(B, want):
    return 0.5 * torch.as_tensor(ulp32(B.hi - B.lo), device=DEV) + 0.5 * torch.as_tensor(ulp32(want.cpu().numpy()), device=DEV) + 1e-30


@pytest.mark.parametrize('shape', SAC_SHAPES, ids=sid)
def test_sac_uniform_warm_up(shape):
    """scg_sac_sample(uniform = 1): column j = low_j + (high_j - low_j) u01(w_j), w = Philox(*d_counter, row, 4, 0x5ac1), within the
    float32 expression's two roundings, 0.5 ulp32(high - low) + 0.5 ulp32(a) (high - low and u01 are exact); degenerate columns exactly
    low; nothing written past row m."""
    _, _, nu, _ = shape
    ag, D = sac_agent(shape)
    cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
    worst = [0.0]
    for m in (1, 1000, 65536 + 3):
        for k, c in enumerate((3, 0xFFFFFFFE)):
            cnt.fill_(int(np.uint32(c).view(np.int32)))
            B = Bounds(BOUND_SETS[k], nu)
            u = torch.as_tensor(pm.uniform01(SEED, c, np.arange(m))[:, :nu], device=DEV)
            out = canary(m, nu)
            sac_sample(ag, D, B, None, m, cnt, None, out, uniform=1)
            torch.cuda.synchronize()
            want = B.t_lo + (B.t_hi - B.t_lo) * u
            check_out(out, m, nu, want, uniform_bound(B, want), B, f'scg_sac_sample/uniform {sid(shape)} m={m} c={c}', worst)
    report('b/sac_uniform', shape, worst)


# ---------------------------------------------------------------------------------------------------------------- (c) DDPG noise
NARROW = [(-2.0, 1.0), (-0.5, 1.5), (-1.0, 0.25), (0.0, 3.0)]        # (c)'s bounds: the wide / degenerate columns are (a)'s business


class Noise:
    """A DdpgNoise struct over fresh device state (x_prev, x_next, calls, pending)."""

    def __init__(self, kind, theta=0.0, dt=1.0, start=0.3, end=0.05, inc=0.0, x0=(0.0,) * 4, calls=0):
        f = dict(device=DEV, dtype=torch.float64)
        self.x_prev, self.x_next = torch.tensor(list(x0), **f), torch.zeros(4, **f)
        self.calls = torch.tensor([calls], dtype=torch.int64, device=DEV)
        self.pending = torch.zeros(1, dtype=torch.int32, device=DEV)
        self.theta, self.dt, self.start, self.end, self.inc = theta, dt, start, end, inc
        self.struct = _ddpg.DdpgNoise(kind=kind, theta=theta, dt=dt, std_start=start, std_end=end, std_inc=inc, d_x_prev=ptr(self.x_prev),
                                      d_x_next=ptr(self.x_next), d_calls=ptr(self.calls), d_pending=ptr(self.pending))

    def std(self, calls0, m):
        v = self.start + (calls0 + np.arange(m)) * self.inc
        return np.minimum(v, self.end) if self.end > self.start else np.maximum(v, self.end)


def ddpg_noisy(ag, D, B, x, m, cnt, nz, eps, out, uniform=0):
    fl = ag._flat
    p, lay = (None, None) if uniform else (ptr(fl['p']), C.byref(fl['actor']))
    _ddpg.check(D, D.scg_ddpg_noisy_act(p, lay, B.c_lo, B.c_hi, None if uniform else ptr(x), m, SEED, ptr(cnt), uniform,
                                        None if nz is None else C.byref(nz.struct), ptr(eps), ptr(out), stream()))


def launch_and_commit(ag, D, B, x, m, cnt, nz, eps, out):
    """One noisy launch: before the commit, x_prev / calls unchanged and pending = m; after it, pending = 0."""
    x_prev, calls = nz.x_prev.clone(), int(nz.calls)
    ddpg_noisy(ag, D, B, x, m, cnt, nz, eps, out)
    torch.cuda.synchronize()
    assert torch.equal(nz.x_prev, x_prev) and int(nz.calls) == calls and int(nz.pending) == m, 'launch without commit moved the process'
    _ddpg.check(D, D.scg_ddpg_noise_commit(C.byref(nz.struct), stream()))
    torch.cuda.synchronize()
    assert int(nz.calls) == calls + m and int(nz.pending) == 0


@pytest.mark.parametrize('shape', DDPG_SHAPES, ids=sid)
def test_ddpg_gaussian_noise(shape):
    """Gaussian process with the in-kernel draw: a = f32(a64 + std(calls + i) eps64_i), eps64 = normal4 (stream 3) at the counter word;
    tolerance: the deterministic one + std (D_EPS (1 + |eps|) + D_LOG / r) + ulp32(a) of the final rounding.  Three consecutive calls per batch size,
    the std schedule reaching its end inside them; calls advances by m per commit only."""
    nobs, _, nu, _ = shape
    ag, D = ddpg_agent(shape)
    gen = torch.Generator().manual_seed(8)
    B = Bounds(NARROW, nu)
    cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
    worst = [0.0]
    for m in (1000, 70000):
        nz = Noise(_ddpg.NOISE_GAUSSIAN, start=0.3, end=0.05, inc=(0.05 - 0.3) / (1.5 * m), calls=17)
        for call in range(3):
            c = 100 + call
            cnt.fill_(c)
            x = torch.randn(m, nobs, generator=gen).to(DEV)
            u, S = ddpg_ref(ag, x)
            calls0 = int(nz.calls)
            sd = torch.as_tensor(nz.std(calls0, m), device=DEV)[:, None]
            eps, tol = (torch.as_tensor(v, device=DEV) for v in draws(c, m, nu))
            want = B.squash(u) + sd * eps
            bound = B.bound(u, S) + sd * tol + torch.as_tensor(ulp32(want.cpu().numpy()), device=DEV)
            out = canary(m, nu)
            launch_and_commit(ag, D, B, x, m, cnt, nz, None, out)
            check_out(out, m, nu, want, bound, B, f'gaussian {sid(shape)} m={m} call={call}', worst)
            assert torch.equal(nz.x_prev, torch.zeros(4, dtype=torch.float64, device=DEV))
    report('c/ddpg_gaussian', shape, worst)


def ou_reference(eps, x0, sd, a, sqrt_dt, e0=None, tol=None):
    """float64 sequential x_i = a x_{i-1} + sd_i sqrt(dt) eps_i from x_{-1} = x0, per column; with tol (the allowed draw error of each
    eps), also the propagated bound e_i = |a| e_{i-1} + sd_i sqrt(dt) tol_i from e0."""
    b = (sd * sqrt_dt)[:, None]
    x = np.stack([lfilter([1.0], [1.0, -a], b[:, 0] * eps[:, j], zi=[a * x0[j]])[0] for j in range(eps.shape[1])], axis=1)
    if tol is None:
        return x, None
    e = np.stack([lfilter([1.0], [1.0, -abs(a)], b[:, 0] * tol[:, j], zi=[abs(a) * e0[j]])[0]
                  for j in range(eps.shape[1])], axis=1)
    return x, e


OU_THETA = {0.0015: 0.15, 0.5: 50.0, 0.0: 0.0, 1.5: 150.0}          # theta dt -> theta at dt = 0.01


@pytest.mark.parametrize('theta_dt', list(OU_THETA), ids=lambda v: f'thdt{v}')
@pytest.mark.parametrize('shape', DDPG_SHAPES, ids=sid)
def test_ddpg_ou_noise(shape, theta_dt):
    """Ornstein-Uhlenbeck process (the shipped theta dt = 0.0015; 0.5: a 50-env window, every workgroup past the first truncates; 0: a
    random walk, nothing truncates; 1.5: a = -0.5, an oscillating contraction), m in {1000, 70 000}, three consecutive calls from a
    non-zero carry, against the float64 sequential recurrence:
      draws through d_eps_in (float32 normal4 values): actions at atol 1e-5, x_prev to 1e-12 of the call's largest |x|;
      the in-kernel draw: the same plus the propagated draw-error bound (ou_reference's e) on the actions and on x_prev.
    calls advances by m per commit exactly."""
    nobs, _, nu, _ = shape
    ag, D = ddpg_agent(shape)
    theta, dt = OU_THETA[theta_dt], 0.01
    B = Bounds(NARROW, nu)
    cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
    worst = [0.0]
    for mode in ('eps_in', 'philox'):
        gen = torch.Generator().manual_seed(9)
        for m in (1000, 70000):
            x0 = np.array([0.3, -0.2, 0.1, 0.05])
            nz = Noise(_ddpg.NOISE_OU, theta=theta, dt=dt, start=0.3, end=0.05, inc=(0.05 - 0.3) / 50000, x0=x0, calls=1000)
            a = 1.0 - theta * dt
            xr, er = x0[:nu].copy(), np.zeros(nu)
            for call in range(3):
                c = 200 + call
                cnt.fill_(c)
                x = torch.randn(m, nobs, generator=gen).to(DEV)
                u, S = ddpg_ref(ag, x)
                calls0 = int(nz.calls)
                eps64, tol = draws(c, m, nu)
                if mode == 'eps_in':
                    eps32 = torch.as_tensor(eps64, dtype=torch.float32, device=DEV).contiguous()
                    ref, err = ou_reference(eps32.double().cpu().numpy(), xr, nz.std(calls0, m), a, np.sqrt(dt))
                    err = np.zeros_like(ref)
                else:
                    eps32 = None
                    ref, err = ou_reference(eps64, xr, nz.std(calls0, m), a, np.sqrt(dt), er, tol)
                out = canary(m, nu)
                launch_and_commit(ag, D, B, x, m, cnt, nz, eps32, out)
                want = B.squash(u) + torch.as_tensor(ref, device=DEV)
                bound = 1e-5 + torch.as_tensor(err, device=DEV)
                tag = f'ou {sid(shape)} theta_dt={theta_dt} {mode} m={m} call={call}'
                check_out(out, m, nu, want, bound, B, tag, worst)
                scale = np.abs(ref).max(axis=0)
                got_x = nz.x_prev[:nu].cpu().numpy()
                assert np.all(np.abs(got_x - ref[-1]) <= 1e-12 * scale + err[-1]), f'{tag}: x_prev {got_x} vs {ref[-1]}'
                assert int(nz.calls) == calls0 + m
                xr, er = ref[-1].copy(), err[-1].copy()
    report(f'c/ddpg_ou_{theta_dt}', shape, worst)


@pytest.mark.parametrize('shape', DDPG_SHAPES, ids=sid)
def test_ddpg_uniform_warm_up(shape):
    """scg_ddpg_noisy_act(uniform = 1): as scg_sac_sample's warm-up (the expression's two float32 roundings, canary), and it clears
    pending without advancing the process."""
    _, _, nu, _ = shape
    ag, D = ddpg_agent(shape)
    cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
    worst = [0.0]
    for m in (1, 1000, 65536 + 3):
        for k, c in enumerate((3, 0xFFFFFFFE)):
            cnt.fill_(int(np.uint32(c).view(np.int32)))
            B = Bounds(BOUND_SETS[k], nu)
            nz = Noise(_ddpg.NOISE_OU, theta=0.15, dt=0.01, x0=(0.1, 0.2, 0.3, 0.4), calls=5)
            nz.pending.fill_(9)
            u = torch.as_tensor(pm.uniform01(SEED, c, np.arange(m))[:, :nu], device=DEV)
            out = canary(m, nu)
            ddpg_noisy(ag, D, B, None, m, cnt, nz, None, out, uniform=1)
            torch.cuda.synchronize()
            want = B.t_lo + (B.t_hi - B.t_lo) * u
            check_out(out, m, nu, want, uniform_bound(B, want), B, f'ddpg uniform {sid(shape)} m={m} c={c}', worst)
            assert int(nz.pending) == 0 and int(nz.calls) == 5 and nz.x_prev.tolist() == [0.1, 0.2, 0.3, 0.4]
    report('c/ddpg_uniform', shape, worst)


def test_in_kernel_draw_readout():
    """The in-kernel N(0, 1) draw read out directly: Gaussian noise of std 2^20 swamps the action, so (a - a64) / 2^20 is the kernel's
    eps to ~1e-7.  Checks |eps_kernel - eps64| <= D_EPS (1 + |eps|) + D_LOG / r and prints the two constants' measured counterparts:
    max |d eps| r where r < 0.05 (the __logf term) and max |d eps| / (1 + |eps|) where r >= 0.05.  The SAC library compiles the same
    normal4 (scg_wide.h holds the one definition), pinned within the same allowance through test_sac_sample_in_kernel_draw."""
    shape = (24, 128, 4, 'relu')
    ag, D = ddpg_agent(shape)
    B = Bounds(NARROW, 4)
    gen = torch.Generator().manual_seed(10)
    cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
    m, big = 1 << 20, 2.0 ** 20
    q_log = q_lin = worst = 0.0
    for c in (0, 0x7FFFFFFF):
        cnt.fill_(c)
        x = torch.randn(m, 24, generator=gen).to(DEV)
        u, _ = ddpg_ref(ag, x)
        nz = Noise(_ddpg.NOISE_GAUSSIAN, start=big, end=big, inc=0.0)
        out = canary(m, 4)
        launch_and_commit(ag, D, B, x, m, cnt, nz, None, out)
        e_k = ((out[:m * 4].view(m, 4).double() - B.squash(u)) / big).cpu().numpy()
        e64, tol = draws(c, m, 4)
        r = D_LOG / (tol - D_EPS * (1.0 + np.abs(e64)))
        d = np.abs(e_k - e64)
        q_log = max(q_log, float(np.max(np.where(r < 0.05, d * r, 0.0))))
        q_lin = max(q_lin, float(np.max(np.where(r >= 0.05, d / (1.0 + np.abs(e64)), 0.0))))
        worst = max(worst, float(np.max(d / tol)))
    print(f'[ratio] draw readout: max |d eps| r (r < 0.05) = {q_log:.3g} (D_LOG {D_LOG:g}), max |d eps| / (1 + |eps|) (r >= 0.05) = '
          f'{q_lin:.3g} (D_EPS {D_EPS:g}), worst |d eps| / allowance = {worst:.3f}')
    assert worst <= 1.0


# ---------------------------------------------------------------------------------------------------------------- (d) ring push
def bits(t):
    return np.ascontiguousarray(t.detach().cpu().numpy()).view(np.uint8)


class Ring:
    def __init__(self, cap, nobs, nu, start, counter=11):
        f = dict(device=DEV, dtype=torch.float32)
        nan = float('nan')
        self.cap = cap
        self.obs, self.next_obs = torch.full((cap, nobs), nan, **f), torch.full((cap, nobs), nan, **f)
        self.act, self.rew, self.mask = torch.full((cap, nu), nan, **f), torch.full((cap,), nan, **f), torch.full((cap,), nan, **f)
        self.pos = torch.tensor(start, dtype=torch.int64, device=DEV)
        self.size_f = torch.tensor(float(start), **f)
        self.size_i32 = torch.tensor([start], dtype=torch.int32, device=DEV)
        self.counter = torch.tensor([counter], dtype=torch.int32, device=DEV)
        kw = dict(d_obs=ptr(self.obs), d_act=ptr(self.act), d_rew=ptr(self.rew), d_next_obs=ptr(self.next_obs), d_mask=ptr(self.mask), capacity=cap,
                  d_pos=ptr(self.pos), d_size_f=ptr(self.size_f), d_size_i32=ptr(self.size_i32), d_counter=ptr(self.counter))
        self.sac, self.ddpg = _sac.SacRing(**kw), _ddpg.DdpgRing(**kw)
        self.host = {k: getattr(self, k).cpu().numpy().copy() for k in ('obs', 'act', 'rew', 'next_obs', 'mask', 'pos', 'size_f', 'size_i32', 'counter')}

    def host_push(self, cur, act, rew, nxt, term, done, flags):
        """The push with the time-limit fix-up: a truncated row stores the terminal observation with mask 1."""
        H, n = self.host, cur.shape[0]
        slot = (int(H['pos']) + np.arange(n)) % self.cap
        trunc = (done != 0) & ((flags & 1) != 0)
        H['obs'][slot], H['act'][slot], H['rew'][slot] = cur, act, rew
        H['next_obs'][slot] = np.where(trunc[:, None], term, nxt)
        H['mask'][slot] = np.where(trunc, np.float32(1.0), np.where(done != 0, np.float32(0.0), np.float32(1.0)))
        H['pos'] = np.int64((int(H['pos']) + n) % self.cap)
        H['size_f'] = np.float32(min(float(H['size_f']) + n, self.cap))
        H['size_i32'] = np.minimum(H['size_i32'] + n, self.cap).astype(np.int32)
        H['counter'] = (H['counter'] + 1).astype(np.int32)

    def check(self, tag):
        for k, want in self.host.items():
            assert np.array_equal(bits(getattr(self, k)), np.ascontiguousarray(want).view(np.uint8)), f'{tag}: ring {k} differs'


def push_batches(n, nobs, nu, gen, steps=4):
    for _ in range(steps):
        r = lambda *s: torch.randn(*s, generator=gen)      # noqa: E731
        done = (torch.rand(n, generator=gen) < 0.3).to(torch.uint8)
        flags = torch.randint(0, 4, (n,), generator=gen).to(torch.uint8)           # bit 0 = truncated by the time limit
        yield r(n, nu), r(n), r(n, nobs), r(n, nobs), done, flags


RING_CASES = [(1, 3, 0), (1, 3, 2), (300, 700, 0), (300, 700, 699)]             # (n, capacity, start position)


def ring_case(shape, family, n, cap, start):
    nobs, _, nu, _ = shape
    ag, D = sac_agent(shape) if family == 'sac' else ddpg_agent(shape)
    gen = torch.Generator().manual_seed(12 + n + start)
    R = Ring(cap, nobs, nu, start)
    cur = torch.randn(n, nobs, generator=gen)
    cur_d = cur.to(DEV)
    if family == 'ddpg':
        ou = Noise(_ddpg.NOISE_OU, theta=0.15, dt=0.01, x0=(0.1, -0.1, 0.2, -0.2), calls=40)
        gs = Noise(_ddpg.NOISE_GAUSSIAN, calls=7)
        B = Bounds(NARROW, nu)
        cnt = torch.zeros(1, dtype=torch.int32, device=DEV)
    for step, (act, rew, nxt, term, done, flags) in enumerate(push_batches(n, nobs, nu, gen)):
        dv = [t.to(DEV).contiguous() for t in (act, rew, nxt, term, done, flags)]
        tag = f'{family} push {sid(shape)} n={n} cap={cap} start={start} step={step}'
        if family == 'sac':
            _sac.check(D, D.scg_sac_push(C.byref(R.sac), ptr(cur_d), *[ptr(t) for t in dv], n, stream()))
        else:
            # the bookkeeping launch's commit: 0 after an OU launch, 1 with nothing pending, 2 after a Gaussian launch, 3 no process
            nz = (ou, ou, gs, None)[step]
            if step in (0, 2):
                ddpg_noisy(ag, D, B, cur_d, n, cnt, nz, None, torch.empty(n * nu, device=DEV))
            torch.cuda.synchronize()
            before = None if nz is None else (nz.x_prev.clone(), nz.x_next.clone(), int(nz.calls), int(nz.pending))
            _ddpg.check(D, D.scg_ddpg_push(C.byref(R.ddpg), None if nz is None else C.byref(nz.struct), ptr(cur_d), *[ptr(t) for t in dv], n,
                                           stream()))
        torch.cuda.synchronize()
        R.host_push(cur.numpy(), act.numpy(), rew.numpy(), nxt.numpy(), term.numpy(), done.numpy(), flags.numpy())
        cur = nxt.clone()
        R.check(tag)
        assert np.array_equal(bits(cur_d), bits(cur)), f'{tag}: current observation batch'
        if family == 'ddpg' and nz is not None:
            x_prev, x_next, calls, pending = before
            assert pending == (n if step in (0, 2) else 0), tag
            assert int(nz.pending) == 0 and int(nz.calls) == calls + pending, tag
            want_x = torch.cat([x_next[:nu], x_prev[nu:]]) if step == 0 else x_prev       # the process has act_dim columns
            assert torch.equal(nz.x_prev, want_x), f'{tag}: x_prev after the commit'


@pytest.mark.parametrize('n,cap,start', RING_CASES)
@pytest.mark.parametrize('shape', SAC_SHAPES, ids=sid)
def test_sac_ring_push(shape, n, cap, start):
    """scg_sac_push, four pushes (the ring wraps) into a NaN-filled ring, against the host model: ring rows, the current-observation
    batch, pos, size_f, size_i32 and counter, bit for bit."""
    ring_case(shape, 'sac', n, cap, start)


@pytest.mark.parametrize('n,cap,start', RING_CASES)
@pytest.mark.parametrize('shape', DDPG_SHAPES, ids=sid)
def test_ddpg_ring_push(shape, n, cap, start):
    """scg_ddpg_push as scg_sac_push, bit for bit, plus the noise commit of its bookkeeping launch after an OU launch (x_prev <- x_next,
    calls += pending), with nothing pending (no change), after a Gaussian launch (calls only) and without a process."""
    ring_case(shape, 'ddpg', n, cap, start)

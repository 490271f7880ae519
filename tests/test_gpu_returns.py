"""scg_ppo_returns_prepare / _moments / _normalise (csrc/scg_learn.hip: the collector's work between rollout and update) against a
float64 NumPy reference: ill-conditioned advantages, every launch geometry, moments summed over shards, and the chain as PPO runs it.

Reference and bound: tests/returns_cases.py — float64 `(a - a.mean()) / (a.std() + 1e-6)`; bound = 4 x the deviation of that same line
in NumPy float32 (the yardstick: what the reference achieves, never the code under test) + 2 float32 ulps of max |reference|.

MEASURED (MI355X; max |out - float64 reference| as test_normalise_holds_the_reference_bound_on_ill_conditioned_input and test_exact_cases
print it; last column: the same inputs through the kernels before the moments became float64, which miss the bound from |mean| / std = 10 on):
case                              yardstick      bound  deviation   parent commit (float32 one-pass): deviation
mean0.5_std3_M7x1000              3.562e-07  1.902e-06  1.186e-07    4.045e-07 passes
mean10_std1_M7x1000               3.514e-07  1.882e-06  1.189e-07    4.491e-05 FAILS
mean30_std0.3_M7x1000             1.891e-06  8.039e-06  1.192e-07    1.036e-03 FAILS
mean100_std0.5_M7x1000            3.439e-06  1.423e-05  1.188e-07    1.599e-03 FAILS
mean-300_std0.3_M7x1000           7.082e-05  2.837e-04  1.187e-07    2.701e-01 FAILS
mean1000_std0.1_M7x1000           5.676e-04  2.271e-03  1.239e-07    3.929e+05 FAILS
mean0.5_std3_M5x52429             4.633e-07  2.807e-06  2.189e-07    5.589e-07 passes
mean10_std1_M5x52429              3.513e-07  2.359e-06  2.347e-07    4.704e-06 FAILS
mean30_std0.3_M5x52429            5.545e-06  2.313e-05  2.286e-07    7.200e-04 FAILS
mean100_std0.5_M5x52429           1.863e-05  7.548e-05  2.205e-07    8.537e-04 FAILS
mean-300_std0.3_M5x52429          1.961e-04  7.855e-04  2.211e-07    4.735e-01 FAILS
mean1000_std0.1_M5x52429          6.397e-04  2.560e-03  2.334e-07    3.042e+00 FAILS
constant_0.5_M4096                0.000e+00  2.803e-45  0.000e+00    0.000e+00 passes
single_element                    0.000e+00  2.803e-45  0.000e+00    0.000e+00 passes
half_64_half_65                   2.656e-08  2.255e-07  2.656e-08    2.656e-08 passes
"""
import ctypes as C

import numpy as np
import pytest

from tests import returns_cases as rc

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

PAD = 64                            # every output buffer is this much too long; the tail must come back untouched


class _Launches:
    """The three launches on padded device buffers.  Outputs are pre-filled with NaN (0xFF bytes) and come back as (body, tail)."""

    def __init__(self):
        from safe_control_gym_amd import _learn
        self.learn = _learn
        self.D = _learn.lib(12, 128, 2, 'tanh')
        self.dev = torch.device('cuda:0')
        self.scratch_bytes = int(self.D.scg_ppo_returns_scratch_bytes())
        assert self.scratch_bytes % 8 == 0

    def st(self):
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def dev_in(self, a):
        return torch.as_tensor(np.ascontiguousarray(a), device=self.dev)

    def padded(self, n, dtype):
        """n + PAD elements of `dtype`, every byte 0xFF (NaN for the floating types)."""
        return torch.full(((n + PAD) * torch.empty((), dtype=dtype).element_size(),), 0xFF, dtype=torch.uint8, device=self.dev).view(dtype)

    @staticmethod
    def tail_untouched(t, n):
        return bool((t[n:].contiguous().view(torch.uint8) == 0xFF).all())

    def moments(self, adv, T, N, acc=None, totals=None):
        """adv: device float32 [>= T N].  Returns the device moments buffer (float64 [3 + PAD]) after checking the scratch's tail."""
        scratch = self.padded(self.scratch_bytes // 8, torch.float64)
        mom = self.padded(3, torch.float64)
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None                               # noqa: E731
        self.learn.check(self.D, self.D.scg_ppo_returns_moments(p(adv), T, N, p(acc), p(scratch), p(mom), p(totals), self.st()))
        torch.cuda.synchronize()
        assert self.tail_untouched(scratch, self.scratch_bytes // 8) and self.tail_untouched(mom, 3)
        return mom

    def normalise(self, adv, mom, T, N, out=None):
        out = self.padded(T * N, torch.float32) if out is None else out
        self.learn.check(self.D, self.D.scg_ppo_returns_normalise(C.c_void_p(adv.data_ptr()), C.c_void_p(mom.data_ptr()), T, N,
                                                                  C.c_void_p(out.data_ptr()), self.st()))
        torch.cuda.synchronize()
        assert self.tail_untouched(out, T * N)
        return out

    def both(self, a, T, N):
        """moments then normalise on the host array a [T N]: (moments [3] float64, out [T N] float32) as NumPy."""
        adv = self.dev_in(a)
        mom = self.moments(adv, T, N)
        out = self.normalise(adv, mom, T, N)
        return mom[:3].cpu().numpy(), out[:T * N].cpu().numpy()


@pytest.fixture(scope='module')
def L():
    return _Launches()


# ---------------------------------------------------------------------------------------------------------------- (a) conditioning
@pytest.mark.parametrize('name,mean,std,T,N', rc.drawn_cases(), ids=[c[0] for c in rc.drawn_cases()])
def test_normalise_holds_the_reference_bound_on_ill_conditioned_input(L, name, mean, std, T, N):
    """|mean| / std from 0.17 to 1e4: a one-pass variance in float32 loses every digit from 1e3 on (and misses this bound from 1e2 on)."""
    a = rc.draw(mean, std, T * N, seed=T * N + int(abs(mean)))
    mom, out = L.both(a, T, N)
    _, b, d = rc.report(name, a, out)
    rc.check_moments(mom, a)
    assert d <= b


@pytest.mark.parametrize('name', list(rc.exact_cases()))
def test_exact_cases(L, name):
    a, closed = rc.exact_cases()[name]
    mom, out = L.both(a, 1, a.size)
    _, b, d = rc.report(name, a, out)
    rc.check_moments(mom, a)
    assert d <= b
    if not closed.any():
        assert (out == 0).all()                     # a constant batch, a batch of one: exactly 0
    else:
        assert np.abs(out.astype(np.float64) - closed).max() <= b


# ---------------------------------------------------------------------------------------------------------------- (b) launch geometry
GEOMETRY = [(1, 1), (1, 2), (1, 255), (1, 257),             # a partial single block (and one element into the second)
            (7, 1000), (16, 1024),
            (3, 21846),                                     # 65 538: two elements past one per thread under the moments launch's 256-block cap
            (1, 70001),                                     # the strided loop over the episode-accumulator rows
            (5, 52429),
            (3, 349527)]                                    # 1 048 581: past the 4096-block cap of prepare and one trip of normalise's 1024 blocks


@pytest.mark.parametrize('T,N', GEOMETRY)
def test_launch_geometry(L, T, N):
    M = T * N
    rng = np.random.default_rng(1000 * T + N)
    p = lambda t: C.c_void_p(t.data_ptr())                                                              # noqa: E731
    # prepare: exact outputs, bit-equal copies
    done = (rng.uniform(size=M) < 0.2).astype(np.uint8)
    flags = rng.integers(0, 256, M, dtype=np.uint8)
    rew, v_all = rng.standard_normal(M).astype(np.float32), rng.standard_normal(M + N).astype(np.float32)
    trunc, mask, rew_c, v = L.padded(M, torch.uint8), L.padded(M, torch.float32), L.padded(M, torch.float32), L.padded(M, torch.float32)
    ins = [L.dev_in(x) for x in (done, flags, rew, v_all)]          # (held: a freed input's memory would be handed to the next one)
    L.learn.check(L.D, L.D.scg_ppo_returns_prepare(*[p(t) for t in ins], T, N, p(trunc), p(mask), p(rew_c), p(v), L.st()))
    torch.cuda.synchronize()
    for t in (trunc, mask, rew_c, v):
        assert L.tail_untouched(t, M)
    assert np.array_equal(trunc[:M].cpu().numpy(), (flags & 1) & done)
    assert np.array_equal(mask[:M].cpu().numpy().view(np.uint32), (1.0 - done.astype(np.float32)).view(np.uint32))
    assert np.array_equal(rew_c[:M].cpu().numpy().view(np.uint32), rew.view(np.uint32))
    assert np.array_equal(v[:M].cpu().numpy().view(np.uint32), v_all[:M].view(np.uint32))
    # moments with episode accumulators: small integer-valued floats, so that every column total (< 2^24) is exact in float32 in any order
    a = rc.draw(0.5, 3.0, M, seed=M)
    adv = L.dev_in(a)
    acc_h = rng.integers(0, 16, (N, 8)).astype(np.float32)
    start = np.array([1.0, 2.0, 3.0, 4.0], np.float32)
    assert acc_h.astype(np.int64).sum(0).max() + 4 < 2 ** 24
    acc, totals = L.padded(N * 8, torch.float32), L.padded(4, torch.float32)
    acc[:N * 8].copy_(L.dev_in(acc_h.reshape(-1)))
    totals[:4].copy_(L.dev_in(start))
    mom = L.moments(adv, T, N, acc=acc, totals=totals)
    assert L.tail_untouched(acc, N * 8) and L.tail_untouched(totals, 4)
    rc.check_moments(mom[:3].cpu().numpy(), a)
    assert np.array_equal(totals[:4].cpu().numpy().astype(np.int64), start.astype(np.int64) + acc_h.astype(np.int64).sum(0)[:4])
    assert np.array_equal(acc[:N * 8].cpu().numpy().view(np.uint32), np.zeros(N * 8, np.uint32))      # all eight columns of every row: +0
    # normalise out of place: body fully written (finite, within the bound), tail untouched (L.normalise)
    out = L.normalise(adv, mom, T, N)
    out_h = out[:M].cpu().numpy()
    _, b, d = rc.report(f'geometry {T}x{N}', a, out_h)
    assert d <= b
    # a null accumulator pointer: the running totals are left alone; the same moments, bit for bit
    before = totals.clone()
    mom2 = L.moments(adv, T, N, acc=None, totals=totals)
    assert torch.equal(totals.view(torch.int32), before.view(torch.int32))
    assert torch.equal(mom2[:3].view(torch.int64), mom[:3].view(torch.int64))
    # in place == out of place, bit for bit
    adv_io = L.padded(M, torch.float32)
    adv_io[:M].copy_(adv)
    L.normalise(adv_io, mom, T, N, out=adv_io)
    assert np.array_equal(adv_io[:M].cpu().numpy().view(np.uint32), out_h.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------- (c) shards
def test_moments_summed_over_unequal_shards(L):
    """What four ranks do, on one device: each shard's moments from the kernel, summed by the tensor add the all-reduce performs, every
    shard normalised with the sum — against the float64 reference of the whole array.  The same through the PyTorch helpers."""
    from safe_control_gym_amd.ppo import advantage_moments, normalise_advantages
    parts = rc.shards()
    whole = np.concatenate(parts)
    devs = [L.dev_in(s) for s in parts]
    total = torch.zeros(3, dtype=torch.float64, device=L.dev)
    for d_, s in zip(devs, parts):
        total += L.moments(d_, 1, s.size)[:3]
    rc.check_moments(total.cpu().numpy(), whole)
    out = np.concatenate([L.normalise(d_, total, 1, s.size)[:s.size].cpu().numpy() for d_, s in zip(devs, parts)])
    _, b, d = rc.report('four shards (kernels)', whole, out)
    assert d <= b
    total_t = torch.zeros(3, dtype=torch.float64, device=L.dev)
    for d_ in devs:
        total_t += advantage_moments(d_)
    rc.check_moments(total_t.cpu().numpy(), whole)
    out_t = np.concatenate([normalise_advantages(d_, total_t).cpu().numpy() for d_ in devs])
    _, b, d = rc.report('four shards (torch helpers)', whole, out_t)
    assert d <= b


# ---------------------------------------------------------------------------------------------------------------- (d) the trainer's chain
@pytest.mark.parametrize('use_gae', [True, False])
@pytest.mark.parametrize('N,T', [(1024, 20),            # scg_gae: gae_seg_kernel
                                 (320, 8)])             # scg_gae: gae_env_kernel
def test_collector_chain_against_float64(N, T, use_gae):
    """PPO._collect_fused() then _normalised on cartpole_stab with 15-step episodes, recomputed in float64 from the trainer's own
    buffers: returns and advantages from rew / done / flags, a float64 copy of the critic on obs and term_obs and the oracle's
    compute_returns_and_advantages; the normalised advantages from the kernel's own adv; the episode count from done."""
    from oracle.vec import compute_returns_and_advantages
    from safe_control_gym_amd.ppo import MLP, PPO, PPOConfig
    from safe_control_gym_amd.registration import load_task
    from safe_control_gym_amd.vec_env import HipVecEnv
    env_id, cfg = load_task(rc.CHAIN_TASK)
    hidden, act = rc.CHAIN_POLICY
    env = HipVecEnv(env_id, N, seed=7, return_numpy=False, policy=rc.CHAIN_POLICY, **dict(cfg, **rc.CHAIN_OVERRIDE))
    torch.manual_seed(0)
    ppo = PPO(env, PPOConfig(hidden_dim=hidden, activation=act, use_gae=use_gae, rollout_batch_size=N, rollout_steps=T,
                             mini_batch_size=N * T // 2, opt_epochs=1), seed=0)
    assert ppo._fused_rollout and ppo.agent.use_fused
    critic64 = MLP(ppo.obs_dim, 1, [hidden, hidden], act).double()
    critic64.load_state_dict({k: v.detach().double().cpu() for k, v in ppo.agent.ac.critic.v_net.state_dict().items()})
    seen_trunc = seen_term = 0
    for it in range(2):                                 # the second collection of the T = 8 case holds step 15 of the first episodes
        count0 = float(ppo._ep_tot[0])
        ret, adv, mom = ppo._collect_fused()
        ret_h, adv_h = ret.cpu().numpy(), adv.cpu().numpy()         # (before _normalised: the GAE outputs are reused buffers)
        adv_n = ppo._normalised(adv, mom).cpu().numpy()
        torch.cuda.synchronize()
        done, flags = ppo.done.cpu().numpy(), ppo.flags.cpu().numpy()
        trunc = ((flags & 1) & done).astype(bool)
        seen_trunc += int(trunc.sum())
        seen_term += int((done.astype(bool) & ~trunc).sum())
        with torch.no_grad():
            v_all = critic64(ppo.obs.double().cpu()).squeeze(-1).numpy()                    # [T + 1][N]
            tv = critic64(ppo.term_obs.double().cpu()).squeeze(-1).numpy() * trunc
        rew = ppo.rew.double().cpu().numpy()
        ret_o, adv_o = compute_returns_and_advantages(rew[..., None].copy(), v_all[:T, :, None], (1.0 - done)[..., None].astype(np.float64),
                                                      tv[..., None], v_all[T][:, None], ppo.cfg.gamma, use_gae, ppo.cfg.gae_lambda)
        scale = max(1.0, float(np.abs(ret_o).max()))
        np.testing.assert_allclose(ret_h / scale, ret_o[..., 0] / scale, rtol=3e-4, atol=3e-4)
        np.testing.assert_allclose(adv_h / scale, adv_o[..., 0] / scale, rtol=3e-4, atol=3e-4)
        rc.check_moments(mom.cpu().numpy(), adv_h)
        _, b, d = rc.report(f'chain N={N} T={T} gae={use_gae} #{it}', adv_h, adv_n)
        assert d <= b
        assert float(ppo._ep_tot[0]) - count0 == float(done.sum())
        assert not ppo._episode_acc.any()
    assert seen_trunc > 0 and seen_term > 0, (seen_trunc, seen_term)
    env.close()

"""ppo.advantage_moments / ppo.normalise_advantages — the one PyTorch implementation of the global advantage normalisation that PPO,
RARL, RAP and Safe-Explorer PPO share — on CPU tensors, against the float64 reference and under the measured bound of
tests/returns_cases.py: ill-conditioned inputs (|mean| / std up to 1e4, where the float32 one-pass variance sum a^2 / n - mean^2 these
trainers used before has no digit left), the exact cases, and moments summed over unequal shards the way the ranks' all-reduce sums them."""
import numpy as np
import pytest

from tests import returns_cases as rc

torch = pytest.importorskip('torch')


def _normalise(a, device='cpu'):
    from safe_control_gym_amd.ppo import advantage_moments, normalise_advantages
    t = torch.as_tensor(a, device=device)
    mom = advantage_moments(t)
    out = normalise_advantages(t, mom)
    assert mom.dtype == torch.float64 and mom.shape == (3,) and out.dtype == torch.float32 and out.shape == t.shape
    return mom.cpu().numpy(), out.cpu().numpy()


@pytest.mark.parametrize('name,mean,std,T,N', rc.drawn_cases(), ids=[c[0] for c in rc.drawn_cases()])
def test_helpers_hold_the_reference_bound_on_ill_conditioned_input(name, mean, std, T, N):
    a = rc.draw(mean, std, T * N, seed=T * N + int(abs(mean)))
    mom, out = _normalise(a.reshape(T, N))
    _, b, d = rc.report(name, a, out)
    rc.check_moments(mom, a)
    assert d <= b


@pytest.mark.parametrize('name', list(rc.exact_cases()))
def test_helpers_exact_cases(name):
    a, closed = rc.exact_cases()[name]
    mom, out = _normalise(a)
    _, b, d = rc.report(name, a, out)
    rc.check_moments(mom, a)
    assert d <= b
    if not closed.any():
        assert (out == 0).all()                     # a constant batch, a batch of one: exactly 0
    else:
        assert np.abs(out.astype(np.float64) - closed).max() <= b


def test_helpers_moments_summed_over_unequal_shards():
    from safe_control_gym_amd.ppo import advantage_moments, normalise_advantages
    parts = rc.shards()
    whole = np.concatenate(parts)
    ts = [torch.as_tensor(p) for p in parts]
    total = torch.zeros(3, dtype=torch.float64)
    for t in ts:
        total += advantage_moments(t)               # the SUM all-reduce, one rank at a time
    rc.check_moments(total.numpy(), whole)
    out = np.concatenate([normalise_advantages(t, total).numpy() for t in ts])
    _, b, d = rc.report('four shards', whole, out)
    assert d <= b


def test_rarl_wrapper_is_the_helper():
    from safe_control_gym_amd import rarl
    from safe_control_gym_amd.ppo import advantage_moments, normalise_advantages
    t = torch.as_tensor(rc.draw(-300.0, 0.3, 7000, seed=1))
    assert torch.equal(rarl._normalised(t, advantage_moments(t)), normalise_advantages(t, advantage_moments(t)))

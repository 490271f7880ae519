"""The width-256 actor rollout's host side, without a GPU: which shapes are served (_lib.actor_supported against policy_supported), the
library names of the wide variants, FlatAgent.packed_actor() on CPU agents, the controller key and the served-or-not decision
(controllers.offpolicy_fused_shape)."""
import itertools
import warnings
from types import SimpleNamespace

import pytest

torch = pytest.importorskip('torch')

from safe_control_gym_amd import _cbf, controllers  # noqa: E402
from safe_control_gym_amd import _lib as L  # noqa: E402

ACTS = ('tanh', 'relu', 'leaky_relu')


def test_actor_supported_adds_256_and_nothing_else():
    for hidden, act in itertools.product((32, 64, 96, 128), ACTS):
        assert L.policy_supported(12, hidden, 2, act) and L.actor_supported(12, hidden, 2, act)
    for act in ACTS:
        assert L.actor_supported(12, 256, 2, act) and not L.policy_supported(12, 256, 2, act)
    for hidden in (160, 192, 512, 0, 255, 257):
        assert not L.actor_supported(12, hidden, 2, 'relu') and not L.policy_supported(12, hidden, 2, 'relu')
    # the same observation / action / activation limits as the narrow widths
    for obs, nu, act in ((0, 1, 'relu'), (33, 1, 'relu'), (4, 0, 'relu'), (4, 5, 'relu'), (4, 1, 'gelu')):
        assert not L.actor_supported(obs, 256, nu, act) and not L.actor_supported(obs, 128, nu, act)
    for obs, nu in ((1, 1), (32, 4), (24, 4), (4, 1)):
        assert L.actor_supported(obs, 256, nu, 'tanh')


def test_256_is_served_for_three_element_tuples_only():
    assert L.is_wide((256, 'relu', 'sac')) and L.is_wide((256, 'tanh', 'ddpg'))
    assert not L.is_wide((256, 'relu')) and not L.is_wide((128, 'relu', 'sac')) and not L.is_wide(None)
    assert L.policy_tuple((256, 'relu', 'sac')) == (256, 'relu', 'sac')
    # the CBF filter behind a 256-wide actor: its own predicate, a kind is required; the narrow predicates are as they were
    assert _cbf.supported_wide_actor('cartpole', 4, 256, 1, 'relu', 'sac') and _cbf.supported_wide_actor('cartpole', 8, 256, 1, 'tanh', 'ddpg')
    assert not _cbf.supported_wide_actor('cartpole', 4, 128, 1, 'relu', 'sac') and not _cbf.supported_wide_actor('cartpole', 4, 256, 1, 'relu', None)
    assert not _cbf.supported_wide_actor('quadrotor', 12, 256, 2, 'relu', 'sac')
    assert not _cbf.supported_actor('cartpole', 4, 256, 1, 'relu', 'sac') and not _cbf.supported('cartpole', 4, 256, 1, 'relu')
    assert _cbf.is_wide(256, 'sac') and not _cbf.is_wide(256, None) and not _cbf.is_wide(128, 'sac')


def test_wide_library_names_collide_with_no_pol_variant(monkeypatch):
    monkeypatch.delenv('SCG_SPEC_TAG', raising=False)
    h = 0x0123456789ABCDEF
    narrow = {L.spec_paths(h, p)[1] for p in [None] + [(w, a) for w in (32, 64, 96, 128, 256) for a in ACTS]
              + [(w, a, k) for w in (32, 64, 96, 128) for a in ACTS for k in ('sac', 'ddpg')]}
    wide = [L.spec_paths(h, (256, a, k))[1] for a in ACTS for k in ('sac', 'ddpg')]
    assert len(set(wide)) == 6 and not narrow & set(wide)
    assert all('_pol' not in w.rsplit('/', 1)[-1] and '_wide256_' in w for w in wide)
    assert all(L.spec_paths(h, (256, 'relu', 'sac'))[0] == L.spec_paths(h, p)[0] for p in (None, (64, 'relu')))     # one spec header
    # the source hash covers the new files and differs from the narrow variants'
    assert len({L.source_hash(), L.actor_source_hash(), L.wide_source_hash()}) == 3
    assert L._policy_hash((256, 'relu', 'sac')) == L.wide_source_hash() and L._policy_hash((128, 'relu', 'sac')) == L.actor_source_hash()
    assert L._policy_hash((256, 'relu')) == L.source_hash()
    assert _cbf.source_hash(wide=True) != _cbf.source_hash()


def _cpu_agent(kind, obs_dim=5, nu=2, act='relu', hidden=256):
    from safe_control_gym_amd import ddpg
    from safe_control_gym_amd.sac import SACAgent, SACConfig
    lo, hi = torch.tensor([-1.0, 0.25][:nu]), torch.tensor([2.0, 0.5][:nu])
    torch.manual_seed(3)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        if kind == 'sac':
            return SACAgent(obs_dim, nu, lo, hi, SACConfig(hidden_dim=hidden, activation=act), 'cpu')
        return ddpg.DDPGAgent(obs_dim, nu, lo.numpy(), hi.numpy(), ddpg.DDPGConfig(hidden_dim=hidden, activation=act), 'cpu')


def _expected(kind, ag):
    a = ag.ac.actor
    f = a.net.fcs
    if kind == 'sac':
        w3, b3 = torch.cat([a.mu_layer.weight, a.log_std_layer.weight]), torch.cat([a.mu_layer.bias, a.log_std_layer.bias])
    else:
        w3, b3 = f[2].weight, f[2].bias
    return {'W1': f[0].weight, 'b1': f[0].bias, 'W2': f[1].weight, 'b2': f[1].bias, 'W3': w3, 'b3': b3}


@pytest.mark.parametrize('kind', ['sac', 'ddpg'])
def test_packed_actor_vector(kind):
    obs_dim, nu, H = 5, 2, 256
    ag = _cpu_agent(kind, obs_dim, nu)
    assert not ag.use_fused
    pk = ag.packed_actor()
    rows3 = 2 * nu if kind == 'sac' else nu
    sizes = {'W1': H * obs_dim, 'b1': H, 'W2': H * H, 'b2': H, 'W3': rows3 * H, 'b3': rows3}
    off = 0
    for name in ('W1', 'b1', 'W2', 'b2', 'W3', 'b3'):
        assert pk['offsets'][name] == off, name
        off += sizes[name]
    assert pk['p'].numel() == off and pk['p'].dtype == torch.float32
    for name, t in _expected(kind, ag).items():
        o = pk['offsets'][name]
        assert torch.equal(pk['p'][o:o + t.numel()], t.detach().reshape(-1)), name
    if kind == 'sac':                       # the mean's rows come first in the stacked head
        o = pk['offsets']['W3']
        assert torch.equal(pk['p'][o:o + nu * H].view(nu, H), ag.ac.actor.mu_layer.weight.detach())
        assert torch.equal(pk['p'][pk['offsets']['b3']:pk['offsets']['b3'] + nu], ag.ac.actor.mu_layer.bias.detach())
    assert list(pk['low'])[:nu] == [-1.0, 0.25] and list(pk['high'])[:nu] == [2.0, 0.5] and list(pk['low'])[nu:] == [0.0] * (4 - nu)
    # a stable pointer; the contents follow an in-place parameter change
    ptr = pk['p'].data_ptr()
    with torch.no_grad():
        for p in ag.ac.actor.parameters():
            p.mul_(-1.5).add_(0.125)
    pk2 = ag.packed_actor()
    assert pk2 is pk and pk2['p'].data_ptr() == ptr
    for name, t in _expected(kind, ag).items():
        o = pk['offsets'][name]
        assert torch.equal(pk['p'][o:o + t.numel()], t.detach().reshape(-1)), name
    # the struct of a non-fused agent points at it
    s = ag.actor_struct()
    assert s.d_params == ptr and (s.hidden, s.activation, s.kind) == (H, L.POLICY_ACTS['relu'], L.ACTOR_KINDS[kind])
    assert [getattr(s, n) for n in ('W1', 'b1', 'W2', 'b2', 'W3', 'b3')] == [pk['offsets'][n] for n in ('W1', 'b1', 'W2', 'b2', 'W3', 'b3')]
    assert list(s.act_low)[:nu] == [-1.0, 0.25] and list(s.act_high)[:nu] == [2.0, 0.5]


def test_the_key_is_an_extension_key():
    assert 'wide_actor' not in controllers.SAC_DEFAULTS and 'wide_actor' not in controllers.DDPG_DEFAULTS
    assert 'fused_rollout' not in controllers.SAC_DEFAULTS and 'fused_rollout' not in controllers.DDPG_DEFAULTS
    assert controllers.SAC_DEFAULTS['hidden_dim'] == controllers.DDPG_DEFAULTS['hidden_dim'] == 256


SPEC = SimpleNamespace(obs_dim=12, nx=6, nu=2)              # Quadrotor 2D tracking: one observation row of state + goal
SPEC_ROWS = SimpleNamespace(obs_dim=18, nx=6, nu=2)         # obs_goal_horizon = 2: two goal rows behind the state


@pytest.mark.parametrize('kind', ['sac', 'ddpg'])
def test_the_served_or_not_decision(kind):
    f = controllers.offpolicy_fused_shape

    def cfg(hidden, **over):
        return dict(hidden_dim=hidden, activation='relu', norm_obs=False, norm_reward=False, **over)
    for hidden in (128, 256):
        # without fused_rollout: nothing asked, nothing said; wide_actor alone is an error
        assert f(SPEC, cfg(hidden), kind) == (None, None)
        with pytest.raises(ValueError, match='wide_actor'):
            f(SPEC, cfg(hidden, wide_actor=True), kind)
        # running normalisers and multi-row observations warn, with or without wide_actor
        for keys in (dict(fused_rollout=True), dict(fused_rollout=True, wide_actor=True)):
            for norm in (dict(norm_obs=True), dict(norm_reward=True)):
                shape, warning = f(SPEC, dict(cfg(hidden, **keys), **norm), kind)
                assert shape is None and 'fused_rollout=True is not served' in warning
            shape, warning = f(SPEC_ROWS, cfg(hidden, **keys), kind)
            assert shape is None and 'fused_rollout=True is not served' in warning
    # 128: served with fused_rollout, with or without wide_actor, and only on the agent's fused path
    assert f(SPEC, cfg(128, fused_rollout=True), kind) == ((128, 'relu', kind), None)
    assert f(SPEC, cfg(128, fused_rollout=True, wide_actor=True), kind) == ((128, 'relu', kind), None)
    for off in (dict(fused_update=False), dict(cuda_graphs=False)):
        for keys in (dict(fused_rollout=True), dict(fused_rollout=True, wide_actor=True)):
            shape, warning = f(SPEC, cfg(128, **keys, **off), kind)
            assert shape is None and warning
    # 256: today's warning without the key, served with it, and the agent's fused update is not required
    shape, warning = f(SPEC, cfg(256, fused_rollout=True), kind)
    assert shape is None and warning == (f'{kind}: fused_rollout=True is not served for hidden_dim 256 / relu / obs {SPEC.obs_dim} (widths 32, 64, '
                                         f'96, 128 on the fused agent, no running normaliser): keeping the eager evaluation loop')
    assert f(SPEC, cfg(256, fused_rollout=True, wide_actor=True), kind) == ((256, 'relu', kind), None)
    assert f(SPEC, cfg(256, fused_rollout=True, wide_actor=True, fused_update=False, cuda_graphs=False), kind) == ((256, 'relu', kind), None)
    # other widths above 128 stay unserved
    for hidden in (160, 192, 512):
        shape, warning = f(SPEC, cfg(hidden, fused_rollout=True, wide_actor=True), kind)
        assert shape is None and warning

"""The fused Safe-Explorer PPO collector's host side without a GPU: library naming and hash, the stale-library sweep, the LDS placement
calculator, supported() edges, the packed safety-layer layout against a PyTorch SafetyLayer, and the controller / collector plumbing with
its fallback warning."""
import os
import warnings

import numpy as np
import pytest

torch = pytest.importorskip('torch')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_name_prefix_and_source_hash():
    from safe_control_gym_amd import _adversarial, _safe_explorer
    p = _safe_explorer.lib_path(0x1234, 128, 'tanh', 150)
    assert os.path.basename(p) == 'libscg_saferoll_0000000000001234_128_tanh_150.so'
    assert _safe_explorer.PREFIX == 'libscg_saferoll_'
    h = _safe_explorer.source_hash()
    assert isinstance(h, int) and 0 <= h < 2 ** 64 and h == _safe_explorer.source_hash()
    assert h != _adversarial.source_hash()
    names = [os.path.basename(d) for d in _safe_explorer.DEPS]
    assert {'scg_safe_explorer.hip', 'scg_safe_explorer.h', 'scg_adversarial.h', 'scg_kernels.hip'} <= set(names)


def test_stale_sweep_knows_the_prefix():
    import __graft_entry__ as G
    from safe_control_gym_amd import _lib, _safe_explorer
    base = os.path.basename(_safe_explorer.lib_path(0xabc, 32, 'tanh', 16))
    assert G.expected_source_hash(base) == _safe_explorer.source_hash() != _lib.source_hash()


# (obs, A, C, H, Hc) -> where the launcher puts the safety layer (the issue's table of shipped shapes)
TABLE = [((4, 1, 8, 32, 100), 'lds'), ((6, 2, 12, 128, 150), 'lds'), ((12, 2, 12, 128, 150), 'global'),
         ((24, 4, 24, 128, 150), 'global'), ((12, 2, 12, 64, 10), 'lds'), ((12, 2, 12, 32, 16), 'lds')]


@pytest.mark.parametrize('shape,where', TABLE)
def test_placement_calculator_verdicts(shape, where):
    from safe_control_gym_amd import _adversarial, _safe_explorer
    obs, A, C, H, hc = shape
    assert _safe_explorer.placement(obs, H, A, C, hc) == where
    b, w, il = _safe_explorer.lds_bytes(obs, H, A, C, hc, 4)
    assert w == 4 and il == (where == 'lds') and b <= 163840
    img = 4 * _adversarial._image_words(obs, H, A)
    safe = 4 * _safe_explorer.packed_words(obs, A, C, hc)
    assert (img + safe <= 163840) or where == 'global'
    # forcing LDS on a shape whose layer does not fit there: no waves
    b, w, il = _safe_explorer.lds_bytes(obs, H, A, C, hc, 4, placement='lds')
    assert il and (w == 0) == (where == 'global')
    # forcing memory always fits (the actor image alone is at most ~80 KiB)
    assert _safe_explorer.lds_bytes(obs, H, A, C, hc, 4, placement='global')[1:] == (4, False)
    # hidden 128 runs 4 waves per workgroup whatever is asked for
    assert _safe_explorer.lds_bytes(obs, H, A, C, hc, 8)[1] == (4 if H == 128 else 8 if b <= 163840 else 4) or H < 128


def test_supported_edges():
    from safe_control_gym_amd._safe_explorer import supported
    assert supported(12, 128, 2, 'tanh', 12, 150)
    assert supported(12, 128, 2, 'tanh', 12, [150])                 # a one-element list is one hidden layer
    assert not supported(12, 128, 2, 'tanh', 12, [64, 64])          # more than one hidden layer
    assert not supported(12, 48, 2, 'tanh', 12, 16)                 # no actor tile of 48
    assert not supported(12, 64, 2, 'gelu', 12, 16)
    assert not supported(33, 64, 2, 'tanh', 12, 16)                 # obs <= 32
    assert not supported(12, 64, 5, 'tanh', 12, 16)                 # A <= 4
    assert not supported(12, 64, 2, 'tanh', 33, 16) and not supported(12, 64, 2, 'tanh', 0, 16)
    assert supported(12, 64, 2, 'tanh', 32, 16) and supported(12, 64, 2, 'tanh', 12, 256)
    assert not supported(12, 64, 2, 'tanh', 12, 257) and not supported(12, 64, 2, 'tanh', 12, 0)


@pytest.mark.parametrize('obs,A,C,hc', [(12, 2, 12, 150), (4, 1, 8, 100), (24, 4, 3, 32), (7, 3, 2, 5)])
def test_packing_layout_against_a_safety_layer(obs, A, C, hc):
    """Unpacking the packed buffer by the header's layout gives back every weight; every padded entry is zero; and g computed from
    the packed buffer the way the kernel reads it equals SafetyLayer.g."""
    from safe_control_gym_amd import _safe_explorer
    from safe_control_gym_amd.safe_explorer import SafetyLayer
    torch.manual_seed(0)
    layer = SafetyLayer(obs, A, C, hc)
    buf = _safe_explorer.pack_safety_layer(layer.constraint_models, obs, A, hc)
    hp, nt, q, stride = _safe_explorer.packed_dims(obs, A, hc)
    assert buf.dtype == torch.float32 and buf.numel() == C * stride == _safe_explorer.packed_words(obs, A, C, hc)
    assert hp % 32 == 0 and hp >= hc and stride % 4 == 0
    blk = buf.view(C, stride)
    x = torch.randn(9, obs)
    for i, m in enumerate(layer.constraint_models):
        W1, b1, W2, b2 = (t.detach() for t in (m.fcs[0].weight, m.fcs[0].bias, m.fcs[1].weight, m.fcs[1].bias))
        w1f = blk[i, :nt * q * 64].view(nt, q, 64)
        rec = torch.zeros(hp, 8 * (q // 4))
        for t in range(nt):
            for qq in range(q):
                for lane in range(64):
                    r = (qq & 3) + 8 * (qq >> 2) + 4 * (lane >> 5)
                    rec[32 * t + (lane & 31), r] = w1f[t, qq, lane]
        assert torch.equal(rec[:hc, :obs], W1)
        assert (rec[hc:] == 0).all() and (rec[:, obs:] == 0).all()
        o = nt * q * 64
        assert torch.equal(blk[i, o:o + hc], b1) and (blk[i, o + hc:o + hp] == 0).all()
        o += hp
        w2 = blk[i, o:o + A * hp].view(A, hp)
        assert torch.equal(w2[:, :hc], W2) and (w2[:, hc:] == 0).all()
        o += A * hp
        assert torch.equal(blk[i, o:o + A], b2) and (blk[i, o + A:o + 4] == 0).all()
        # g from the padded operands = the layer's own
        h = torch.relu(x.double() @ rec[:, :obs].double().T + blk[i, nt * q * 64:nt * q * 64 + hp].double())
        g = h @ w2.double().T + b2.double()
        torch.testing.assert_close(g, m(x.double().float()).double(), rtol=1e-5, atol=1e-5)
    out = torch.zeros_like(buf)
    assert _safe_explorer.pack_safety_layer(layer.constraint_models, obs, A, hc, out=out) is out and torch.equal(out, buf)


def test_controller_defaults_still_equal_the_yaml_and_omit_the_key():
    from safe_control_gym_amd.controllers import SAFE_EXPLORER_PPO_DEFAULTS
    from safe_control_gym_amd.registration import get_config
    assert 'fused_rollout' not in SAFE_EXPLORER_PPO_DEFAULTS
    assert get_config('safe_explorer_ppo') == SAFE_EXPLORER_PPO_DEFAULTS


def test_controller_key_plumbing_picks_the_env_shape():
    """_safety_shape: the (policy, safety_layer) the controller builds its envs with — only with fused_rollout, a one-layer safety
    layer, no normaliser and a servable shape."""
    from safe_control_gym_amd.controllers import SafeExplorerPPO
    from safe_control_gym_amd.registration import load_task
    env_id, cfg = load_task('quadrotor_2D_track')

    def shape(**kw):
        c = SafeExplorerPPO.__new__(SafeExplorerPPO)
        c.env_id, c.task_config = env_id, dict(cfg)
        algo = dict(SafeExplorerPPO.DEFAULTS, activation='tanh', hidden_dim=128, constraint_hidden_dim=150)
        algo.update(kw)
        c.algo_config = algo
        for k, v in algo.items():
            setattr(c, k, v)
        return c._safety_shape()
    assert shape() == (None, None)                                    # the key is opt-in
    assert shape(fused_rollout=True) == ((128, 'tanh'), 150)
    assert shape(fused_rollout=True, constraint_hidden_dim=[150]) == ((128, 'tanh'), 150)
    assert shape(fused_rollout=True, constraint_hidden_dim=[64, 64]) == (None, None)
    assert shape(fused_rollout=True, norm_obs=True) == (None, None)
    assert shape(fused_rollout=True, norm_reward=True) == (None, None)
    assert shape(fused_rollout=True, hidden_dim=48) == (None, None)


def _replay_env():
    from replay_env import ReplayVecEnv
    from safe_control_gym_amd.env_config import EnvSpec
    from safe_control_gym_amd.registration import load_task
    env_id, cfg = load_task('quadrotor_2D_track')
    spec = EnvSpec(env_id, cfg)
    n, T = 8, 4
    rng = np.random.default_rng(0)
    z = lambda *s: rng.normal(size=s).astype(np.float32)             # noqa: E731
    env = ReplayVecEnv(spec, 'cpu', z(n, spec.obs_dim), z(T, n, spec.obs_dim), z(T, n), np.zeros((T, n), bool), np.zeros((T, n), bool),
                       z(T, n, spec.obs_dim))
    env.out.state = torch.zeros(spec.nx, n)
    return env


def test_collector_falls_back_with_a_warning_on_an_env_without_the_shape():
    """fused_rollout on an env that carries no safety shape (here a CPU replay env): one warning, the eager collector; without the key:
    no warning."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    from safe_control_gym_amd.ppo import PPOConfig
    from safe_control_gym_amd.safe_explorer import SafeExplorerPPO
    for key in (True, False):
        env = _replay_env()
        cfg = PPOConfig(hidden_dim=32, activation='tanh', rollout_steps=4, opt_epochs=1, mini_batch_size=16, extra={'fused_rollout': key})
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter('always')
            s = SafeExplorerPPO(env, cfg, seed=0, constraint_hidden_dim=16)
        hits = [x for x in w if 'eager collector' in str(x.message)]
        assert len(hits) == (1 if key else 0)
        assert s._fused_safe is None and not hasattr(s, '_f_episode_acc')

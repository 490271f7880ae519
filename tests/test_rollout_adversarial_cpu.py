"""The fused RARL / RAP collector without a GPU: the ctypes structs against include/scg_adversarial.h, library naming, the LDS budget
the launcher applies (scg_adversarial.hip, AdvShape) at its boundary cases, the build's stale-library sweep, the controller defaults,
and the guard on the env / learner source hashes the committed profiles name."""
import ctypes as C
import json
import os
import re

import pytest

from safe_control_gym_amd import _adversarial, _learn, _lib, _sac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_actor_ptrs_struct_matches_header():
    with open(_adversarial.HEADER) as f:
        src = f.read()
    m = re.search(r'typedef struct \{\s*const float \*(.*?);\s*\} scg_actor_ptrs;', src, re.S)
    assert m, 'scg_actor_ptrs not found in include/scg_adversarial.h'
    names = [n.strip().lstrip('*') for n in m.group(1).split(',')]
    assert names == [f[0] for f in _adversarial.ActorPtrs._fields_] == ['W1', 'b1', 'W2', 'b2', 'W3', 'b3', 'logstd']
    assert C.sizeof(_adversarial.ActorPtrs) == 7 * C.sizeof(C.c_void_p)
    # the entry point takes the protagonist and the rollout outputs as the existing scg_policy / scg_policy_rollout structs
    proto = re.search(r'int scg_rollout_adversarial\((.*?)\);', src, re.S).group(1)
    assert 'const scg_policy* protagonist' in proto and 'const scg_policy_rollout* out' in proto
    assert 'const scg_actor_ptrs* adversaries' in proto and 'const int32_t* d_adv_index' in proto


def test_library_naming():
    p = _adversarial.lib_path(0x1234abcd, 64, 'tanh', 2)
    assert os.path.dirname(p) == _lib.SPEC_DIR
    assert os.path.basename(p) == 'libscg_advroll_000000001234abcd_64_tanh_2.so'
    assert os.path.basename(p).startswith(_adversarial.PREFIX)
    assert _adversarial.SRC.endswith('scg_adversarial.hip') and os.path.exists(_adversarial.SRC)
    assert all(os.path.exists(d) for d in _adversarial.DEPS)


# (obs_dim, act_dim, dynamics adversary dim) of the shipped tasks: goal horizon 1 doubles the state row for tracking
Q2T, Q3T, CP = (12, 2, 2), (24, 4, 3), (4, 1, 2)


@pytest.mark.parametrize('task', [Q2T, Q3T, CP])
@pytest.mark.parametrize('n', [1, 2, 3, 4])
def test_lds_budget_at_reference_hidden_64(task, n):
    """rarl.yaml / rap.yaml (hidden_dim 64): every task fits with up to four adversaries; Quadrotor3D tracking with four drops to
    4 waves per workgroup."""
    obs, nu, ad = task
    b8, w8 = _adversarial.lds_bytes(obs, 64, nu, ad, n, 8)
    assert w8 in (4, 8) and b8 <= _adversarial.LDS_BUDGET
    assert _adversarial.supported(obs, 64, nu, ad, 'tanh', n)
    if task == Q3T and n == 4:
        assert _adversarial.lds_bytes(obs, 64, nu, ad, n, 8) == (143952, 4)
    else:
        assert w8 == 8


def test_lds_budget_boundaries():
    # Quadrotor3D tracking, four adversaries: 168 528 B at 8 waves -> 4 waves, 143 952 B
    img = 4 * (_adversarial._image_words(24, 64, 4) + 4 * _adversarial._image_words(24, 64, 3))
    assert img + 8 * 64 * 24 * 4 == 168528
    # hidden 128, one adversary, Quadrotor2D tracking: 163 872 B with the transpose scratch at 4 waves (32 B over); the rows are then
    # stored one by one and the images alone fit
    img = 4 * 2 * _adversarial._image_words(12, 128, 2)
    assert img == 151584 and img + 4 * 64 * 12 * 4 == 163872
    assert _adversarial.lds_bytes(12, 128, 2, 2, 1, 8) == (151584, 4)
    assert _adversarial.lds_bytes(12, 128, 2, 2, 1, 4) == (151584, 4)
    assert _adversarial.supported(12, 128, 2, 2, 'tanh', 1)
    # hidden 96: one adversary on every task, two on Quadrotor2D tracking and CartPole with the transpose scratch; two on Quadrotor3D
    # tracking only with the rows stored one by one (169 008 B with the scratch at 4 waves, 144 432 B without)
    for obs, nu, ad in (Q2T, Q3T, CP):
        assert _adversarial.supported(obs, 96, nu, ad, 'tanh', 1)
    assert _adversarial.lds_bytes(12, 96, 2, 2, 2, 8)[0] == 4 * (_adversarial._image_words(12, 96, 2) * 3) + 8 * 64 * 12 * 4
    assert _adversarial.supported(4, 96, 1, 2, 'relu', 2)
    img = 4 * (_adversarial._image_words(24, 96, 4) + 2 * _adversarial._image_words(24, 96, 3))
    assert img == 144432 and img + 4 * 64 * 24 * 4 == 169008
    assert _adversarial.lds_bytes(24, 96, 4, 3, 2, 8) == (144432, 8)
    # over budget: the fallback shape of the GPU test
    assert not _adversarial.supported(24, 128, 4, 3, 'relu', 3)
    assert _adversarial.lds_bytes(24, 128, 4, 3, 3, 8)[1] == 0
    # bounds: population size, adversary width, policy bounds
    assert not _adversarial.supported(12, 64, 2, 2, 'tanh', 5)
    assert not _adversarial.supported(12, 64, 2, 2, 'tanh', 0)
    assert not _adversarial.supported(12, 64, 2, 5, 'tanh', 1)
    assert not _adversarial.supported(12, 48, 2, 2, 'tanh', 1)
    assert not _adversarial.supported(12, 64, 2, 2, 'gelu', 1)


def test_build_sweep_keeps_fresh_adversarial_libraries():
    import __graft_entry__ as g
    h = _adversarial.source_hash()
    assert g.expected_source_hash(os.path.basename(_adversarial.lib_path(0xabc, 64, 'tanh', 1))) == h
    assert h != _lib.source_hash()
    assert g.expected_source_hash('libscg_spec_0000000000000abc_pol64_tanh.so') == _lib.source_hash()


def test_controller_defaults_free_of_the_extension_key():
    from safe_control_gym_amd.controllers import RAP_DEFAULTS, RARL_DEFAULTS
    assert 'fused_rollout' not in RARL_DEFAULTS and 'fused_rollout' not in RAP_DEFAULTS


def test_committed_profiles_of_other_sources_are_dropped_not_quoted():
    """The r06 profiles name the kernel sources they were measured on, and bench.py quotes them only while the tree's hash matches.
    The env hash is a hash of text: scg_env_kernels.h now reaches rollout_policy_kernel's shared pieces through scg_rollout_common.h,
    so it differs from the profiles' although the step kernels' assembly is the same, and bench.py drops the env entries instead of
    quoting them.  The SAC library has changed since its profile entry was measured (its ring push writes every action column), and so
    has the PPO learner library (its advantage moments are float64: scg_ppo_returns_moments / _normalise), so bench.py drops both
    entries instead of quoting measurements of other sources."""
    import bench
    with open(os.path.join(ROOT, 'profiles', 'r06_learner_kernel_sums.json')) as f:
        want = json.load(f)['_meta']['source_hashes']
    assert want == {'env': '0xb151b347b3bf3a71', 'learn': '0x473679a837dcce88', 'sac': '0x693001d1e2321112'}
    assert f'0x{_lib.source_hash():016x}' != want['env']
    assert f'0x{_learn.source_hash():016x}' != want['learn']
    e, src = bench.learner_kernel_sum('ppo/65536/48x16256')
    assert e is None and 'dropped' in src
    assert f'0x{_sac.source_hash():016x}' != want['sac']
    e, src = bench.learner_kernel_sum('sac/4096/16')
    assert e is None and 'dropped' in src
    for name in ('r06_chain_latency.json', 'r06_hbm_traffic.json'):
        with open(os.path.join(ROOT, 'profiles', name)) as f:
            assert json.load(f)['_meta']['source_hash'] == want['env']
    e, src = bench.pmc_entry('quadrotor_2D_track/f32/65536')
    assert e is None and 'dropped' in src
    assert 'dropped' in bench.chain_latency_of('quadrotor_2D_track', 20.0)

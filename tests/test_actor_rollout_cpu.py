"""The fused SAC / DDPG actor rollout without a GPU: library naming for two- and three-element policy tuples, the scg_actor ctypes
struct against include/scg_actor_rollout.h, tuple validation before any build, and the source hashes of the old and the new libraries."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_spec_paths_naming(monkeypatch):
    from safe_control_gym_amd import _lib as L
    monkeypatch.delenv('SCG_SPEC_TAG', raising=False)
    h = 0x0123456789ABCDEF
    hdr2, so2 = L.spec_paths(h, (64, 'tanh'))
    # the two-element name is today's, byte for byte
    assert so2 == os.path.join(L.SPEC_DIR, 'libscg_spec_0123456789abcdef_pol64_tanh.so')
    assert hdr2 == os.path.join(L.SPEC_DIR, 'scg_spec_0123456789abcdef.h')
    assert L.spec_paths(h)[1] == os.path.join(L.SPEC_DIR, 'libscg_spec_0123456789abcdef.so')
    for kind in ('sac', 'ddpg'):
        hdr3, so3 = L.spec_paths(h, (128, 'relu', kind))
        assert so3 == os.path.join(L.SPEC_DIR, f'libscg_spec_0123456789abcdef_pol128_relu_{kind}.so') and hdr3 == hdr2
    monkeypatch.setenv('SCG_SPEC_TAG', 'dev')
    assert L.spec_paths(h, (32, 'leaky_relu', 'sac'))[1].endswith('libscg_spec_0123456789abcdef_pol32_leaky_relu_sac_dev.so')
    assert L.ACTOR_KINDS == {'sac': 1, 'ddpg': 2}


def test_cbf_library_naming():
    from safe_control_gym_amd import _cbf
    from safe_control_gym_amd import _lib as L
    assert _cbf.lib_path(0xAB, 64, 'tanh') == os.path.join(L.SPEC_DIR, 'libscg_cbfroll_00000000000000ab_64_tanh.so')
    assert _cbf.lib_path(0xAB, 64, 'tanh', 'sac') == os.path.join(L.SPEC_DIR, 'libscg_cbfroll_00000000000000ab_64_tanh_sac.so')
    assert _cbf.supported_actor('cartpole', 4, 64, 1, 'relu', 'sac') and not _cbf.supported_actor('quadrotor', 6, 64, 2, 'relu', 'sac')
    assert not _cbf.supported_actor('cartpole', 4, 256, 1, 'relu', 'sac') and not _cbf.supported_actor('cartpole', 4, 64, 1, 'relu', 'ppo')


@pytest.mark.parametrize('bad', [(64,), (64, 'tanh', 'sac', 1), (64, 'tanh', 'ppo'), (64, 'gelu', 'sac'), (0, 'tanh', 'ddpg'), (64.5, 'relu', 'sac'),
                                 'sac'])
def test_tuple_validation_raises_before_any_build(bad, monkeypatch):
    from safe_control_gym_amd import _lib as L

    def no_build(*a, **k):
        raise AssertionError('a compiler or the library was reached')
    monkeypatch.setattr(L.subprocess, 'run', no_build)
    monkeypatch.setattr(L, 'spec_source', no_build)
    with pytest.raises(ValueError):
        L.policy_tuple(bad)
    if isinstance(bad, tuple) and len(bad) != 2:
        with pytest.raises(ValueError):
            L.spec_paths(1, bad)
        with pytest.raises(ValueError):
            L.build_spec(L.Config(), policy=bad)
        with pytest.raises(ValueError):
            L.lib_for(L.Config(), policy=bad)
    assert L.policy_tuple((64, 'tanh')) == (64, 'tanh') and L.policy_tuple([96, 'relu', 'ddpg']) == (96, 'relu', 'ddpg')
    assert L.policy_tuple(None) is None


def _struct_fields(hdr, name):
    """[(c type, field name, array length or None)] of `typedef struct { ... } name;`."""
    body = re.search(r'typedef struct\s*\{([^}]*)\}\s*' + name + r'\s*;', hdr, re.S).group(1)
    out = []
    for decl in body.split(';'):
        decl = decl.strip()
        if not decl:
            continue
        ctype, names = re.match(r'((?:const\s+)?\w+\s*\*?)\s*(.*)', decl, re.S).groups()
        for n in names.split(','):
            m = re.match(r'\s*(\w+)\s*(?:\[(\d+)\])?\s*$', n)
            out.append((ctype.replace(' ', ''), m.group(1), int(m.group(2)) if m.group(2) else None))
    return out


def test_actor_struct_layout_matches_the_header():
    from safe_control_gym_amd import _lib as L
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'scg_actor_rollout.h')).read(), flags=re.S)
    fields = _struct_fields(hdr, 'scg_actor')
    assert [f[1] for f in fields] == [f[0] for f in L.Actor._fields_]
    size_align = {'constfloat*': (8, 8), 'int32_t': (4, 4), 'float': (4, 4)}
    off, worst = 0, 1
    for ctype, name, count in fields:
        size, align = size_align[ctype]
        off = (off + align - 1) // align * align
        assert getattr(L.Actor, name).offset == off, name
        assert getattr(L.Actor, name).size == size * (count or 1), name
        off += size * (count or 1)
        worst = max(worst, align)
    assert C.sizeof(L.Actor) == (off + worst - 1) // worst * worst == 8 + 9 * 4 + 4 + 2 * 16
    assert re.search(r'enum\s*\{\s*SCG_ACTOR_SAC\s*=\s*1\s*,\s*SCG_ACTOR_DDPG\s*=\s*2\s*\}', hdr)
    names = set(re.findall(r'\b(scg_[a-z_0-9]+)\s*\(', hdr))
    assert names == {'scg_rollout_actor', 'scg_actor_rollout_shape'} == set(L.ACTOR_EXPORTS)
    cbf = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'scg_cbf.h')).read(), flags=re.S)
    assert 'scg_rollout_cbf_actor' in set(re.findall(r'\b(scg_[a-z_0-9]+)\s*\(', cbf))


def test_simulator_sources_are_untouched_and_the_variant_has_its_own_hash():
    """The actor rollout lives in new files: the simulator's libraries keep their source hash (and do not carry the entry points); the
    kind variants are stamped with a hash that covers the new files too."""
    from safe_control_gym_amd import _cbf
    from safe_control_gym_amd import _lib as L
    assert 'scg_actor_rollout.h' not in L.HEADERS and L.SOURCES == ['scg_kernels.hip']
    assert not set(L.ACTOR_EXPORTS) & set(L.EXPORTS)
    assert L.actor_source_hash() != L.source_hash()
    assert L._policy_hash((64, 'tanh')) == L.source_hash() and L._policy_hash((64, 'tanh', 'sac')) == L.actor_source_hash()
    for d in L.ACTOR_DEPS:
        assert os.path.exists(os.path.normpath(os.path.join(L.CSRC_DIR, d))), d
    deps = {os.path.basename(d) for d in _cbf.DEPS}
    assert {'scg_cbf_actor.h', 'scg_actor_rollout.h'} <= deps
    src = open(os.path.join(L.CSRC_DIR, L.ACTOR_SOURCE)).read()
    assert '#include "scg_kernels.hip"' in src and '#include "scg_actor_rollout.h"' in src

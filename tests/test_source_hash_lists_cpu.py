"""Every file a library's translation unit includes is in that library's staleness hash: a library built from older text of any of
them is rebuilt, never loaded.  The lists are kept by hand (_lib.HEADERS / ACTOR_DEPS / WIDE_DEPS, _cbf.DEPS / WIDE_DEPS,
_adversarial.DEPS, _safe_explorer.DEPS, _sac.DEPS, _ddpg.DEPS); this walks the #include "..." lines of each source file transitively within csrc/ and include/
and holds the list to what it finds."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from safe_control_gym_amd import _adversarial, _cbf, _ddpg, _sac, _safe_explorer  # noqa: E402
from safe_control_gym_amd import _lib as L  # noqa: E402

TREES = tuple(os.path.join(ROOT, d) + os.sep for d in (os.path.join('safe_control_gym_amd', 'csrc'), 'include'))


def reached(source):
    """The files `source` reaches through #include "..." lines (whatever the preprocessor conditions around them), itself included."""
    seen, todo = set(), [os.path.normpath(source)]
    while todo:
        path = todo.pop()
        if path in seen:
            continue
        seen.add(path)
        with open(path) as f:
            for name in re.findall(r'^\s*#\s*include\s+"([^"]+)"', f.read(), re.M):
                nxt = os.path.normpath(os.path.join(os.path.dirname(path), name))
                assert nxt.startswith(TREES) and os.path.exists(nxt), f'{path} includes {name}: not a file of csrc/ or include/'
                todo.append(nxt)
    return seen


def lib_list(names):
    return {os.path.normpath(os.path.join(L.CSRC_DIR, n)) for n in names}


ENV = L.SOURCES + L.HEADERS
CASES = {
    '_lib.source_hash': (os.path.join(L.CSRC_DIR, L.SOURCES[0]), lib_list(ENV)),
    '_lib.actor_source_hash': (os.path.join(L.CSRC_DIR, L.ACTOR_SOURCE), lib_list(ENV + L.ACTOR_DEPS)),
    '_lib.wide_source_hash': (os.path.join(L.CSRC_DIR, L.WIDE_SOURCE), lib_list(ENV + L.WIDE_DEPS)),
    '_cbf.source_hash()': (_cbf.SRC, {os.path.normpath(p) for p in _cbf.DEPS}),
    '_cbf.source_hash(wide)': (_cbf.WIDE_SRC, {os.path.normpath(p) for p in _cbf.WIDE_DEPS}),
    '_adversarial.source_hash': (_adversarial.SRC, {os.path.normpath(p) for p in _adversarial.DEPS}),
    '_safe_explorer.source_hash': (_safe_explorer.SRC, {os.path.normpath(p) for p in _safe_explorer.DEPS}),
    '_sac.source_hash': (_sac.SRC, {os.path.normpath(p) for p in _sac.DEPS}),
    '_ddpg.source_hash': (_ddpg.SRC, {os.path.normpath(p) for p in _ddpg.DEPS}),
}
OFFPOLICY = ('_sac.source_hash', '_ddpg.source_hash')


@pytest.mark.parametrize('name', sorted(CASES))
def test_every_included_file_is_hashed(name):
    source, hashed = CASES[name]
    missing = sorted(os.path.relpath(p, ROOT) for p in reached(source) - hashed)
    assert not missing, f'{name} does not cover {missing}'


def test_the_walk_sees_the_shared_rollout_headers():
    """The guard guards: the two shared headers are reached from the libraries that use them, so dropping one from a list fails above."""
    common = os.path.join(L.CSRC_DIR, 'scg_rollout_common.h')
    core = os.path.join(L.CSRC_DIR, 'scg_cbf_core.h')
    for name, (source, _) in CASES.items():
        if name not in OFFPOLICY:                   # (the learners' libraries hold no rollout)
            assert common in reached(source), name
    for name in OFFPOLICY:                          # and theirs: the wide-tile passes and the step both learners share
        for header in ('scg_wide.h', 'scg_offpolicy_step.h'):
            assert os.path.join(L.CSRC_DIR, header) in reached(CASES[name][0]), name
    assert core in reached(_cbf.SRC) and core in reached(_cbf.WIDE_SRC)
    source, hashed = CASES['_cbf.source_hash(wide)']
    assert reached(source) - (hashed - {core}) == {core}

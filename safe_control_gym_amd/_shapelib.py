"""What the builders of the per-network-shape libraries (_learn, _sac, _ddpg) have in common: the source digest that stamps a
library, the "current? else hipcc" build, and the load that refuses a stale or mis-shaped library — and what the two off-policy
libraries (_sac, _ddpg) share beyond that: the replay-ring struct and the shapes they serve.  Each module keeps its sources (SRC,
DEPS), its argument structs and bindings, and its public names."""
import ctypes as C
import hashlib
import os
import subprocess

from safe_control_gym_amd import _lib as L


class Ring(C.Structure):
    """scg_sac_ring / scg_ddpg_ring (include/scg_sac.h, scg_ddpg.h: the same fields): the replay ring a collector's push writes."""
    _fields_ = [('d_obs', C.c_void_p), ('d_act', C.c_void_p), ('d_rew', C.c_void_p), ('d_next_obs', C.c_void_p), ('d_mask', C.c_void_p),
                ('capacity', C.c_int32), ('d_pos', C.c_void_p), ('d_size_f', C.c_void_p), ('d_size_i32', C.c_void_p), ('d_counter', C.c_void_p)]


def supported(obs_dim, hidden, act_dim, activation):
    """The network shapes the off-policy libraries (_sac, _ddpg: the wide-tile passes of csrc/scg_wide.h) serve."""
    from safe_control_gym_amd._learn import ACTS
    return (1 <= act_dim <= 4 and obs_dim >= 1 and obs_dim + act_dim < 32 and hidden % 32 == 0 and 32 <= hidden <= 128
            and activation in ACTS)


def source_hash(deps):
    """64-bit digest over (basename, bytes) of the files in `deps`: compiled into the library (-DSCG_SRC_HASH) and compared at load
    time, so that a library of older sources is rebuilt, never used."""
    h = hashlib.sha256()
    for p in deps:
        with open(p, 'rb') as f:
            h.update(os.path.basename(p).encode() + b'\0' + f.read())
    return int.from_bytes(h.digest()[:8], 'little')


def current(so, deps):
    return os.path.exists(so) and L._lib_source_hash(so) == source_hash(deps)


def build(so, src, deps, defines, what, flags_env=None, force=False):
    """`so` from `src` for gfx950 unless it is there and current.  defines: {macro: value}; flags_env: the environment variable whose
    words are appended to the hipcc line (development builds); what: the library's name in the error message."""
    if not force and current(so, deps):
        return so
    os.makedirs(L.SPEC_DIR, exist_ok=True)
    cmd = [L._hipcc(), '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-shared'] + [f'-D{k}={v}' for k, v in defines.items()] \
        + [f'-DSCG_SRC_HASH=0x{source_hash(deps):016x}ULL', '-o', so, src] + (os.environ.get(flags_env, '').split() if flags_env else [])
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise L.ScgError(f'hipcc failed ({what} build):\n' + res.stdout + res.stderr)
    return so


def load(cache, key, so, deps, rebuild, bind, shape_fn, shape):
    """cache[key], or `so` loaded into it: rebuilt first (rebuild()) when missing or stale, bound (bind(D)), and checked to be the
    library of `shape` (the four ints its `shape_fn` export reports)."""
    if key in cache:
        return cache[key]
    if not current(so, deps):
        if not os.path.exists(L._hipcc()):
            raise L.ScgError(f'{so} is missing or stale and hipcc is not available to build it')
        rebuild()
    D = C.CDLL(so)
    bind(D)
    got = [C.c_int32() for _ in range(4)]
    getattr(D, shape_fn)(*[C.byref(v) for v in got])
    if tuple(v.value for v in got) != tuple(shape):
        raise L.ScgError(f'{so} was built for another network shape')
    cache[key] = D
    return D

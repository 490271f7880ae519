"""ctypes binding + builder of libscg_advroll_<spechash>_<hidden>_<activation>_<n>.so (include/scg_adversarial.h): the RARL / RAP
collector — protagonist, adversary (or a population of up to four) and the env step in one launch — compiled per task config,
actor shape and population size from csrc/scg_adversarial.hip.  The library carries every scg_hip.h entry point as well
(_lib.EXPORTS, scg_rollout_policy included): HipVecEnv(..., policy=(hidden, activation), adversaries=n) drives its handle with it.
No fallback lives here: rarl.py keeps the PyTorch collector, with a warning, for shapes this library does not serve."""
import ctypes as C
import os
import subprocess

from safe_control_gym_amd import _lib as L

SRC = os.path.join(L.CSRC_DIR, 'scg_adversarial.hip')
HEADER = os.path.normpath(os.path.join(L.CSRC_DIR, '..', '..', 'include', 'scg_adversarial.h'))
# the env library's hash inputs (_lib.SOURCES + _lib.HEADERS) and the two new files
DEPS = [os.path.join(L.CSRC_DIR, s) for s in L.SOURCES + L.HEADERS] + [SRC, HEADER]
PREFIX = 'libscg_advroll_'
MAX_ADVERSARIES = 4
LDS_BUDGET = 163840                 # 160 KiB of LDS per CU (MI355X)


class ActorPtrs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ('W1', 'b1', 'W2', 'b2', 'W3', 'b3', 'logstd')]


def actor_ptrs(actor):
    """ActorPtrs of a ppo.MLPActor (per-tensor pointers: the storage is updated in place, so they stay valid across graph replays)."""
    f = actor.pi_net.fcs
    return ActorPtrs(*[t.data_ptr() for t in (f[0].weight, f[0].bias, f[1].weight, f[1].bias, f[2].weight, f[2].bias, actor.logstd)])


def _image_words(nin, hidden, nout):
    """Words of one MlpLds<nin, hidden, nout, 16> image (csrc/scg_mlp.h)."""
    nt, l1q = hidden // 32, 4 * ((nin + 7) // 8)
    end = nt * l1q * 64 + nt * nt * 64 * 16 + nout * hidden + 2 * hidden + nout
    return (end + 3) // 4 * 4


def lds_bytes(obs_dim, hidden, act_dim, adv_dim, n, wpw):
    """(bytes, waves per workgroup) the launcher uses when asked for `wpw` waves (scg_adversarial.hip, AdvShape): the weight images,
    plus the obs transpose scratch for 16-byte rows while it fits at 4 waves; 8 waves drop to 4 when over budget.  wpw 0: no fit."""
    img = 4 * (_image_words(obs_dim, hidden, act_dim) + n * _image_words(obs_dim, hidden, adv_dim))
    per_wave = 64 * obs_dim * 4
    xpose = (obs_dim * 4) % 16 == 0 and img + 4 * per_wave <= LDS_BUDGET
    b = lambda w: img + (w * per_wave if xpose else 0)      # noqa: E731
    for w in ((wpw, 4) if hidden < 128 else (4,)):          # (hidden 128: the 8-wave kernels would spill)
        if b(w) <= LDS_BUDGET:
            return b(w), w
    return b(4), 0


def supported(obs_dim, hidden, act_dim, adv_dim, activation, n, wpw=8):
    return (L.policy_supported(obs_dim, hidden, act_dim, activation) and 1 <= adv_dim <= 4 and 1 <= n <= MAX_ADVERSARIES
            and lds_bytes(obs_dim, hidden, act_dim, adv_dim, n, wpw)[1] > 0)


def source_hash():
    import hashlib
    h = hashlib.sha256()
    for p in DEPS:
        with open(p, 'rb') as f:
            h.update(os.path.basename(p).encode() + b'\0' + f.read())
    return int.from_bytes(h.digest()[:8], 'little')


def lib_path(spec_hash, hidden, activation, n):
    return os.path.join(L.SPEC_DIR, f'{PREFIX}{spec_hash:016x}_{int(hidden)}_{activation}_{int(n)}.so')


def build(cfg, hidden, activation, n, force=False):
    """Compile the collector for this scg_config, actor shape and population size (hipcc, gfx950)."""
    if activation not in L.POLICY_ACTS or not 1 <= int(n) <= MAX_ADVERSARIES:
        raise L.ScgError(f'no fused adversarial rollout for {activation} / {n} adversaries')
    src, h = L.spec_source(cfg)
    hdr, _ = L.spec_paths(h)
    so = lib_path(h, hidden, activation, n)
    if not force and os.path.exists(so) and L._lib_source_hash(so) == source_hash():
        return so
    os.makedirs(L.SPEC_DIR, exist_ok=True)
    with open(hdr, 'w') as f:
        f.write(src)
    cmd = [L._hipcc(), '--offload-arch=gfx950', '-O3', '-ffp-contract=on', '-std=c++17', '-fPIC', '-shared', '-DSCG_SPEC', '-include', hdr,
           f'-DSCG_POLICY_H={int(hidden)}', f'-DSCG_POLICY_ACT={L.POLICY_ACTS[activation]}', f'-DSCG_ADV_N={int(n)}',
           f'-DSCG_SRC_HASH=0x{source_hash():016x}ULL', '-o', so]
    res = None
    for extra in L.sched_flags(cfg):
        res = subprocess.run(cmd + extra + [SRC], capture_output=True, text=True)
        if res.returncode == 0:
            return so
    raise L.ScgError('hipcc failed (adversarial rollout build):\n' + res.stdout + res.stderr)


_libs = {}


def lib_for(cfg, hidden, activation, n):
    """The bound library (every _lib.EXPORTS symbol + scg_rollout_adversarial), built now if missing or stale."""
    _, h = L.spec_source(cfg)
    key = (h, int(hidden), activation, int(n))
    if key in _libs:
        return _libs[key]
    so = lib_path(*key)
    if not os.path.exists(so) or L._lib_source_hash(so) != source_hash():
        if not os.path.exists(L._hipcc()):
            raise L.ScgError(f'{so} is missing or stale and hipcc is not available to build it')
        build(cfg, hidden, activation, n, force=True)
    D = L._bind(so)
    if int(D.scg_spec_hash()) != h:
        raise L.ScgError(f'{so} was built for another config')
    D.scg_rollout_adversarial.argtypes = [C.c_void_p, C.POINTER(L.Policy), C.POINTER(ActorPtrs), C.c_int, C.c_void_p, C.c_int, C.c_int,
                                          C.POINTER(L.PolicyRollout), C.c_void_p, C.c_void_p, C.c_void_p]
    D.scg_adversarial_shape.argtypes = [C.POINTER(C.c_int32)] * 4
    D.scg_adversarial_lds.argtypes = [C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    shape = [C.c_int32() for _ in range(4)]
    D.scg_adversarial_shape(*[C.byref(v) for v in shape])
    if tuple(v.value for v in shape[:3]) != (int(n), int(hidden), L.POLICY_ACTS[activation]):
        raise L.ScgError(f'{so} was built for another adversary population / actor shape')
    _libs[key] = D
    return D

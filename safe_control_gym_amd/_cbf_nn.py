"""ctypes binding + builder of libscg_cbfnn_<spechash>_<hidden>_<activation>.so (include/scg_cbf_nn.h): the CBF-QP safety filter with
a learned correction of the Lie derivative as a batched certify kernel and as the policy rollout with the residual network and the
filter between PPO's actor and the env step, compiled per task config and actor shape from csrc/scg_cbf_nn.hip.  The filter's settings
(CbfParams) and the residual network (Residual: a flat parameter vector + offsets) travel with every call: one library serves every
filter config and every set of weights.  The library carries every scg_hip.h entry point as well (_lib.EXPORTS) and scg_cbf_certify:
HipVecEnv(..., policy=(hidden, activation), cbf_nn=True) drives its handle with it.  No fallback lives here: a shape or a system the
library does not serve is an error."""
import ctypes as C
import os
import subprocess

from safe_control_gym_amd import _adversarial, _cbf
from safe_control_gym_amd import _lib as L

SRC = os.path.join(L.CSRC_DIR, 'scg_cbf_nn.hip')
HEADER = os.path.normpath(os.path.join(L.CSRC_DIR, '..', '..', 'include', 'scg_cbf_nn.h'))
DEPS = [os.path.join(L.CSRC_DIR, s) for s in L.SOURCES + L.HEADERS] + \
    [_adversarial.HEADER, _cbf.HEADER, SRC, HEADER, os.path.normpath(os.path.join(L.CSRC_DIR, '..', '..', 'include', 'scg_learn.h')),
     os.path.normpath(os.path.join(L.CSRC_DIR, '..', '..', 'include', 'scg_actor_rollout.h')),
     os.path.join(L.CSRC_DIR, 'scg_cbf_core.h'), os.path.join(L.CSRC_DIR, 'scg_mlp_rows.h')]
PREFIX = 'libscg_cbfnn_'
HIDDEN = 256                      # the residual network served: MLP(4 -> 256 -> 256 -> 2), relu
NX, NOUT = 4, 2
LDS_LIMIT = 160 * 1024            # a CU's LDS
CERT_ROWS_PER_GROUP = 256         # scg_cbf_nn_certify: 8 column tiles of 32 rows per 512-thread workgroup


class MlpLayout(C.Structure):
    """scg_mlp_layout (include/scg_learn.h)."""
    _fields_ = [(n, C.c_int32) for n in ('W1', 'b1', 'W2', 'b2', 'W3', 'b3')]


class Residual(C.Structure):
    """scg_cbf_residual."""
    _fields_ = [('d_params', C.c_void_p), ('mlp', MlpLayout), ('hidden', C.c_int32)]


class Mode(C.Structure):
    """scg_cbf_nn_mode."""
    _fields_ = [('deterministic', C.c_int32), ('uniform', C.c_int32), ('act_low', C.c_float), ('act_high', C.c_float), ('blend', C.c_float)]


def residual_sizes(hidden=HIDDEN):
    """Word counts of the residual network's six tensors in packing order (W1, b1, W2, b2, W3, b3)."""
    return [hidden * NX, hidden, hidden * hidden, hidden, NOUT * hidden, NOUT]


def residual_of(flat, hidden=HIDDEN):
    """Residual of a flat float32 device tensor packed in residual_sizes' order."""
    sizes = residual_sizes(hidden)
    if flat.numel() != sum(sizes):
        raise ValueError(f'the packed residual network holds {sum(sizes)} words, got {flat.numel()}')
    offs = [0]
    for s in sizes[:-1]:
        offs.append(offs[-1] + s)
    return Residual(d_params=flat.data_ptr(), mlp=MlpLayout(*offs), hidden=hidden)


# ---- LDS arithmetic (csrc/scg_mlp_rows.h: MlpRowsLds<4, 2, G>; csrc/scg_mlp.h: MlpLds<obs_dim, hidden, 1, 16>), in bytes
def rows_image_bytes(tiles):
    l1q = 4 * ((NX + 7) // 8)
    nt = HIDDEN // 32
    b3 = nt * l1q * 64 + NOUT * HIDDEN + 2 * HIDDEN
    x = (b3 + NOUT + 3) // 4 * 4
    part = x + tiles * l1q * 64 + 2 * nt * 1024
    return (part + tiles * 8 * 32 * NOUT + 3) // 4 * 4 * 4


def actor_image_bytes(obs_dim, hidden, act_dim=1):
    l1q = 4 * ((obs_dim + 7) // 8)
    nt = hidden // 32
    b3 = nt * l1q * 64 + nt * nt * 64 * 16 + act_dim * hidden + 2 * hidden
    return (b3 + act_dim + 3) // 4 * 4 * 4


def rollout_lds_bytes(obs_dim, hidden, tiles):
    """Dynamic LDS of scg_rollout_cbf_nn with `tiles` column tiles per workgroup (scg_cbf_nn_lds reports the same number)."""
    return rows_image_bytes(tiles) + actor_image_bytes(obs_dim, hidden)


def rollout_tiles(obs_dim, hidden, num_envs):
    """Column tiles per workgroup scg_rollout_cbf_nn uses: csrc/scg_actor_rollout_wide.h's rule; G = 1 at every N when the actor's image
    does not fit beside the G = 8 row-split image; None when it does not fit at G = 1 either."""
    if rollout_lds_bytes(obs_dim, hidden, 1) > LDS_LIMIT:
        return None
    if rollout_lds_bytes(obs_dim, hidden, 8) > LDS_LIMIT:
        return 1
    return 1 if num_envs <= 32768 else 8


def supported(env_id, obs_dim, hidden, act_dim, activation, kind=None):
    """The filter serves the cartpole with PPO's actor shapes (the two-element policy= tuples) whose image fits a CU's LDS beside the
    residual's.  A SAC / DDPG actor (kind given) is not served: a 256-wide actor and the residual do not share a register file."""
    if kind is not None:
        return False
    try:
        hidden = int(hidden)
    except (TypeError, ValueError):
        return False
    return env_id == 'cartpole' and act_dim == 1 and obs_dim in (4, 8) and hidden != L.WIDE_HIDDEN and \
        L.policy_supported(obs_dim, hidden, act_dim, activation) and rollout_tiles(obs_dim, hidden, 1) is not None


def source_hash():
    import hashlib
    h = hashlib.sha256()
    for p in DEPS:
        with open(p, 'rb') as f:
            h.update(os.path.basename(p).encode() + b'\0' + f.read())
    return int.from_bytes(h.digest()[:8], 'little')


def lib_path(spec_hash, hidden, activation):
    return os.path.join(L.SPEC_DIR, f'{PREFIX}{spec_hash:016x}_{int(hidden)}_{activation}.so')


def build(cfg, hidden, activation, force=False, remarks=False):
    """Compile the library for this scg_config and actor shape (hipcc, gfx950).  remarks=True: return (path, the compiler's
    kernel-resource-usage remarks) instead of the path, and always compile."""
    if activation not in L.POLICY_ACTS:
        raise L.ScgError(f'no fused cbf_nn rollout for activation {activation}')
    src, h = L.spec_source(cfg)
    hdr, _ = L.spec_paths(h)
    so = lib_path(h, hidden, activation)
    if not force and not remarks and os.path.exists(so) and L._lib_source_hash(so) == source_hash():
        return so
    os.makedirs(L.SPEC_DIR, exist_ok=True)
    with open(hdr, 'w') as f:
        f.write(src)
    cmd = [L._hipcc(), '--offload-arch=gfx950', '-O3', '-ffp-contract=on', '-std=c++17', '-fPIC', '-shared', '-DSCG_SPEC', '-include', hdr,
           f'-DSCG_SRC_HASH=0x{source_hash():016x}ULL', f'-DSCG_POLICY_H={int(hidden)}', f'-DSCG_POLICY_ACT={L.POLICY_ACTS[activation]}', '-o', so]
    if remarks:
        cmd.append('-Rpass-analysis=kernel-resource-usage')
    res = None
    for extra in L.sched_flags(cfg):
        res = subprocess.run(cmd + extra + [SRC], capture_output=True, text=True)
        if res.returncode == 0:
            return (so, res.stderr) if remarks else so
    raise L.ScgError('hipcc failed (cbf_nn build):\n' + res.stdout + res.stderr)


_libs = {}


def bind(so):
    """_lib._bind + the argument types of this header's entry points (and scg_cbf_certify's)."""
    D = L._bind(so)
    D.scg_cbf_certify.argtypes = [C.c_void_p, C.POINTER(_cbf.CbfParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                  C.c_void_p]
    D.scg_cbf_nn_certify.argtypes = [C.c_void_p, C.POINTER(_cbf.CbfParams), C.POINTER(Residual), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    D.scg_rollout_cbf_nn.argtypes = [C.c_void_p, C.POINTER(_adversarial.ActorPtrs), C.POINTER(_cbf.CbfParams), C.POINTER(Residual),
                                     C.POINTER(Mode), C.c_int, C.POINTER(L.PolicyRollout), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    D.scg_cbf_nn_shape.argtypes = [C.POINTER(C.c_int32)] * 5
    D.scg_cbf_nn_lds.argtypes = [C.c_int, C.POINTER(C.c_int32)]
    return D


def lib_for(cfg, hidden, activation):
    """The bound library (every _lib.EXPORTS symbol + this header's), built now if missing or stale."""
    _, h = L.spec_source(cfg)
    key = (h, int(hidden), activation)
    if key in _libs:
        return _libs[key]
    so = lib_path(*key)
    if not os.path.exists(so) or L._lib_source_hash(so) != source_hash():
        if not os.path.exists(L._hipcc()):
            raise L.ScgError(f'{so} is missing or stale and hipcc is not available to build it')
        build(cfg, hidden, activation, force=True)
    D = bind(so)
    if int(D.scg_spec_hash()) != h:
        raise L.ScgError(f'{so} was built for another config')
    if shape_of(D)[:3] != (int(hidden), L.POLICY_ACTS[activation], HIDDEN):
        raise L.ScgError(f'{so} was built for another actor shape or another system')
    _libs[key] = D
    return D


def shape_of(D):
    """(actor hidden, activation id, residual hidden, obs_dim, act_dim) of a bound library (zeros: not a float32 cartpole library)."""
    v = [C.c_int32() for _ in range(5)]
    D.scg_cbf_nn_shape(*[C.byref(x) for x in v])
    return tuple(x.value for x in v)


def lds_of(D, tiles):
    v = C.c_int32()
    D.scg_cbf_nn_lds(int(tiles), C.byref(v))
    return v.value

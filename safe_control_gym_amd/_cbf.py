"""ctypes binding + builder of libscg_cbfroll_<spechash>_<hidden>_<activation>.so (include/scg_cbf.h): the CBF-QP safety filter as a
batched certify kernel and as the policy rollout with the filter between the actor and the env step, compiled per task config and
actor shape from csrc/scg_cbf.hip.  The filter's own settings travel by value (CbfParams): one library serves every filter config.
The library carries every scg_hip.h entry point as well (_lib.EXPORTS): HipVecEnv(..., policy=(hidden, activation), cbf=True) drives
its handle with it.  With a kind and hidden width 256 the library is built from csrc/scg_cbf_wide.hip instead (same name pattern, its
own source hash: source_hash(wide=True)) and serves scg_rollout_cbf_actor and scg_cbf_certify; scg_rollout_cbf refuses there.  No fallback lives here: a shape or a system the library does not serve is an error."""
import ctypes as C
import os
import subprocess

from safe_control_gym_amd import _adversarial
from safe_control_gym_amd import _lib as L

SRC = os.path.join(L.CSRC_DIR, 'scg_cbf.hip')
HEADER = os.path.normpath(os.path.join(L.CSRC_DIR, '..', '..', 'include', 'scg_cbf.h'))
# the env library's hash inputs (_lib.SOURCES + _lib.HEADERS), the adversarial header the ABI includes, and the two new files
DEPS = [os.path.join(L.CSRC_DIR, s) for s in L.SOURCES + L.HEADERS] + [_adversarial.HEADER, SRC, HEADER,
                                                                         os.path.join(L.CSRC_DIR, 'scg_cbf_core.h'),
                                                                         os.path.join(L.CSRC_DIR, 'scg_cbf_actor.h')] + \
    [os.path.normpath(os.path.join(L.CSRC_DIR, d)) for d in L.ACTOR_DEPS[1:]]
PREFIX = 'libscg_cbfroll_'
# the filter behind an actor of hidden width 256 (kind given): its own translation unit on csrc/scg_actor_rollout_wide.h
WIDE_SRC = os.path.join(L.CSRC_DIR, 'scg_cbf_wide.hip')
WIDE_DEPS = [os.path.join(L.CSRC_DIR, s) for s in L.SOURCES + L.HEADERS] + [_adversarial.HEADER, WIDE_SRC, HEADER,
                                                                              os.path.join(L.CSRC_DIR, 'scg_cbf_core.h')] + \
    [os.path.normpath(os.path.join(L.CSRC_DIR, d)) for d in L.WIDE_DEPS[1:]]


def is_wide(hidden, kind):
    return kind is not None and int(hidden) == L.WIDE_HIDDEN


class CbfParams(C.Structure):
    """scg_cbf_params (include/scg_cbf.h)."""
    _fields_ = [('L', C.c_float * 4)] + [(n, C.c_float) for n in ('m', 'M', 'l', 'g', 'slope', 'slack_weight', 'slack_tolerance', 'lo', 'hi')] + \
               [('soft', C.c_int32)]


def supported(env_id, obs_dim, hidden, act_dim, activation):
    """The filter serves the cartpole (the reference's CBF raises for every other system) with the fused policy rollout's actor shapes."""
    return env_id == 'cartpole' and act_dim == 1 and obs_dim in (4, 8) and L.policy_supported(obs_dim, hidden, act_dim, activation)


def supported_actor(env_id, obs_dim, hidden, act_dim, activation, kind):
    """The filter behind a SAC / DDPG actor (scg_rollout_cbf_actor): the cartpole with the fused actor rollout's shapes."""
    return kind in L.ACTOR_KINDS and env_id == 'cartpole' and act_dim == 1 and obs_dim in (4, 8) and \
        L.policy_supported(obs_dim, hidden, act_dim, activation)


def supported_wide_actor(env_id, obs_dim, hidden, act_dim, activation, kind):
    """The same at hidden width 256 (csrc/scg_cbf_wide.hip on scg_actor_rollout_wide.h): a kind is required, PPO's actor has no such variant."""
    return kind in L.ACTOR_KINDS and env_id == 'cartpole' and act_dim == 1 and obs_dim in (4, 8) and int(hidden) == L.WIDE_HIDDEN and \
        L.actor_supported(obs_dim, hidden, act_dim, activation)


def source_hash(wide=False):
    import hashlib
    h = hashlib.sha256()
    for p in WIDE_DEPS if wide else DEPS:
        with open(p, 'rb') as f:
            h.update(os.path.basename(p).encode() + b'\0' + f.read())
    return int.from_bytes(h.digest()[:8], 'little')


def lib_path(spec_hash, hidden, activation, kind=None):
    return os.path.join(L.SPEC_DIR, f'{PREFIX}{spec_hash:016x}_{int(hidden)}_{activation}{"_" + kind if kind else ""}.so')


def build(cfg, hidden, activation, kind=None, force=False):
    """Compile the filter library for this scg_config and actor shape (hipcc, gfx950); kind 'sac' | 'ddpg': the variant that also
    carries scg_rollout_actor / scg_rollout_cbf_actor for that actor."""
    if activation not in L.POLICY_ACTS:
        raise L.ScgError(f'no fused CBF rollout for activation {activation}')
    if kind is not None and kind not in L.ACTOR_KINDS:
        raise L.ScgError(f'no fused CBF rollout for actor kind {kind}')
    src, h = L.spec_source(cfg)
    hdr, _ = L.spec_paths(h)
    so = lib_path(h, hidden, activation, kind)
    wide = is_wide(hidden, kind)
    if not force and os.path.exists(so) and L._lib_source_hash(so) == source_hash(wide):
        return so
    os.makedirs(L.SPEC_DIR, exist_ok=True)
    with open(hdr, 'w') as f:
        f.write(src)
    cmd = [L._hipcc(), '--offload-arch=gfx950', '-O3', '-ffp-contract=on', '-std=c++17', '-fPIC', '-shared', '-DSCG_SPEC', '-include', hdr,
           f'-DSCG_SRC_HASH=0x{source_hash(wide):016x}ULL', '-o', so]
    if wide:
        cmd += [f'-DSCG_ACTOR_WIDE_H={L.WIDE_HIDDEN}', f'-DSCG_ACTOR_WIDE_ACT={L.POLICY_ACTS[activation]}',
                f'-DSCG_ACTOR_WIDE_KIND={L.ACTOR_KINDS[kind]}']
    else:
        cmd += [f'-DSCG_POLICY_H={int(hidden)}', f'-DSCG_POLICY_ACT={L.POLICY_ACTS[activation]}']
        if kind is not None:
            cmd.append(f'-DSCG_POLICY_KIND={L.ACTOR_KINDS[kind]}')
    res = None
    for extra in L.sched_flags(cfg):
        res = subprocess.run(cmd + extra + [WIDE_SRC if wide else SRC], capture_output=True, text=True)
        if res.returncode == 0:
            return so
    raise L.ScgError('hipcc failed (CBF rollout build):\n' + res.stdout + res.stderr)


_libs = {}


def bind(so):
    """_lib._bind + the argument types of this header's entry points."""
    D = L._bind(so)
    D.scg_cbf_certify.argtypes = [C.c_void_p, C.POINTER(CbfParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                  C.c_void_p]
    D.scg_rollout_cbf.argtypes = [C.c_void_p, C.POINTER(_adversarial.ActorPtrs), C.POINTER(CbfParams), C.c_int, C.c_int,
                                  C.POINTER(L.PolicyRollout), C.c_void_p, C.c_void_p, C.c_void_p]
    D.scg_rollout_cbf_actor.argtypes = [C.c_void_p, C.POINTER(L.Actor), C.POINTER(CbfParams), C.c_int, C.POINTER(L.PolicyRollout),
                                        C.c_void_p, C.c_void_p, C.c_void_p]
    D.scg_cbf_shape.argtypes = [C.POINTER(C.c_int32)] * 4
    return D


def lib_for(cfg, hidden, activation, kind=None):
    """The bound library (every _lib.EXPORTS symbol + scg_cbf_certify / scg_rollout_cbf / scg_rollout_cbf_actor), built now if
    missing or stale."""
    _, h = L.spec_source(cfg)
    key = (h, int(hidden), activation) + ((kind,) if kind else ())
    if key in _libs:
        return _libs[key]
    so = lib_path(*key)
    if not os.path.exists(so) or L._lib_source_hash(so) != source_hash(is_wide(hidden, kind)):
        if not os.path.exists(L._hipcc()):
            raise L.ScgError(f'{so} is missing or stale and hipcc is not available to build it')
        build(cfg, hidden, activation, kind, force=True)
    D = bind(so)
    if int(D.scg_spec_hash()) != h:
        raise L.ScgError(f'{so} was built for another config')
    if shape_of(D)[:2] != (int(hidden), L.POLICY_ACTS[activation]):
        raise L.ScgError(f'{so} was built for another actor shape or another system')
    if kind and actor_shape_of(D) != (int(hidden), L.POLICY_ACTS[activation], L.ACTOR_KINDS[kind]):
        raise L.ScgError(f'{so} was built for another actor kind')
    _libs[key] = D
    return D


def actor_shape_of(D):
    """(hidden, activation id, kind id) of the actor rollout a bound library carries (zeros: none)."""
    v = [C.c_int32() for _ in range(3)]
    D.scg_actor_rollout_shape(*[C.byref(x) for x in v])
    return tuple(x.value for x in v)


def shape_of(D):
    """(hidden, activation id, obs_dim, act_dim) of a bound library (zeros: its task is not the cartpole)."""
    v = [C.c_int32() for _ in range(4)]
    D.scg_cbf_shape(*[C.byref(x) for x in v])
    return tuple(x.value for x in v)


def actor_ptrs_of_policy(policy):
    """ActorPtrs of an _lib.Policy (flat float32 parameter vector + word offsets)."""
    base = int(policy.d_params)
    return _adversarial.ActorPtrs(*[base + 4 * int(getattr(policy, n)) for n in ('W1', 'b1', 'W2', 'b2', 'W3', 'b3', 'logstd_off')])

"""ctypes binding + builder of libscg_ilqr_<spechash>.so (include/scg_ilqr.h): the LQR / iLQR baseline controllers' two kernels — the
closed-loop rollout with an affine time-varying state feedback in the loop and iLQR's backward pass — and the PID baseline's rollout
(include/scg_pid.h, csrc/scg_pid.h) and the LDS-resident backward pass that serves Quadrotor 3D (include/scg_ilqr_wide.h,
csrc/scg_ilqr_wide.h), compiled per task config from csrc/scg_ilqr.hip.  The controllers' own settings (Q, R, the prior model's parameters) travel by value: one library serves every
controller config of its task.  The library carries every scg_hip.h entry point as well (_lib.EXPORTS): HipVecEnv(..., ilqr=True)
drives its handle with it.  No fallback lives here: a system or an env config the library does not serve is an error."""
import ctypes as C
import os
import subprocess

from safe_control_gym_amd import _lib as L

SRC = os.path.join(L.CSRC_DIR, 'scg_ilqr.hip')
HEADER = os.path.normpath(os.path.join(L.CSRC_DIR, '..', '..', 'include', 'scg_ilqr.h'))
PID_SRC = os.path.join(L.CSRC_DIR, 'scg_pid.h')                    # the PID rollout: included by scg_ilqr.hip
PID_HEADER = os.path.normpath(os.path.join(L.CSRC_DIR, '..', '..', 'include', 'scg_pid.h'))
WIDE_SRC = os.path.join(L.CSRC_DIR, 'scg_ilqr_wide.h')              # the LDS-resident backward pass: included by scg_ilqr.hip
WIDE_HEADER = os.path.normpath(os.path.join(L.CSRC_DIR, '..', '..', 'include', 'scg_ilqr_wide.h'))
DEPS = [os.path.join(L.CSRC_DIR, s) for s in L.SOURCES + L.HEADERS] + [SRC, HEADER, PID_SRC, PID_HEADER, WIDE_SRC, WIDE_HEADER]
PREFIX = 'libscg_ilqr_'


class FeedbackRollout(C.Structure):
    """scg_feedback_rollout (include/scg_ilqr.h)."""
    _fields_ = [('d_gains', C.c_void_p), ('d_ff', C.c_void_p), ('schedule_len', C.c_int32), ('per_env', C.c_int32), ('d_x', C.c_void_p),
                ('d_u', C.c_void_p), ('d_final_obs', C.c_void_p), ('d_stats', C.c_void_p), ('d_n_steps', C.c_void_p),
                ('d_final_flags', C.c_void_p), ('d_reward', C.c_void_p), ('d_done', C.c_void_p), ('d_flags', C.c_void_p)]


class PidConfig(C.Structure):
    """scg_pid_config (include/scg_pid.h)."""
    _fields_ = [('kf', C.c_double), ('gravity', C.c_double), ('pwm2rpm_scale', C.c_double), ('pwm2rpm_const', C.c_double), ('min_pwm', C.c_double),
                ('max_pwm', C.c_double), ('dt', C.c_double)]


class PidRollout(C.Structure):
    """scg_pid_rollout (include/scg_pid.h)."""
    _fields_ = [('d_gains', C.c_void_p), ('per_env', C.c_int32), ('reserved', C.c_int32), ('d_pid_state', C.c_void_p), ('config', PidConfig),
                ('d_x', C.c_void_p), ('d_u', C.c_void_p), ('d_final_obs', C.c_void_p), ('d_stats', C.c_void_p), ('d_n_steps', C.c_void_p),
                ('d_final_flags', C.c_void_p), ('d_reward', C.c_void_p), ('d_done', C.c_void_p), ('d_flags', C.c_void_p)]


class IlqrModel(C.Structure):
    """scg_ilqr_model (include/scg_ilqr.h)."""
    _fields_ = [('q', C.c_double * 12), ('r', C.c_double * 4), ('u_eq', C.c_double * 4), ('par', C.c_double * 4), ('arm', C.c_double), ('dt', C.c_double),
                ('eps', C.c_double)]


def source_hash():
    import hashlib
    h = hashlib.sha256()
    for p in DEPS:
        with open(p, 'rb') as f:
            h.update(os.path.basename(p).encode() + b'\0' + f.read())
    return int.from_bytes(h.digest()[:8], 'little')


def lib_path(spec_hash):
    return os.path.join(L.SPEC_DIR, f'{PREFIX}{spec_hash:016x}.so')


def build(cfg, force=False, extra_flags=()):
    """Compile the controller library for this scg_config (hipcc, gfx950)."""
    src, h = L.spec_source(cfg)
    hdr, _ = L.spec_paths(h)
    so = lib_path(h)
    if not force and os.path.exists(so) and L._lib_source_hash(so) == source_hash():
        return so
    os.makedirs(L.SPEC_DIR, exist_ok=True)
    with open(hdr, 'w') as f:
        f.write(src)
    cmd = [L._hipcc(), '--offload-arch=gfx950', '-O3', '-ffp-contract=on', '-std=c++17', '-fPIC', '-shared', '-DSCG_SPEC', '-include', hdr,
           f'-DSCG_SRC_HASH=0x{source_hash():016x}ULL', '-o', so] + list(extra_flags)
    res = None
    for extra in L.sched_flags(cfg):
        res = subprocess.run(cmd + extra + [SRC], capture_output=True, text=True)
        if res.returncode == 0:
            build.last_log = res.stdout + res.stderr
            return so
    raise L.ScgError('hipcc failed (LQR / iLQR build):\n' + res.stdout + res.stderr)


_libs = {}


def lib_for(cfg):
    """The bound library (every _lib.EXPORTS symbol + scg_rollout_feedback / scg_ilqr_backward / scg_ilqr_backward_wide / scg_rollout_pid), built now if missing or stale."""
    _, h = L.spec_source(cfg)
    if h in _libs:
        return _libs[h]
    so = lib_path(h)
    if not os.path.exists(so) or L._lib_source_hash(so) != source_hash():
        if not os.path.exists(L._hipcc()):
            raise L.ScgError(f'{so} is missing or stale and hipcc is not available to build it')
        build(cfg, force=True)
    D = L._bind(so)
    if int(D.scg_spec_hash()) != h:
        raise L.ScgError(f'{so} was built for another config')
    D.scg_rollout_feedback.argtypes = [C.c_void_p, C.c_int, C.POINTER(FeedbackRollout), C.c_void_p]
    D.scg_ilqr_backward.argtypes = [C.c_void_p, C.POINTER(IlqrModel), C.c_int] + [C.c_void_p] * 9
    D.scg_ilqr_backward_wide.argtypes = [C.c_void_p, C.POINTER(IlqrModel), C.c_int] + [C.c_void_p] * 9
    D.scg_ilqr_snapshot.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    D.scg_ilqr_restart.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    D.scg_rollout_pid.argtypes = [C.c_void_p, C.c_int, C.POINTER(PidRollout), C.c_void_p]
    _libs[h] = D
    return D

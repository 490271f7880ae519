"""ctypes binding + builder of libscg_ddpg_<obs>_<hidden>_<act_dim>_<activation>.so (include/scg_ddpg.h): one fused gradient step
of DDPGAgent.update on the matrix cores, the collector's noisy action (deterministic actor + the reference's exploration noise, one
launch) and its ring push, compiled per network shape from csrc/scg_ddpg.hip.  No fallback lives here: ddpg.py uses the PyTorch
update, visibly, for shapes this library does not serve."""
import ctypes as C
import os

from safe_control_gym_amd import _lib as L
from safe_control_gym_amd import _shapelib
from safe_control_gym_amd._learn import ACTS, MlpLayout

SRC = os.path.join(L.CSRC_DIR, 'scg_ddpg.hip')
DEPS = [SRC] + [os.path.join(L.CSRC_DIR, h) for h in ('scg_wide.h', 'scg_offpolicy_step.h', 'scg_adam.h', 'scg_mlp.h', 'scg_once.h', 'scg_rng.h')] + \
    [os.path.normpath(os.path.join(L.CSRC_DIR, '..', '..', 'include', h)) for h in ('scg_ddpg.h', 'scg_learn.h')]
PREFIX = 'libscg_ddpg_'

NOISE_NONE, NOISE_OU, NOISE_GAUSSIAN = 0, 1, 2


class DdpgArgs(C.Structure):
    _fields_ = [('d_params', C.c_void_p), ('d_target', C.c_void_p), ('d_grad', C.c_void_p), ('d_m', C.c_void_p), ('d_v', C.c_void_p),
                ('d_steps', C.c_void_p), ('actor', MlpLayout), ('q', MlpLayout), ('n_actor', C.c_int32), ('n_params', C.c_int32),
                ('d_obs', C.c_void_p), ('d_act', C.c_void_p), ('d_rew', C.c_void_p), ('d_next_obs', C.c_void_p), ('d_mask', C.c_void_p),
                ('d_ring_size', C.c_void_p), ('batch', C.c_int32), ('gamma', C.c_float), ('tau', C.c_float), ('actor_lr', C.c_float),
                ('critic_lr', C.c_float), ('act_low', C.c_float * 4), ('act_high', C.c_float * 4), ('seed', C.c_uint64),
                ('d_counter', C.c_void_p), ('d_idx_in', C.c_void_p), ('d_workspace', C.c_void_p), ('d_stats', C.c_void_p),
                ('d_stats_acc', C.c_void_p)]


class DdpgNoise(C.Structure):
    _fields_ = [('kind', C.c_int32), ('theta', C.c_double), ('dt', C.c_double), ('std_start', C.c_double), ('std_end', C.c_double),
                ('std_inc', C.c_double), ('d_x_prev', C.c_void_p), ('d_x_next', C.c_void_p), ('d_calls', C.c_void_p), ('d_pending', C.c_void_p)]


DdpgRing = _shapelib.Ring
supported = _shapelib.supported


def source_hash():
    return _shapelib.source_hash(DEPS)


def lib_path(obs_dim, hidden, act_dim, activation):
    return os.path.join(L.SPEC_DIR, f'{PREFIX}{obs_dim}_{hidden}_{act_dim}_{activation}.so')


def build(obs_dim, hidden, act_dim, activation, force=False):
    if not supported(obs_dim, hidden, act_dim, activation):
        raise L.ScgError(f'no fused DDPG update for obs {obs_dim} hidden {hidden} act {act_dim} {activation}')
    defines = {'SCG_D_NOBS': obs_dim, 'SCG_D_H': hidden, 'SCG_D_NU': act_dim, 'SCG_D_ACT': ACTS[activation]}
    return _shapelib.build(lib_path(obs_dim, hidden, act_dim, activation), SRC, DEPS, defines, 'DDPG', force=force)


def _bind(D):
    D.scg_ddpg_last_error.restype = C.c_char_p
    D.scg_ddpg_workspace_bytes.restype = C.c_size_t
    D.scg_ddpg_workspace_bytes.argtypes = [C.c_int]
    D.scg_ddpg_update.argtypes = [C.POINTER(DdpgArgs), C.c_void_p]
    D.scg_ddpg_update_n.argtypes = [C.POINTER(DdpgArgs), C.c_int, C.c_void_p]
    fl4 = C.POINTER(C.c_float)
    D.scg_ddpg_act.argtypes = [C.c_void_p, C.POINTER(MlpLayout), fl4, fl4, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    D.scg_ddpg_noisy_act.argtypes = [C.c_void_p, C.POINTER(MlpLayout), fl4, fl4, C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_int,
                                     C.POINTER(DdpgNoise), C.c_void_p, C.c_void_p, C.c_void_p]
    D.scg_ddpg_noise_commit.argtypes = [C.POINTER(DdpgNoise), C.c_void_p]
    D.scg_ddpg_push.argtypes = [C.POINTER(DdpgRing), C.POINTER(DdpgNoise), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]


_libs = {}


def lib(obs_dim, hidden, act_dim, activation):
    key = (obs_dim, hidden, act_dim, activation)
    return _shapelib.load(_libs, key, lib_path(*key), DEPS, lambda: build(*key, force=True), _bind, 'scg_ddpg_shape',
                          (obs_dim, hidden, act_dim, ACTS[activation]))


def check(D, rc):
    if rc != 0:
        raise L.ScgError(f'libscg_ddpg error {rc}: {D.scg_ddpg_last_error().decode()}')

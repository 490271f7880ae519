"""ctypes binding + builder of libscg_sac_<obs>_<hidden>_<act_dim>_<activation>.so (include/scg_sac.h): one fused gradient step
of SACAgent.update on the matrix cores, compiled per network shape from csrc/scg_sac.hip (hipcc cross-compiles without a
GPU; ~8 s).  No fallback lives here: sac.py uses the PyTorch update, visibly, for shapes this library does not serve."""
import ctypes as C
import os

from safe_control_gym_amd import _lib as L
from safe_control_gym_amd import _shapelib
from safe_control_gym_amd._learn import ACTS, MlpLayout

SRC = os.path.join(L.CSRC_DIR, 'scg_sac.hip')
DEPS = [SRC] + [os.path.join(L.CSRC_DIR, h) for h in ('scg_wide.h', 'scg_offpolicy_step.h', 'scg_adam.h', 'scg_mlp.h', 'scg_once.h', 'scg_rng.h')] + \
    [os.path.normpath(os.path.join(L.CSRC_DIR, '..', '..', 'include', h)) for h in ('scg_sac.h', 'scg_learn.h')]


class SacArgs(C.Structure):
    _fields_ = [('d_params', C.c_void_p), ('d_target', C.c_void_p), ('d_grad', C.c_void_p), ('d_m', C.c_void_p), ('d_v', C.c_void_p),
                ('d_steps', C.c_void_p), ('actor', MlpLayout), ('q1', MlpLayout), ('q2', MlpLayout), ('n_actor', C.c_int32),
                ('n_params', C.c_int32), ('d_obs', C.c_void_p), ('d_act', C.c_void_p), ('d_rew', C.c_void_p), ('d_next_obs', C.c_void_p),
                ('d_mask', C.c_void_p), ('d_ring_size', C.c_void_p), ('batch', C.c_int32), ('gamma', C.c_float), ('tau', C.c_float),
                ('actor_lr', C.c_float), ('critic_lr', C.c_float), ('entropy_lr', C.c_float), ('use_entropy_tuning', C.c_int32),
                ('target_entropy', C.c_float), ('act_low', C.c_float * 4), ('act_high', C.c_float * 4), ('seed', C.c_uint64),
                ('d_counter', C.c_void_p), ('d_idx_in', C.c_void_p), ('d_eps_in', C.c_void_p), ('d_eps_next_in', C.c_void_p),
                ('d_workspace', C.c_void_p), ('d_stats', C.c_void_p), ('d_stats_acc', C.c_void_p), ('phases', C.c_int32)]


SacRing = _shapelib.Ring
supported = _shapelib.supported
ACTOR_GRAD, CRITIC_GRAD, FINISH, ALL = 1, 2, 4, 7


def source_hash():
    return _shapelib.source_hash(DEPS)


def lib_path(obs_dim, hidden, act_dim, activation):
    return os.path.join(L.SPEC_DIR, f'libscg_sac_{obs_dim}_{hidden}_{act_dim}_{activation}.so')


def build(obs_dim, hidden, act_dim, activation, force=False):
    if not supported(obs_dim, hidden, act_dim, activation):
        raise L.ScgError(f'no fused SAC update for obs {obs_dim} hidden {hidden} act {act_dim} {activation}')
    defines = {'SCG_S_NOBS': obs_dim, 'SCG_S_H': hidden, 'SCG_S_NU': act_dim, 'SCG_S_ACT': ACTS[activation]}
    return _shapelib.build(lib_path(obs_dim, hidden, act_dim, activation), SRC, DEPS, defines, 'SAC', 'SCG_SAC_FLAGS', force)


def _bind(D):
    D.scg_sac_last_error.restype = C.c_char_p
    D.scg_sac_workspace_bytes.restype = C.c_size_t
    D.scg_sac_workspace_bytes.argtypes = [C.c_int]
    D.scg_sac_update.argtypes = [C.POINTER(SacArgs), C.c_void_p]
    D.scg_sac_update_n.argtypes = [C.POINTER(SacArgs), C.c_int, C.c_void_p]
    D.scg_sac_act.argtypes = [C.c_void_p, C.POINTER(MlpLayout), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_void_p, C.c_int, C.c_void_p,
                              C.c_void_p]
    D.scg_sac_sample.argtypes = [C.c_void_p, C.POINTER(MlpLayout), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_void_p, C.c_int, C.c_uint64,
                                 C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    D.scg_sac_push.argtypes = [C.POINTER(SacRing), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]


_libs = {}


def lib(obs_dim, hidden, act_dim, activation):
    key = (obs_dim, hidden, act_dim, activation)
    return _shapelib.load(_libs, key, lib_path(*key), DEPS, lambda: build(*key, force=True), _bind, 'scg_sac_shape',
                          (obs_dim, hidden, act_dim, ACTS[activation]))


def check(D, rc):
    if rc != 0:
        raise L.ScgError(f'libscg_sac error {rc}: {D.scg_sac_last_error().decode()}')

"""ctypes binding + builder of libscg_resupd_256.so (include/scg_cbf_nn_update.h): the Adam steps of the cbf_nn filter's residual
network, every minibatch of a training episode enqueued by one call, compiled from csrc/scg_cbf_nn_update.hip (hipcc cross-compiles
without a GPU).  One network shape, no env handle, no task config: one library.  No fallback lives here: a batch the library does not
serve is an error."""
import ctypes as C
import os

from safe_control_gym_amd import _lib as L
from safe_control_gym_amd import _shapelib

SRC = os.path.join(L.CSRC_DIR, 'scg_cbf_nn_update.hip')
HEADER = os.path.normpath(os.path.join(L.CSRC_DIR, '..', '..', 'include', 'scg_cbf_nn_update.h'))
DEPS = [SRC, os.path.join(L.CSRC_DIR, 'scg_adam.h'), HEADER]
PREFIX = 'libscg_resupd_'             # (not a name libscg_cbfnn_ is a prefix of: __graft_entry__.expected_source_hash dispatches on it)
NX, HIDDEN, NOUT = 4, 256, 2
N_PARAMS = HIDDEN * NX + HIDDEN + HIDDEN * HIDDEN + HIDDEN + NOUT * HIDDEN + NOUT
MAX_BATCH = 256


class UpdateArgs(C.Structure):
    """scg_cbf_nn_update_args."""
    _fields_ = [('d_params', C.c_void_p), ('d_m', C.c_void_p), ('d_v', C.c_void_p), ('d_step', C.c_void_p), ('d_state', C.c_void_p),
                ('d_act', C.c_void_p), ('d_barrier_dot', C.c_void_p), ('d_barrier_dot_approx', C.c_void_p), ('d_rows', C.c_void_p),
                ('n_batches', C.c_int32), ('batch', C.c_int32), ('lr', C.c_float), ('train', C.c_int32), ('d_loss', C.c_void_p),
                ('d_grad', C.c_void_p), ('d_work', C.c_void_p)]


def source_hash():
    return _shapelib.source_hash(DEPS)


def lib_path():
    return os.path.join(L.SPEC_DIR, f'{PREFIX}{HIDDEN}.so')


def build(force=False):
    return _shapelib.build(lib_path(), SRC, DEPS, {}, 'cbf_nn update', 'SCG_CBF_NN_UPDATE_FLAGS', force)


def _bind(D):
    D.scg_cbf_nn_update_last_error.restype = C.c_char_p
    D.scg_cbf_nn_update.argtypes = [C.POINTER(UpdateArgs), C.c_void_p]
    D.scg_cbf_nn_update_work_bytes.argtypes = [C.c_int32, C.POINTER(C.c_int64)]
    D.scg_cbf_nn_update_shape.argtypes = [C.POINTER(C.c_int32)] * 4


_libs = {}


def lib():
    return _shapelib.load(_libs, HIDDEN, lib_path(), DEPS, lambda: build(force=True), _bind, 'scg_cbf_nn_update_shape',
                          (NX, HIDDEN, NOUT, MAX_BATCH))


def check(D, rc):
    if rc != 0:
        raise L.ScgError(f'libscg_resupd error {rc}: {D.scg_cbf_nn_update_last_error().decode()}')


def work_bytes(D, batch):
    v = C.c_int64()
    check(D, D.scg_cbf_nn_update_work_bytes(int(batch), C.byref(v)))
    return v.value

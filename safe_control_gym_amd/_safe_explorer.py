"""ctypes binding + builder of libscg_saferoll_<spechash>_<hidden>_<activation>_<Hc>.so (include/scg_safe_explorer.h): the Safe-Explorer
PPO collector — actor, safety layer, projection, sampling and the env step in one launch — compiled per task config, actor shape and
safety-layer width from csrc/scg_safe_explorer.hip.  The library carries every scg_hip.h entry point as well (_lib.EXPORTS):
HipVecEnv(..., policy=(hidden, activation), safety_layer=Hc) drives its handle with it.
No fallback lives here: safe_explorer.py keeps the eager collector, with a warning, for shapes this library does not serve."""
import ctypes as C
import os
import subprocess

from safe_control_gym_amd import _adversarial
from safe_control_gym_amd import _lib as L

SRC = os.path.join(L.CSRC_DIR, 'scg_safe_explorer.hip')
HEADER = os.path.normpath(os.path.join(L.CSRC_DIR, '..', '..', 'include', 'scg_safe_explorer.h'))
# the pre-training kernels (collector + fused constraint-model update) ride in the same library: csrc/scg_safe_pretrain.h + its ABI
PRETRAIN_SRC = os.path.join(L.CSRC_DIR, 'scg_safe_pretrain.h')
PRETRAIN_HEADER = os.path.normpath(os.path.join(L.CSRC_DIR, '..', '..', 'include', 'scg_safe_pretrain.h'))
# the env library's hash inputs (_lib.SOURCES + _lib.HEADERS), the adversarial header the ABI includes, and this library's own files
DEPS = [os.path.join(L.CSRC_DIR, s) for s in L.SOURCES + L.HEADERS] + [_adversarial.HEADER, SRC, HEADER, PRETRAIN_SRC, PRETRAIN_HEADER,
                                                                       os.path.join(L.CSRC_DIR, 'scg_adam.h')]
PREFIX = 'libscg_saferoll_'
LDS_BUDGET = 163840                 # 160 KiB of LDS per CU (MI355X)
MAX_CONSTRAINTS, MAX_HIDDEN_C = 32, 256


def packed_dims(obs_dim, act_dim, hidden_c):
    """(padded hidden width Hp, hidden tiles NT, layer-1 steps Q, words per constraint block) of the packed layer (scg_safe_explorer.h)."""
    hp = (int(hidden_c) + 31) // 32 * 32
    q = 4 * ((int(obs_dim) + 7) // 8)
    return hp, hp // 32, q, (hp // 32) * q * 64 + hp * (1 + int(act_dim)) + 4


def packed_words(obs_dim, act_dim, n_constraints, hidden_c):
    return int(n_constraints) * packed_dims(obs_dim, act_dim, hidden_c)[3]


def lds_bytes(obs_dim, hidden, act_dim, n_constraints, hidden_c, wpw, placement=None):
    """(bytes, waves per workgroup, safety layer in LDS) the launcher uses when asked for `wpw` waves (scg_safe_explorer.hip,
    SafeShape / safe_choose): the actor image, the packed layer when it fits next to it, plus the obs transpose scratch for 16-byte
    rows while it fits next to the actor image at 4 waves; 8 waves drop to 4 when over budget (hidden 128: always 4).
    placement: None (the launcher's choice), 'lds' or 'global' (SCG_SAFE_WEIGHTS).  Waves 0: that placement does not fit."""
    img = 4 * _adversarial._image_words(obs_dim, hidden, act_dim)
    safe = 4 * packed_words(obs_dim, act_dim, n_constraints, hidden_c)
    per_wave = 64 * obs_dim * 4
    xpose = (obs_dim * 4) % 16 == 0 and img + 4 * per_wave <= LDS_BUDGET
    b = lambda w, il: img + (safe if il else 0) + (w * per_wave if xpose else 0)      # noqa: E731

    def used(il):
        for w in ((wpw, 4) if hidden < 128 else (4,)):
            if b(w, il) <= LDS_BUDGET:
                return w
        return 0
    wl, wg = used(True), used(False)
    if placement == 'lds' or (placement != 'global' and wl):
        return b(wl or 4, True), wl, True
    return b(wg or 4, False), wg, False


def placement(obs_dim, hidden, act_dim, n_constraints, hidden_c, wpw=4):
    """'lds', 'global' or None (no fit): where the launcher puts the safety layer."""
    _, w, il = lds_bytes(obs_dim, hidden, act_dim, n_constraints, hidden_c, wpw)
    return None if w == 0 else 'lds' if il else 'global'


def supported(obs_dim, hidden, act_dim, activation, n_constraints, hidden_c):
    """Shapes the fused collector serves: the fused policy rollout's actor shapes, 1..32 constraints, one hidden layer of 1..256."""
    if isinstance(hidden_c, (list, tuple)):
        if len(hidden_c) != 1:
            return False
        hidden_c = hidden_c[0]
    return (L.policy_supported(obs_dim, hidden, act_dim, activation) and 1 <= int(n_constraints) <= MAX_CONSTRAINTS
            and 1 <= int(hidden_c) <= MAX_HIDDEN_C and placement(obs_dim, hidden, act_dim, n_constraints, hidden_c) is not None)


def flat_words(obs_dim, act_dim, hidden_c):
    """P: the float words of ONE constraint model in scg_safety_update's flat layout  W1 [Hc][obs] | b1 [Hc] | W2 [A][Hc] | b2 [A]."""
    return int(hidden_c) * (int(obs_dim) + 1 + int(act_dim)) + int(act_dim)


def pretrain_lds_bytes(obs_dim, act_dim, hidden_c):
    """LDS bytes per workgroup of scg_safety_update (csrc/scg_safe_pretrain.h, PretrainShape): parameters, both Adam moments and the
    gradient of one constraint model, the waves' loss partials, and a chunk of 1024 staged rows (halved while over budget, down to 32)."""
    fixed = 4 * ((flat_words(obs_dim, act_dim, hidden_c) + 3) // 4 * 4) + 16
    roww = int(obs_dim) + int(act_dim) + 1
    rc = 1024
    while rc >= 64 and (fixed + rc * roww) * 4 > LDS_BUDGET:
        rc //= 2
    return (fixed + rc * roww) * 4


def supported_pretrain(obs_dim, act_dim, n_constraints, hidden_c):
    """Shapes scg_collect_constraints / scg_safety_update serve: 1..32 constraints, one hidden layer of 1..256, at most 32 inputs and 4
    actions, and an LDS need within 160 KiB.  (The library itself is compiled per actor shape too: _safe_explorer.supported.)"""
    if isinstance(hidden_c, (list, tuple)):
        if len(hidden_c) != 1:
            return False
        hidden_c = hidden_c[0]
    return (isinstance(hidden_c, int) and 1 <= int(n_constraints) <= MAX_CONSTRAINTS and 1 <= hidden_c <= MAX_HIDDEN_C
            and 1 <= int(act_dim) <= 4 and 1 <= int(obs_dim) <= 32 and pretrain_lds_bytes(obs_dim, act_dim, hidden_c) <= LDS_BUDGET)


class CollectIO(C.Structure):
    """scg_collect_io (include/scg_safe_pretrain.h)."""
    _fields_ = [('d_obs', C.c_void_p), ('d_act', C.c_void_p), ('d_c', C.c_void_p), ('d_c_next', C.c_void_p), ('pos', C.c_int64),
                ('capacity', C.c_int64), ('low', C.c_float * 4), ('high', C.c_float * 4), ('d_c_carry', C.c_void_p),
                ('d_last_obs', C.c_void_p), ('d_ep_stats', C.c_void_p)]


class SafetyUpdateArgs(C.Structure):
    """scg_safety_update_args (include/scg_safe_pretrain.h)."""
    _fields_ = [('d_params', C.c_void_p), ('d_m', C.c_void_p), ('d_v', C.c_void_p), ('d_steps', C.c_void_p), ('d_obs', C.c_void_p),
                ('d_act', C.c_void_p), ('d_c', C.c_void_p), ('d_c_next', C.c_void_p), ('d_rows', C.c_void_p), ('n_batches', C.c_int32),
                ('batch', C.c_int32), ('lr', C.c_float), ('train', C.c_int32), ('d_loss', C.c_void_p), ('d_grad', C.c_void_p)]


def pack_safety_layer(models, obs_dim, act_dim, hidden_c, out=None):
    """The packed float32 layer (scg_safe_explorer.h) of an nn.ModuleList of one-hidden-layer ppo.MLPs (SafetyLayer.constraint_models),
    on their device; `out` (a 1-D float32 tensor of packed_words entries) is filled in place when given."""
    import torch
    hp, nt, q, stride = packed_dims(obs_dim, act_dim, hidden_c)
    n = len(models)
    dev = models[0].fcs[0].weight.device
    W1 = torch.stack([m.fcs[0].weight.detach() for m in models]).to(torch.float32)          # [C][Hc][obs]
    b1 = torch.stack([m.fcs[0].bias.detach() for m in models]).to(torch.float32)            # [C][Hc]
    W2 = torch.stack([m.fcs[1].weight.detach() for m in models]).to(torch.float32)          # [C][A][Hc]
    b2 = torch.stack([m.fcs[1].bias.detach() for m in models]).to(torch.float32)            # [C][A]
    blk = torch.zeros(n, stride, dtype=torch.float32, device=dev)
    # W1f[t][q][lane] = W1[32 t + (lane & 31)][row(q, lane >> 5)], row(q, h) = (q & 3) + 8 (q >> 2) + 4 h; zero outside
    W1p = torch.zeros(n, hp, 8 * (q // 4), dtype=torch.float32, device=dev)
    W1p[:, :hidden_c, :obs_dim] = W1
    lane = torch.arange(64, device=dev)
    qq = torch.arange(q, device=dev)
    rows = (qq[:, None] & 3) + 8 * (qq[:, None] >> 2) + 4 * (lane[None, :] >> 5)                # [q][64]
    feat = 32 * torch.arange(nt, device=dev)[:, None, None] + (lane & 31)[None, None, :]          # [nt][1][64]
    blk[:, :nt * q * 64] = W1p[:, feat.expand(nt, q, 64), rows[None].expand(nt, q, 64)].reshape(n, -1)
    o = nt * q * 64
    blk[:, o:o + hidden_c] = b1
    o += hp
    w2 = torch.zeros(n, act_dim, hp, dtype=torch.float32, device=dev)
    w2[:, :, :hidden_c] = W2
    blk[:, o:o + act_dim * hp] = w2.reshape(n, -1)
    o += act_dim * hp
    blk[:, o:o + act_dim] = b2
    if out is None:
        return blk.reshape(-1).contiguous()
    out.copy_(blk.reshape(-1))
    return out


def source_hash():
    import hashlib
    h = hashlib.sha256()
    for p in DEPS:
        with open(p, 'rb') as f:
            h.update(os.path.basename(p).encode() + b'\0' + f.read())
    return int.from_bytes(h.digest()[:8], 'little')


def lib_path(spec_hash, hidden, activation, hidden_c):
    return os.path.join(L.SPEC_DIR, f'{PREFIX}{spec_hash:016x}_{int(hidden)}_{activation}_{int(hidden_c)}.so')


def build(cfg, hidden, activation, hidden_c, force=False):
    """Compile the collector for this scg_config, actor shape and safety-layer width (hipcc, gfx950)."""
    if activation not in L.POLICY_ACTS or not 1 <= int(hidden_c) <= MAX_HIDDEN_C:
        raise L.ScgError(f'no fused Safe-Explorer rollout for {activation} / safety hidden width {hidden_c}')
    src, h = L.spec_source(cfg)
    hdr, _ = L.spec_paths(h)
    so = lib_path(h, hidden, activation, hidden_c)
    if not force and os.path.exists(so) and L._lib_source_hash(so) == source_hash():
        return so
    os.makedirs(L.SPEC_DIR, exist_ok=True)
    with open(hdr, 'w') as f:
        f.write(src)
    cmd = [L._hipcc(), '--offload-arch=gfx950', '-O3', '-ffp-contract=on', '-std=c++17', '-fPIC', '-shared', '-DSCG_SPEC', '-include', hdr,
           f'-DSCG_POLICY_H={int(hidden)}', f'-DSCG_POLICY_ACT={L.POLICY_ACTS[activation]}', f'-DSCG_SAFE_HC={int(hidden_c)}',
           f'-DSCG_SRC_HASH=0x{source_hash():016x}ULL', '-o', so]
    res = None
    for extra in L.sched_flags(cfg):
        res = subprocess.run(cmd + extra + [SRC], capture_output=True, text=True)
        if res.returncode == 0:
            return so
    raise L.ScgError('hipcc failed (Safe-Explorer rollout build):\n' + res.stdout + res.stderr)


_libs = {}


def lib_for(cfg, hidden, activation, hidden_c):
    """The bound library (every _lib.EXPORTS symbol + scg_rollout_safe + the pre-training entry points), built now if missing or stale."""
    _, h = L.spec_source(cfg)
    key = (h, int(hidden), activation, int(hidden_c))
    if key in _libs:
        return _libs[key]
    so = lib_path(*key)
    if not os.path.exists(so) or L._lib_source_hash(so) != source_hash():
        if not os.path.exists(L._hipcc()):
            raise L.ScgError(f'{so} is missing or stale and hipcc is not available to build it')
        build(cfg, hidden, activation, hidden_c, force=True)
    D = L._bind(so)
    if int(D.scg_spec_hash()) != h:
        raise L.ScgError(f'{so} was built for another config')
    D.scg_rollout_safe.argtypes = [C.c_void_p, C.POINTER(_adversarial.ActorPtrs), C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                   C.POINTER(L.PolicyRollout), C.c_void_p, C.c_void_p, C.c_void_p]
    D.scg_safe_explorer_shape.argtypes = [C.POINTER(C.c_int32)] * 7
    D.scg_safe_explorer_lds.argtypes = [C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    D.scg_collect_constraints.argtypes = [C.c_void_p, C.c_int, C.POINTER(CollectIO), C.c_void_p]
    D.scg_safety_update.argtypes = [C.POINTER(SafetyUpdateArgs), C.c_void_p]
    D.scg_safe_pretrain_lds.argtypes = [C.POINTER(C.c_int32)]
    shape = [C.c_int32() for _ in range(7)]
    D.scg_safe_explorer_shape(*[C.byref(v) for v in shape])
    if tuple(v.value for v in shape[1:4]) != (int(hidden_c), int(hidden), L.POLICY_ACTS[activation]):
        raise L.ScgError(f'{so} was built for another actor / safety-layer shape')
    _libs[key] = D
    return D


def shape_of(D):
    """(C, Hc, hidden, activation id, act_dim, obs_dim, packed words) of a bound library."""
    v = [C.c_int32() for _ in range(7)]
    D.scg_safe_explorer_shape(*[C.byref(x) for x in v])
    return tuple(x.value for x in v)


def pretrain_lds_of(D):
    """LDS bytes per workgroup scg_safety_update uses in this bound library."""
    b = C.c_int32()
    L.check(D.scg_safe_pretrain_lds(C.byref(b)), D)
    return b.value


def launch_plan(D, wpw):
    """(LDS bytes, waves per workgroup, safety layer in LDS) the library's launcher uses for `wpw` (SCG_SAFE_WEIGHTS honoured)."""
    b, w, il = C.c_int32(), C.c_int32(), C.c_int32()
    L.check(D.scg_safe_explorer_lds(int(wpw), C.byref(b), C.byref(w), C.byref(il)), D)
    return b.value, w.value, bool(il.value)

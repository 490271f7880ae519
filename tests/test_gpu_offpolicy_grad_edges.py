"""The fused SAC and DDPG gradient steps (csrc/scg_sac.hip, csrc/scg_ddpg.hip on csrc/scg_wide.h) against the float64 model of
tests/offpolicy_grad_model.py, tensor by tensor, on the edge inputs of tests/offpolicy_grad_cases.py: log_std below, inside and above
its clamp, tanh saturated to +-1, softplus past its threshold, a DDPG actor with 1 - tanh^2 = 0 on part of the batch, an action
interval whose 0.5 (high_j - low_j) differs per action, masked rows, repeated ring rows, and 513 tiles on the 512-workgroup cap.

The reference is NOT the eager float32 update: at the lower clamp that one is off by 1e-3 .. 1e-1 of a tensor
(tests/test_offpolicy_grad_model_cpu.py::test_eager_float32_update_is_no_yardstick_at_the_lower_clamp).

Order: both learners step the actor (SAC: and the temperature) before the critic loss is formed, so the critic half of the reference
takes the stepped actor read back from the fused agent; the critics and targets are the ones saved before the step.  SAC's two halves
are taken with scg_sac_update's phases (ACTOR_GRAD, then CRITIC_GRAD, d_grad read after each); one DDPG step leaves both in d_grad.

Bounds, none derived from what a kernel produced (offpolicy_grad_model.tolerances / loss_tolerance):
  gradient, per tensor t of network k   max |g_fused - g64| <= max(8 d32_k, 8 x 2^-23) x max |g64_t|, d32_k = the float32 run of the
                                        same model against its float64 run on the same batch (CPU), largest over the tensors of k
  losses                                8 x the float32 model's relative deviation, floor 1e-6 relative
  Adam, per element                     |p_after - (p_before - lr g / (|g| + 1e-8))| <= 4 x 2^-23 lr + ulp(p) / 2, in float64 from
                                        the kernel's own g (step 1, zero moments: the bias corrections cancel)
Every test asserts the preconditions of offpolicy_grad_cases.check_preconditions on the reference first and prints d32, the bound and
the achieved deviation per tensor before it asserts.

Measured on the MI355X, kernels as shipped (every tensor of every case inside its bound):
  SAC    worst achieved-to-bound ratio 0.336 (actor.log_std_layer.weight, 16416 rows: deviation 1.8e-7 of a bound of 5.4e-7); the
         other cases 0.09 .. 0.17; losses within 1.8e-7 relative of the float64 model (bound 1e-6)
  DDPG   worst ratio 0.670 (actor.net.fcs.2.bias of the one-float-observation case: 8.5e-9 of 1.27e-8, d32 8.6e-7); the other cases
         0.09 .. 0.26; losses within 2.1e-6 relative where the bound is 8.8e-6 (a policy loss of -0.004), 2.5e-7 elsewhere
  Adam   largest |p_after - expected| / bound 0.996: the half ulp of the parameter's own rounding is most of the bound
"""
import functools

import pytest

from tests import offpolicy_grad_cases as C
from tests import offpolicy_grad_model as M

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


def _ring(c, d):
    from safe_control_gym_amd.offpolicy import DeviceReplay
    r = d['ring']
    buf = DeviceReplay(r['obs'].shape[0], c['obs'], c['act'], torch.device(DEV))
    buf.push(*(r[k].to(DEV) for k in ('obs', 'act', 'rew', 'next_obs', 'mask')))
    return buf


def _fused_sac(c, cpu):
    from safe_control_gym_amd.sac import SACAgent, SACConfig
    low, high = C.bounds(c)
    cfg = SACConfig(hidden_dim=c['hidden'], activation=c['activation'], use_entropy_tuning=True, actor_lr=C.LR, critic_lr=C.LR, entropy_lr=C.LR)
    ag = SACAgent(c['obs'], c['act'], low.to(DEV), high.to(DEV), cfg, torch.device(DEV))
    assert ag.use_fused
    ag.ac.load_state_dict(cpu.ac.state_dict()); ag.ac_targ.load_state_dict(cpu.ac_targ.state_dict())
    assert float(ag.log_alpha.detach()) == float(cpu.log_alpha.detach())
    return ag


def _fused_by_name(ag, flat):
    """{ac-relative tensor name: its slice of the flat vector `flat`, in float64 on the CPU} (+ SAC's log_alpha)."""
    out = {}
    for n, p in ag.ac.named_parameters():
        o = ag._flat_offset(p)
        out[n] = flat[o:o + p.numel()].view_as(p).detach().cpu().double()
    if hasattr(ag, 'log_alpha'):
        out['log_alpha'] = flat[ag._flat['n']].detach().cpu().double()
    return out


def _actor_tensors(ag):
    return {n: p.detach().cpu().clone() for n, p in ag.ac.actor.named_parameters()}


def _check_gradients(what, got, ref):
    """Prints the per-tensor table, then asserts the bound; returns the worst achieved-to-bound ratio."""
    g64, tol, d32 = ref['f64']['grads'], ref['tol'], ref['d32']
    assert set(got) >= set(g64)
    rows, worst = [], 0.0
    for n, want in g64.items():
        dev = float((got[n] - want).abs().max())
        rows.append((n, dev))
        worst = max(worst, dev / tol[n])
        print(f'  {n:32s} max |g64| {float(want.abs().max()):.3e}  d32 {d32[M.network_of(n)]:.2e}  bound {tol[n]:.3e}  fused deviation {dev:.3e}'
              f'  ratio {dev / tol[n]:.3f}')
    print(f'  {what}: worst achieved-to-bound ratio {worst:.3f}')
    for n, dev in rows:
        assert dev <= tol[n], (what, n, dev, tol[n])
    return worst


def _check_losses(what, got, ref):
    for k, v in got.items():
        l64, l32 = ref['f64']['losses'][k], ref['f32']['losses'][k]
        rel = M.loss_tolerance(l64, l32)
        print(f'  {k}: fused {v!r}  float64 {l64!r}  float32 model {l32!r}  relative bound {rel:.2e}  achieved {abs(v - l64) / abs(l64):.2e}')
    for k, v in got.items():
        l64 = ref['f64']['losses'][k]
        assert abs(v - l64) <= M.loss_tolerance(l64, ref['f32']['losses'][k]) * abs(l64), (what, k, v, l64)


def _check_adam(what, before, after, g, lr=C.LR):
    """Every element: Adam's first step from the kernel's own gradient, in float64.  4 float32 places of lr for the step's own float32
    arithmetic (lr / bc1, m, sqrt(v) / sqrt(bc2): one rounding each), half an ulp of the parameter for the final subtraction."""
    worst = 0.0
    for n, p0 in before.items():
        want = M.adam_first_step(p0.double(), g[n], lr)
        ulp = torch.finfo(torch.float32).eps * 2.0 ** torch.floor(torch.log2(torch.maximum(p0.double().abs(), want.abs()).clamp(min=1e-30)))
        bound = 4 * M.ULP32 * lr + 0.5 * ulp
        ratio = float(((after[n].double() - want).abs() / bound).max())
        worst = max(worst, ratio)
        print(f'  adam {n:32s} largest |p_after - expected| / bound {ratio:.3f}')
    assert worst <= 1.0, (what, worst)


@functools.lru_cache(maxsize=None)
def _sac_inputs(name):
    c = C.SAC_CASES[name]
    return c, C.sac_agent(c), C.data(c)


@pytest.mark.parametrize('name', list(C.SAC_CASES))
def test_sac_fused_gradients_losses_and_adam_step(name):
    from safe_control_gym_amd import _sac
    c, cpu, d = _sac_inputs(name)
    ag, buf = _fused_sac(c, cpu), _ring(c, d)
    fl, B = ag._flat, c['batch']
    F = ag._fused_args(buf, B, idx=d['idx'].to(torch.int32).to(DEV), eps=d['eps'].to(DEV).contiguous(), eps_next=d['eps_next'].to(DEV).contiguous())
    before = dict(_actor_tensors(ag), log_alpha=ag.log_alpha.detach().cpu().clone())
    ag._fused_step(F, _sac.ACTOR_GRAD)
    torch.cuda.synchronize()
    got = {n: g for n, g in _fused_by_name(ag, fl['g']).items() if M.network_of(n) in ('actor', 'log_alpha')}
    ag._fused_step(F, _sac.CRITIC_GRAD)                 # the actor / temperature step from d_grad, then the critics' gradient
    torch.cuda.synchronize()
    got.update({n: g for n, g in _fused_by_name(ag, fl['g']).items() if M.network_of(n) in ('q1', 'q2')})
    stepped = (_actor_tensors(ag), ag.log_alpha.detach().cpu().clone())
    ag._fused_step(F, _sac.FINISH)
    torch.cuda.synchronize()
    stats = F['stats'].tolist()
    # ---- the reference and its preconditions; nothing of the kernel's is compared before these hold
    print(f'\nsac {name}')
    ref = C.reference('sac', cpu, d, stepped=stepped)
    C.check_preconditions('sac', c, ref)
    C.report_tolerances(ref)
    _check_gradients(f'sac {name}', got, ref)
    _check_losses(f'sac {name}', dict(zip(('policy_loss', 'critic_loss', 'entropy_loss'), stats[:3])), ref)
    after = dict(stepped[0], log_alpha=stepped[1])
    _check_adam(f'sac {name}', before, after, {n[len('actor.'):] if n != 'log_alpha' else n: g for n, g in got.items()
                                               if M.network_of(n) in ('actor', 'log_alpha')})
    # ---- the whole step in one call (what SACAgent.update_from_buffer captures: the optimiser steps ride in the reductions) leaves
    # the same gradient vector and the same parameters, bit for bit (csrc/scg_adam.h's contract)
    whole = _fused_sac(c, cpu)
    Fw = whole._fused_args(buf, B, idx=d['idx'].to(torch.int32).to(DEV), eps=d['eps'].to(DEV).contiguous(), eps_next=d['eps_next'].to(DEV).contiguous())
    whole._fused_step(Fw)
    torch.cuda.synchronize()
    assert torch.equal(whole._flat['g'], fl['g']) and torch.equal(whole._flat['p'], fl['p']) and torch.equal(whole._flat['targ'], fl['targ'])
    assert Fw['stats'].tolist() == stats


@functools.lru_cache(maxsize=None)
def _ddpg_inputs(name):
    c = C.DDPG_CASES[name]
    return c, C.ddpg_agent(c), C.data(c)


@pytest.mark.parametrize('name', list(C.DDPG_CASES))
def test_ddpg_fused_gradients_losses_and_adam_step(name):
    from safe_control_gym_amd import ddpg
    c, cpu, d = _ddpg_inputs(name)
    low, high = C.bounds(c)
    ag = ddpg.DDPGAgent(c['obs'], c['act'], low.numpy(), high.numpy(),
                        ddpg.DDPGConfig(hidden_dim=c['hidden'], activation=c['activation'], actor_lr=C.LR, critic_lr=C.LR), DEV)
    assert ag.use_fused
    ag.ac.load_state_dict(cpu.ac.state_dict()); ag.ac_targ.load_state_dict(cpu.ac_targ.state_dict())
    buf = _ring(c, d)
    before = _actor_tensors(ag)
    F = ag._fused_args(buf, c['batch'], idx=d['idx'].to(torch.int32).to(DEV))
    ag.fused_step(F)                                    # one step leaves both halves in d_grad
    torch.cuda.synchronize()
    got, stepped, stats = _fused_by_name(ag, ag._flat['g']), _actor_tensors(ag), F['stats'].tolist()
    print(f'\nddpg {name}')
    ref = C.reference('ddpg', cpu, d, stepped=(stepped, None))
    C.check_preconditions('ddpg', c, ref)
    C.report_tolerances(ref)
    _check_gradients(f'ddpg {name}', got, ref)
    _check_losses(f'ddpg {name}', dict(zip(('policy_loss', 'critic_loss'), stats[:2])), ref)
    _check_adam(f'ddpg {name}', before, stepped, {n[len('actor.'):]: g for n, g in got.items() if M.network_of(n) == 'actor'})


def test_sac_rows_with_every_log_std_clamped_give_the_log_std_layer_exactly_nothing():
    """32 rows whose every log_std is clamped (below -20 for actions 0 and 2, above 2 for action 1; tanh saturated on most of the
    upper-clamp entries): torch.clamp's gradient is 0 there, so log_std_layer's gradient is exactly 0.0 — on the reference and on the
    fused path, with no tolerance — and Adam leaves the layer's parameters as they were, bit for bit."""
    c = dict(C.SAC_CASES['relu_3_3_32_b32'])
    cpu, d = C.sac_agent(c), C.data(c)
    with torch.no_grad():
        cpu.ac.actor.log_std_layer.weight.mul_(0.25)            # raw log_std: standard deviation 3 around the biases
        cpu.ac.actor.log_std_layer.bias.copy_(torch.tensor([-40.0, 14.0, -40.0]))
    cpu.ac_targ.load_state_dict(cpu.ac.state_dict())
    m = M.SACModel(cpu)
    pol = m.policy(d['batch'], d['eps'])
    raw, u = pol['inter']['obs/raw_log_std'], pol['inter']['obs/u']
    print(f'\nraw log_std per action: min {raw.min(0).values.tolist()} max {raw.max(0).values.tolist()}; |u| > 10 on '
          f'{int((u[:, 1].abs() > 10).sum())} of {u.shape[0]} upper-clamp entries')
    assert bool(((raw < -20.0 - C.CLAMP_GUARD) | (raw > 2.0 + C.CLAMP_GUARD)).all()) and bool((raw[:, 1] > 2).all()) and bool((raw[:, 0] < -20).all())
    assert int((u[:, 1].abs() > 10).sum()) >= 2
    for n in ('actor.log_std_layer.weight', 'actor.log_std_layer.bias'):
        assert bool((pol['grads'][n] == 0.0).all())
    assert float(pol['grads']['actor.mu_layer.weight'].abs().max()) > 0
    ag, buf = _fused_sac(c, cpu), _ring(c, d)
    head = ag.ac.actor.log_std_layer
    w0, b0 = head.weight.detach().clone(), head.bias.detach().clone()
    F = ag._fused_args(buf, c['batch'], idx=d['idx'].to(torch.int32).to(DEV), eps=d['eps'].to(DEV).contiguous(), eps_next=d['eps_next'].to(DEV).contiguous())
    ag._fused_step(F)
    torch.cuda.synchronize()
    got = _fused_by_name(ag, ag._flat['g'])
    for n in ('actor.log_std_layer.weight', 'actor.log_std_layer.bias'):
        assert bool((got[n] == 0.0).all()), (n, got[n])
    assert float(got['actor.mu_layer.weight'].abs().max()) > 0
    assert torch.equal(head.weight.detach(), w0) and torch.equal(head.bias.detach(), b0)

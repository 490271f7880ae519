"""Edge inputs of the fused SAC / DDPG gradient tests: the case tables, the recipes that push the actors' heads off the easy regime,
the ring data, the float64 / float32 reference run of one case and the preconditions every case must meet ON THE REFERENCE, before a
test looks at a kernel.  Plain PyTorch on the CPU (tests/offpolicy_grad_model.py); imported by tests/test_offpolicy_grad_model_cpu.py
and tests/test_gpu_offpolicy_grad_edges.py.

Default-initialised networks on randn observations never leave the easy regime: raw log_std in about [-1, 1], |u| in the single
digits, pre-tanh DDPG outputs below 1.  The recipes rescale the head layers so that every branch of the heads fires on a sizeable
share of the batch:
  SAC   log_std_layer.weight scaled to a raw log_std of standard deviation `ls_std` (12) around a bias of -9, mu_layer.weight to a mean
        of standard deviation `mu_std` (6): log_std below -20, above 2 and inside; tanh saturated to exactly +-1 in float32 (|u| > 10);
        softplus(-2u) past its threshold (-2u > 20)
  DDPG  the actor's last layer scaled to a pre-tanh output of standard deviation `z_std`: 1 - tanh^2 exactly 0 in float32 (|z| > 9)
        next to the steep part (|z| < 1)
Seeds (and, where a shape needs it, factors) were chosen on the CPU so that the reference alone meets check_preconditions():
  * `q_scale` multiplies the last layer of every critic.  The 16416-row SAC case has it because min |q1 - q2| >= 1e-4 over 16416
    rows needs a wider spread of q1 - q2 than default-initialised critics have (about 0.1: some 13 rows inside the guard band on
    average); the three- and four-action SAC cases because default-initialised critics' dq/da is so small next to the entropy
    term that a wrong 0.5 (high_j - low_j) moved no tensor by much more than 100 x its bound (28 x and 148 x without the factor);
  * the 16416-row batches draw from a ring of 4096 rows: raw log_std is a function of the ring row, and 4096 rows leave a seed that
    keeps every one of them 1e-3 away from the clamp's edges.
"""
import math

import torch

from tests import offpolicy_grad_model as M

LOW, HIGH = [-1.0, 0.0, -0.5, 0.1], [1.0, 2.0, 0.5, 0.3]           # the action interval of every case: [:act]
LR = 1e-3

# name -> (obs, act, hidden, activation, batch): shapes the suite already builds, + the seed / factors chosen on the CPU
SAC_CASES = {
    'tanh_17_2_96_b160': dict(obs=17, act=2, hidden=96, activation='tanh', batch=160, seed=3),
    'tanh_1_1_32_b96': dict(obs=1, act=1, hidden=32, activation='tanh', batch=96, seed=12),
    'leaky_27_4_64_b64': dict(obs=27, act=4, hidden=64, activation='leaky_relu', batch=64, seed=5, q_scale=30.0),
    'relu_7_1_96_b96': dict(obs=7, act=1, hidden=96, activation='relu', batch=96, seed=1),
    'relu_3_3_32_b32': dict(obs=3, act=3, hidden=32, activation='relu', batch=32, seed=1, q_scale=100.0),
    # 513 tiles on the 512-workgroup cap: the multi-tile loops
    'tanh_17_2_96_b16416': dict(obs=17, act=2, hidden=96, activation='tanh', batch=16416, seed=16, ring=4096, q_scale=100.0),
}
DDPG_CASES = {
    'tanh_17_3_96_b160': dict(obs=17, act=3, hidden=96, activation='tanh', batch=160, seed=4),
    'tanh_1_1_32_b96': dict(obs=1, act=1, hidden=32, activation='tanh', batch=96, seed=0, z_std=8.0),
    'leaky_27_4_64_b64': dict(obs=27, act=4, hidden=64, activation='leaky_relu', batch=64, seed=1),
    'relu_7_1_96_b96': dict(obs=7, act=1, hidden=96, activation='relu', batch=96, seed=5),
    'tanh_17_3_96_b16416': dict(obs=17, act=3, hidden=96, activation='tanh', batch=16416, seed=0, ring=4096),
}

MIN_SHARE, MIN_ENTRIES = 0.02, 2            # every branch: at least 2 % of the batch x act entries, and 2 entries
CLAMP_GUARD = 1e-3                          # no raw log_std closer to -20 or 2
MIN_GUARD = 1e-4                            # min |q1 - q2|: a flipped min is not round-off
KINK_FACTOR = 8                             # no pre-activation of a relu / leaky_relu closer to 0 than 8 x its float32-vs-float64 difference


def bounds(c):
    return torch.tensor(LOW[:c['act']]), torch.tensor(HIGH[:c['act']])


def wrong_variants(learner, c):
    """The deliberately wrong variants that CAN differ from the truth on this case.  0.5 (high_j - low_j) is 1 for the first two
    actions of the interval above, so `unit_action_scale` is the true gradient unless the case has a third action."""
    names = ['mask_ignored', 'row_dropped'] + (['clamp_passes_gradient', 'no_log_std_term'] if learner == 'sac' else [])
    if any(0.5 * (h - l) != 1.0 for l, h in zip(LOW[:c['act']], HIGH[:c['act']])):
        names.append('unit_action_scale')
    return names


def _scale_to(layer, x, std, bias=None):
    """Scale layer.weight so that layer(x) - bias has standard deviation `std` over the rows of x; optionally set the bias."""
    with torch.no_grad():
        y = torch.nn.functional.linear(x, layer.weight)
        layer.weight.mul_(std / float(y.std()))
        if bias is not None:
            layer.bias.fill_(bias)


def sac_agent(c):
    """The eager CPU agent of a case (entropy tuning on) with the head recipe applied; float32, as the fused agent will hold it."""
    from safe_control_gym_amd.sac import SACAgent, SACConfig
    torch.manual_seed(1000 + c['seed'])
    low, high = bounds(c)
    cfg = SACConfig(hidden_dim=c['hidden'], activation=c['activation'], use_entropy_tuning=True, actor_lr=LR, critic_lr=LR, entropy_lr=LR,
                    extra={'cuda_graphs': False})
    ag = SACAgent(c['obs'], c['act'], low, high, cfg, 'cpu')
    a = ag.ac.actor
    with torch.no_grad():
        h = a.net(torch.randn(4096, c['obs'], generator=torch.Generator().manual_seed(2000 + c['seed'])))
    _scale_to(a.log_std_layer, h, c.get('ls_std', 12.0), bias=-9.0)
    _scale_to(a.mu_layer, h, c.get('mu_std', 6.0))
    s = c.get('q_scale')
    if s:
        with torch.no_grad():
            for q in (ag.ac.q1, ag.ac.q2):
                q.q_net.fcs[2].weight.mul_(s)
                q.q_net.fcs[2].bias.mul_(s)
    ag.ac_targ.load_state_dict(ag.ac.state_dict())
    return ag


def ddpg_agent(c):
    from safe_control_gym_amd import ddpg
    torch.manual_seed(1000 + c['seed'])
    low, high = bounds(c)
    cfg = ddpg.DDPGConfig(hidden_dim=c['hidden'], activation=c['activation'], actor_lr=LR, critic_lr=LR, extra={'fused_update': False})
    ag = ddpg.DDPGAgent(c['obs'], c['act'], low.numpy(), high.numpy(), cfg, 'cpu')
    net = ag.ac.actor.net
    with torch.no_grad():
        x = torch.randn(4096, c['obs'], generator=torch.Generator().manual_seed(2000 + c['seed']))
        for fc in net.fcs[:-1]:
            x = net.act(fc(x))
    _scale_to(net.fcs[-1], x, c.get('z_std', 4.0))
    ag.ac_targ.load_state_dict(ag.ac.state_dict())
    return ag


def data(c):
    """Ring columns, the index vector (repeated rows), the minibatch it selects and the head's noise, as float32 CPU tensors."""
    B, nobs, nu = c['batch'], c['obs'], c['act']
    n = c.get('ring', 3 * B // 4)
    g = torch.Generator().manual_seed(3000 + c['seed'])
    low, high = bounds(c)
    ring = {'obs': torch.randn(n, nobs, generator=g), 'act': torch.rand(n, nu, generator=g) * (high - low) + low,
            'rew': torch.randn(n, 1, generator=g), 'next_obs': torch.randn(n, nobs, generator=g),
            'mask': (torch.rand(n, 1, generator=g) > 0.3).float()}
    idx = torch.randint(0, n, (B,), generator=g)
    assert len(set(idx.tolist())) < B and 0.2 < 1.0 - float(ring['mask'].mean()) < 0.4
    return {'ring': ring, 'idx': idx, 'batch': {k: v[idx] for k, v in ring.items()},
            'eps': torch.randn(B, nu, generator=g), 'eps_next': torch.randn(B, nu, generator=g)}


# ---------------------------------------------------------------------------------------------------------------- the reference run
def _merge(*parts):
    out = {'grads': {}, 'losses': {}, 'inter': {}}
    for p in parts:
        for k in out:
            out[k].update(p[k])
    return out


def stepped_actor(model32, g32, lr=LR):
    """The actor (and SAC's temperature) after Adam's first step in float32 — what a test without a GPU uses in place of the
    parameters the fused step leaves behind."""
    f = torch.float32
    out = {n: M.adam_first_step(p.detach().to(f), g32['actor.' + n].to(f), lr) for n, p in model32.ac.actor.named_parameters()}
    la = None
    if 'log_alpha' in g32:
        la = M.adam_first_step(model32.log_alpha.detach().to(f), g32['log_alpha'].to(f), lr)
    return out, la


def reference(learner, agent, d, stepped=None, wrong=None):
    """The restated model in float64 and float32 on one case: gradients per tensor, losses, intermediates, the tolerances.
    stepped: (actor tensors {name: tensor}, log_alpha or None) after the actor step; None: stepped_actor() of the float32 model."""
    models = [(M.SACModel if learner == 'sac' else M.DDPGModel)(agent, t) for t in (torch.float64, torch.float32)]
    noise = ([d['eps']], [d['eps_next']]) if learner == 'sac' else ([], [])
    pol = [m.policy(d['batch'], *noise[0], wrong=wrong) for m in models]
    if stepped is None:
        stepped = stepped_actor(models[1], pol[1]['grads'])
    for m in models:
        m.set_actor(*(stepped if learner == 'sac' else stepped[:1]))
    cri = [m.critic(d['batch'], *noise[1], wrong=wrong) for m in models]
    r64, r32 = _merge(pol[0], cri[0]), _merge(pol[1], cri[1])
    tol, d32 = M.tolerances(r64['grads'], r32['grads'])
    return {'f64': r64, 'f32': r32, 'tol': tol, 'd32': d32, 'stepped': stepped}


# ---------------------------------------------------------------------------------------------------------------- preconditions
def branches(learner, inter, tag):
    if learner == 'sac':
        raw, u = inter[tag + '/raw_log_std'], inter[tag + '/u']
        return {'log_std < -20': raw < M.LOG_STD_MIN, 'log_std > 2': raw > M.LOG_STD_MAX,
                '-20 < log_std < 2': (raw > M.LOG_STD_MIN) & (raw < M.LOG_STD_MAX), '|u| > 10': u.abs() > 10.0, '-2u > 20': -2.0 * u > 20.0}
    z = inter[tag + '/z']
    return {'|z| > 9': z.abs() > 9.0, '|z| < 1': z.abs() < 1.0}


def check_preconditions(learner, c, ref, report=print):
    """Asserts the guards on the float64 reference (and prints every figure); returns them."""
    i64, i32 = ref['f64']['inter'], ref['f32']['inter']
    out = {}
    for tag in ('obs', 'next_obs'):
        for name, mask in branches(learner, i64, tag).items():
            n, total = int(mask.sum()), mask.numel()
            out[f'{tag}: {name}'] = n / total
            report(f'  {tag:8s} {name:18s} {n:6d} of {total} entries ({100.0 * n / total:.1f} %)')
            assert n >= max(MIN_ENTRIES, math.ceil(MIN_SHARE * total)), (tag, name, n, total)
        if learner == 'sac':
            raw = i64[tag + '/raw_log_std']
            dist = float(torch.minimum((raw - M.LOG_STD_MIN).abs(), (raw - M.LOG_STD_MAX).abs()).min())
            gap = float(i64[tag + '/q1_minus_q2'].abs().min())
            out[f'{tag}: clamp distance'], out[f'{tag}: min |q1 - q2|'] = dist, gap
            report(f'  {tag:8s} nearest raw log_std to a clamp edge {dist:.2e} (>= {CLAMP_GUARD:.0e})   min |q1 - q2| {gap:.2e} (>= {MIN_GUARD:.0e})')
            assert dist >= CLAMP_GUARD and gap >= MIN_GUARD, (tag, dist, gap)
    diff, small = M.max_pre_activation_difference(i64, i32), M.min_pre_activation(i64)
    out['pre-activation f32-vs-f64'], out['min |pre-activation|'] = diff, small
    kinked = c['activation'] in ('relu', 'leaky_relu')
    report(f'  largest float32-vs-float64 pre-activation difference {diff:.2e}; smallest |pre-activation| {small:.2e}'
           + (f' (>= {KINK_FACTOR} x the difference = {KINK_FACTOR * diff:.2e})' if kinked else ' (tanh: no kink to guard)'))
    if kinked:
        assert small >= KINK_FACTOR * diff, (small, diff)
    return out


def report_tolerances(ref, report=print):
    report('  d32 per network: ' + ', '.join(f'{k} {v:.2e}' for k, v in ref['d32'].items()))
    for k in ref['f64']['losses']:
        a, b = ref['f64']['losses'][k], ref['f32']['losses'][k]
        report(f'  {k}: float64 {a!r}  float32 {b!r}  relative deviation {abs(a - b) / abs(a):.2e}')

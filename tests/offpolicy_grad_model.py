"""Float64 restatement of the off-policy learners' losses (SACAgent.policy_loss / q_loss, DDPGAgent.compute_policy_loss /
compute_q_loss) for the gradient tests of the fused steps: plain PyTorch on the CPU, no kernel.

What the restatement adds to the agents' own methods:
  * the noise of the tanh-Gaussian head is an ARGUMENT (`eps`, `eps_next`: the tensors a test hands the kernel as d_eps_in /
    d_eps_next_in), and the head is written out with z = eps (see tanh_gaussian_head), so that it stays exact where log_std sits at
    its lower clamp — the eager float32 MLPActor.forward does not (tests/test_offpolicy_grad_model_cpu.py shows it);
  * the critic half takes the actor (and SAC's temperature) AFTER the actor step: both learners step the actor before the critic
    loss is formed (SACAgent.update, DDPGAgent.update), so the critic gradient is a function of the stepped actor.  A test reads that
    actor back from the fused agent (`set_actor`), which keeps Adam's sign-like first step — a whole lr apart between float32 and
    float64 where |g| ~ 1e-8 — out of the gradient comparison;
  * everything a test has to guard is returned: raw log_std, u, the pre-activations in front of every activation, q1 - q2;
  * `wrong=`: deliberately wrong variants (WRONG) that the CPU tests use to show that the edge inputs would expose such a kernel.

The same code runs in float32 (dtype=torch.float32): its deviation from the float64 run is the round-off yardstick `d32` of the
tolerance rule (tolerances()).
"""
import copy
import math
from collections import OrderedDict

import torch
import torch.nn.functional as F

LOG2 = math.log(2.0)
LOG_SQRT_2PI = 0.5 * math.log(2.0 * math.pi)
LOG_STD_MIN, LOG_STD_MAX = -20.0, 2.0
ULP32 = 2.0 ** -23

# the deliberately wrong variants: name -> what a kernel with that mistake would compute
WRONG = {
    'clamp_passes_gradient': "torch.clamp's gradient let through on clamped log_std entries",
    'unit_action_scale': 'the factor 0.5 (high_j - low_j) of the action map replaced by 1 in the backward pass',
    'mask_ignored': 'mask taken as 1 in the bootstrap target',
    'no_log_std_term': 'the -log_std term dropped from log pi',
    'row_dropped': 'the last row of the batch (past 512 tiles: the tile that wraps around) left out of the mean',
}


def _mlp(fcs, act, x, pre):
    """MLP.forward (ppo.py) with the pre-activation in front of every activation appended to `pre`."""
    for fc in fcs[:-1]:
        z = F.linear(x, fc.weight, fc.bias)
        pre.append(z.detach())
        x = act(z)
    return F.linear(x, fcs[-1].weight, fcs[-1].bias)


def _rescale(t, low, high, wrong):
    a = low + 0.5 * (t + 1.0) * (high - low)
    if wrong == 'unit_action_scale':            # the value of the true map, the gradient of a = t
        a = a.detach() + (t - t.detach())
    return a


def _mean(x, wrong):
    """x.mean() over the batch rows (x: [B, 1]).
    row_dropped leaves out the last row — or, where the batch has more 32-row tiles than the kernels have workgroups (512), the tile
    that wraps around.  One row of 16416 is 6e-5 of a mean: 100 x the gradient bound is out of its reach on any input (the floor alone,
    100 x 8 x 2^-23, is 9.5e-5, and a float32 sum of that length deviates by up to 6e-6 on some hosts), so what the 16416-row cases
    are there to catch — the 513th tile lost — is what the variant drops there; single rows are covered by the small batches."""
    if wrong != 'row_dropped':
        return x.mean()
    k = 32 if x.shape[0] > 512 * 32 else 1
    return x[:-k].sum() / x.shape[0]


def tanh_gaussian_head(mu, raw, eps, low, high, wrong=None):
    """MLPActor.forward of sac.py past its two head layers: action, log pi, u.
    sac.py:55 forms z = (u - mu) exp(-log_std) with u = mu + exp(log_std) eps: that IS eps, and it is written as eps here (as in
    the kernel's squash()).  In floating point the two differ: at log_std = -20 and |mu| ~ 10 the subtraction u - mu cancels
    completely in float32."""
    ls = torch.clamp(raw, LOG_STD_MIN, LOG_STD_MAX)
    if wrong == 'clamp_passes_gradient':
        ls = raw + (ls - raw).detach()
    u = mu + torch.exp(ls) * eps
    z = eps
    gauss = -0.5 * z * z - LOG_SQRT_2PI
    if wrong != 'no_log_std_term':
        gauss = gauss - ls
    logp = gauss.sum(-1, keepdim=True) - (2 * (LOG2 - u - F.softplus(-2 * u))).sum(dim=1, keepdim=True)
    return _rescale(torch.tanh(u), low, high, wrong), logp, u


def _grads(loss, named):
    g = torch.autograd.grad(loss, [p for _, p in named], allow_unused=True)
    return OrderedDict((n, (torch.zeros_like(p) if x is None else x).detach().double()) for (n, p), x in zip(named, g))


def adam_first_step(p, g, lr, eps=1e-8):
    """torch.optim.Adam's step 1 from zero moments: m_hat = g, v_hat = g^2 (the bias corrections cancel), p - lr g / (|g| + eps),
    in the dtype of the arguments."""
    return p - lr * g / (g.abs() + eps)


class SACModel:
    """The restated SAC losses on deep copies of `agent`'s modules (bounds buffers included) and log_alpha, cast to `dtype`."""
    NETWORKS = ('actor', 'log_alpha', 'q1', 'q2')

    def __init__(self, agent, dtype=torch.float64):
        self.dtype = dtype
        self.ac = copy.deepcopy(agent.ac).cpu().to(dtype)
        self.targ = copy.deepcopy(agent.ac_targ).cpu().to(dtype)
        for p in self.ac.parameters():
            p.requires_grad_(True)
        self.log_alpha = agent.log_alpha.detach().cpu().clone().to(dtype).requires_grad_(True)
        self.gamma, self.target_entropy, self.tuning = float(agent.cfg.gamma), float(agent.target_entropy), bool(agent.cfg.use_entropy_tuning)

    def set_actor(self, tensors, log_alpha=None):
        """The actor's parameters {name within ac.actor: tensor} (and the temperature) after the actor step, cast to the model's dtype."""
        with torch.no_grad():
            own = dict(self.ac.actor.named_parameters())
            assert set(own) == set(tensors)
            for n, t in tensors.items():
                own[n].copy_(t.detach().cpu().to(self.dtype))
            if log_alpha is not None:
                self.log_alpha.copy_(torch.as_tensor(log_alpha).detach().cpu().to(self.dtype).reshape(()))

    def _actor(self, obs, eps, wrong, inter, tag):
        a, pre = self.ac.actor, []
        h = _mlp(a.net.fcs, a.net.act, obs, pre)        # (upstream's trunk: no activation behind its last layer)
        raw = a.log_std_layer(h)
        act, logp, u = tanh_gaussian_head(a.mu_layer(h), raw, eps, a.low, a.high, wrong)
        inter[tag + '/raw_log_std'] = raw.detach()
        inter[tag + '/u'] = u.detach()
        inter[tag + '/pre/actor'] = pre
        return act, logp

    @staticmethod
    def _q(q, obs, act, inter, key):
        pre = []
        out = _mlp(q.q_net.fcs, q.q_net.act, torch.cat([obs, act], dim=-1), pre)
        inter[key] = pre
        return out

    def _batch(self, batch):
        return {k: v.detach().cpu().to(self.dtype) for k, v in batch.items()}

    def policy(self, batch, eps, wrong=None):
        """SACAgent.policy_loss: {'grads': {ac-relative name: d policy_loss / d tensor} + 'log_alpha': d entropy_loss / d log_alpha,
        'losses', 'inter'}."""
        b, inter = self._batch(batch), {}
        obs = b['obs']
        act, logp = self._actor(obs, eps.detach().cpu().to(self.dtype), wrong, inter, 'obs')
        q1, q2 = self._q(self.ac.q1, obs, act, inter, 'obs/pre/q1'), self._q(self.ac.q2, obs, act, inter, 'obs/pre/q2')
        inter['obs/q1_minus_q2'] = (q1 - q2).detach()
        policy_loss = _mean(self.log_alpha.exp().detach() * logp - torch.min(q1, q2), wrong)
        entropy_loss = -_mean(self.log_alpha * (logp + self.target_entropy).detach(), wrong) if self.tuning else None
        grads = _grads(policy_loss, [('actor.' + n, p) for n, p in self.ac.actor.named_parameters()])
        losses = {'policy_loss': float(policy_loss.detach())}
        if self.tuning:
            grads['log_alpha'] = torch.autograd.grad(entropy_loss, [self.log_alpha])[0].detach().double()
            losses['entropy_loss'] = float(entropy_loss.detach())
        return {'grads': grads, 'losses': losses, 'inter': inter}

    def critic(self, batch, eps_next, wrong=None):
        """SACAgent.q_loss with the model's CURRENT actor and temperature (set_actor: the stepped ones)."""
        b, inter = self._batch(batch), {}
        obs, act, rew, next_obs, mask = b['obs'], b['act'], b['rew'], b['next_obs'], b['mask']
        q1, q2 = self._q(self.ac.q1, obs, act, inter, 'critic/pre/q1'), self._q(self.ac.q2, obs, act, inter, 'critic/pre/q2')
        with torch.no_grad():
            next_act, next_logp = self._actor(next_obs, eps_next.detach().cpu().to(self.dtype), wrong, inter, 'next_obs')
            t1 = self._q(self.targ.q1, next_obs, next_act, inter, 'next_obs/pre/q1_targ')
            t2 = self._q(self.targ.q2, next_obs, next_act, inter, 'next_obs/pre/q2_targ')
            inter['next_obs/q1_minus_q2'] = t1 - t2
            if wrong == 'mask_ignored':
                mask = torch.ones_like(mask)
            q_targ = rew + self.gamma * mask * (torch.min(t1, t2) - self.log_alpha.exp() * next_logp)
        critic_loss = _mean((q1 - q_targ).pow(2), wrong) + _mean((q2 - q_targ).pow(2), wrong)
        named = [(k + '.' + n, p) for k in ('q1', 'q2') for n, p in getattr(self.ac, k).named_parameters()]
        return {'grads': _grads(critic_loss, named), 'losses': {'critic_loss': float(critic_loss.detach())}, 'inter': inter}


class DDPGModel:
    """The restated DDPG losses; MLPActor.low / high are plain attributes there (no buffers): cast by hand."""
    NETWORKS = ('actor', 'q')

    def __init__(self, agent, dtype=torch.float64):
        self.dtype = dtype
        self.ac = copy.deepcopy(agent.ac).cpu().to(dtype)
        self.targ = copy.deepcopy(agent.ac_targ).cpu().to(dtype)
        for p in self.ac.parameters():
            p.requires_grad_(True)
        self.low = torch.as_tensor(agent.ac.actor.low).detach().cpu().to(dtype)
        self.high = torch.as_tensor(agent.ac.actor.high).detach().cpu().to(dtype)
        self.gamma = float(agent.cfg.gamma)

    def set_actor(self, tensors):
        with torch.no_grad():
            own = dict(self.ac.actor.named_parameters())
            assert set(own) == set(tensors)
            for n, t in tensors.items():
                own[n].copy_(t.detach().cpu().to(self.dtype))

    def _actor(self, obs, wrong, inter, tag):
        pre = []
        z = _mlp(self.ac.actor.net.fcs, self.ac.actor.net.act, obs, pre)
        inter[tag + '/z'] = z.detach()
        inter[tag + '/pre/actor'] = pre
        return _rescale(torch.tanh(z), self.low, self.high, wrong)

    _q = staticmethod(SACModel._q)
    _batch = SACModel._batch

    def policy(self, batch, wrong=None):
        b, inter = self._batch(batch), {}
        obs = b['obs']
        policy_loss = -_mean(self._q(self.ac.q, obs, self._actor(obs, wrong, inter, 'obs'), inter, 'obs/pre/q'), wrong)
        grads = _grads(policy_loss, [('actor.' + n, p) for n, p in self.ac.actor.named_parameters()])
        return {'grads': grads, 'losses': {'policy_loss': float(policy_loss.detach())}, 'inter': inter}

    def critic(self, batch, wrong=None):
        b, inter = self._batch(batch), {}
        obs, act, rew, next_obs, mask = b['obs'], b['act'], b['rew'], b['next_obs'], b['mask']
        q = self._q(self.ac.q, obs, act, inter, 'critic/pre/q')
        with torch.no_grad():
            if wrong == 'mask_ignored':
                mask = torch.ones_like(mask)
            nq = self._q(self.targ.q, next_obs, self._actor(next_obs, wrong, inter, 'next_obs'), inter, 'next_obs/pre/q_targ')
            q_targ = rew + self.gamma * mask * nq
        critic_loss = _mean((q - q_targ).pow(2), wrong)
        grads = _grads(critic_loss, [('q.' + n, p) for n, p in self.ac.q.named_parameters()])
        return {'grads': grads, 'losses': {'critic_loss': float(critic_loss.detach())}, 'inter': inter}


# ---------------------------------------------------------------------------------------------------------------- the tolerance rule
def network_of(name):
    return name.split('.', 1)[0]


def tolerances(g64, g32):
    """Per tensor t of network k: max(8 d32_k, 8 x 2^-23) x max |g64_t|, d32_k = the largest, over the tensors of network k, of
    max |g32 - g64| / max |g64|.  tests/test_gpu_cbf_nn_update.py's rule (4 x the float32 model's deviation: another float32
    summation order of the same length; floor of a few float32 places) with the factor doubled: the actor's gradient passes through
    two networks' backward passes, and the device's tanhf / expf / log1pf are not the host's.
    Returns ({name: absolute bound}, {network: d32})."""
    d32 = {}
    for n, ref in g64.items():
        big = float(ref.abs().max())
        dev = float((g32[n] - ref).abs().max())
        d32[network_of(n)] = max(d32.get(network_of(n), 0.0), dev / big if big > 0 else 0.0)
    return {n: max(8 * d32[network_of(n)], 8 * ULP32) * float(ref.abs().max()) for n, ref in g64.items()}, d32


def loss_tolerance(l64, l32):
    """Relative: 8 x the float32 model's relative deviation from the float64 model, floor 1e-6."""
    return max(8 * abs(l32 - l64) / abs(l64), 1e-6)


def max_pre_activation_difference(inter64, inter32):
    """Largest |float32 - float64| over all recorded pre-activations of one pass pair."""
    worst = 0.0
    for k, pre in inter64.items():
        if '/pre/' in k:
            for a, b in zip(pre, inter32[k]):
                worst = max(worst, float((a - b.double()).abs().max()))
    return worst


def min_pre_activation(inter):
    return min(float(z.abs().min()) for k, pre in inter.items() if '/pre/' in k for z in pre)

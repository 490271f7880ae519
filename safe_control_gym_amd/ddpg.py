"""DDPG on the HIP rollout engine.

Mirrors the reference's DDPG (paths relative to safe_control_gym/controllers/ddpg and math_and_models):
  ddpg_utils.py:16-121   DDPGAgent.update: actor step on -q(obs, actor(obs)).mean(), then the critic step on
                         (q(obs, act) - y)^2 .mean() with y = rew + gamma mask q_targ(next_obs, actor(next_obs)) — the target
                         action comes from the ONLINE, just-updated actor (upstream's choice, kept) — then soft_update over
                         ALL parameters (sac_utils.py:421-424); two torch-default Adam optimisers
  ddpg_utils.py:126-175  actor MLP(obs, act_dim, [H, H]) with both hidden layers activated, tanh, rescaled to [low, high];
                         critic MLP(obs + act, 1, [H, H])
  ddpg.py:271-341        train_step: uniform actions during warm-up, then ac.act(obs) + noise, one sample() of the noise
                         process per env in env order; the noisy, unclipped action is stored; time-limit fix-up as SAC's
  random_processes.py, schedule.py   OrnsteinUhlenbeckProcess (theta 0.15, dt 1e-2) / GaussianProcess, LinearSchedule std

Deviation: upstream's make_action_noise_process resolves the YAML's class names with eval() inside ddpg_utils.py, which imports
neither LinearSchedule nor OrnsteinUhlenbeckProcess — DDPG(...) with its own default config raises NameError there.  This module
implements the intent: the classes the YAML names, from math_and_models (restated below).

MI355X-first differences (as sac.py): the replay ring lives in HBM and is filled on the device; on a single GPU the whole
gradient step is the fused library (csrc/scg_ddpg.hip) replayed as a HIP graph, and a vector step of the collector is three
library launches + the env kernel, the noise process continued across the env batch on the device (an affine scan in float64).
With several updates owed per vector step, `_since_update` / extra['updates_per_step'] work as in sac.py.

What DDPG shares with SAC — the replay ring, the flat-parameter bookkeeping, the collectors, train_step / learn and the checkpoint
format — lives in offpolicy.py (FlatAgent, OffPolicyTrainer); this module holds the noise processes, the networks, the config, the
losses, the update paths and the hooks in which DDPG differs.
"""
import warnings
from copy import deepcopy
from dataclasses import dataclass, field

import numpy as np
import torch
import torch.nn as nn

from safe_control_gym_amd import parallel
from safe_control_gym_amd.offpolicy import DeviceReplay, FlatAgent, OffPolicyConfig, OffPolicyTrainer  # noqa: F401 (DeviceReplay: re-exported)
from safe_control_gym_amd.ppo import MLP
from safe_control_gym_amd.sac import MLPQFunction


# ---------------------------------------------------------------------------------------------------------------- noise
class LinearSchedule:
    """schedule.py:LinearSchedule — the value advances once per call."""

    def __init__(self, start, end=None, steps=None):
        if end is None:
            end, steps = start, 1
        self.start, self.end = start, end
        self.inc = (end - start) / float(steps)
        self.current = start
        self.bound = min if end > start else max

    def __call__(self, steps=1):
        val = self.current
        self.current = self.bound(self.current + self.inc * steps, self.end)
        return val

    def state_dict(self):
        return {'current': self.current}

    def load_state_dict(self, state):
        self.current = state['current']


class GaussianProcess:
    """random_processes.py:GaussianProcess.  `randn(*size)` supplies the draws (np.random.randn, as upstream, by default)."""

    def __init__(self, size, std, randn=None):
        self.size, self.std = tuple(size), std
        self.randn = randn or np.random.randn

    def sample(self):
        return self.randn(*self.size) * self.std()

    def reset_states(self):
        pass

    def state_dict(self):
        return {}

    def load_state_dict(self, state):
        pass


class OrnsteinUhlenbeckProcess:
    """random_processes.py:OrnsteinUhlenbeckProcess: x <- x + theta (mu - x) dt + std() sqrt(dt) eps, mu = 0."""

    def __init__(self, size, std, theta=.15, dt=1e-2, x0=None, randn=None):
        self.theta, self.mu, self.std, self.dt, self.x0, self.size = theta, 0, std, dt, x0, tuple(size)
        self.randn = randn or np.random.randn
        self.reset_states()

    def sample(self):
        x = self.x_prev + self.theta * (self.mu - self.x_prev) * self.dt + self.std() * np.sqrt(self.dt) * self.randn(*self.size)
        self.x_prev = x
        return x

    def reset_states(self):
        self.x_prev = self.x0 if self.x0 is not None else np.zeros(self.size)

    def state_dict(self):
        return {'x_prev': self.x_prev, 'std': self.std.state_dict()}

    def load_state_dict(self, state):
        self.x_prev = state['x_prev']
        self.std.load_state_dict(state['std'])


NOISE_CLASSES = {'OrnsteinUhlenbeckProcess': OrnsteinUhlenbeckProcess, 'GaussianProcess': GaussianProcess}
SCHEDULES = {'LinearSchedule': LinearSchedule}


def make_action_noise_process(noise_config, act_dim, randn=None):
    """ddpg_utils.py:make_action_noise_process with the names resolved from math_and_models (see the module docstring)."""
    cfg = deepcopy(dict(noise_config))
    process_func = cfg.pop('func')
    std_cfg = dict(cfg.pop('std'))
    std_func, std_args = std_cfg.pop('func'), std_cfg.pop('args')
    std = SCHEDULES[std_func](std_args, **std_cfg)
    return NOISE_CLASSES[process_func](size=(act_dim,), std=std, randn=randn, **cfg)


# ---------------------------------------------------------------------------------------------------------------- networks
class MLPActor(nn.Module):
    def __init__(self, obs_dim, act_dim, hidden_dims, activation, low, high):
        super().__init__()
        self.net = MLP(obs_dim, act_dim, hidden_dims, activation)
        self.low, self.high = low, high            # (plain attributes: upstream's state dict has no bounds)

    def forward(self, obs):
        return self.low + 0.5 * (torch.tanh(self.net(obs)) + 1.0) * (self.high - self.low)


class MLPActorCritic(nn.Module):
    """state_dict layout of the reference (actor.net.fcs.{0,1,2}, q.q_net.fcs.{0,1,2})."""

    def __init__(self, obs_dim, act_dim, low, high, hidden_dims=(64, 64), activation='relu'):
        super().__init__()
        self.actor = MLPActor(obs_dim, act_dim, list(hidden_dims), activation, low, high)
        self.q = MLPQFunction(obs_dim, act_dim, list(hidden_dims), activation)

    @torch.no_grad()
    def act(self, obs, **kwargs):
        return self.actor(obs)


@dataclass
class DDPGConfig(OffPolicyConfig):
    # names and defaults of controllers/ddpg/ddpg.yaml
    hidden_dim: int = 256
    activation: str = 'relu'
    gamma: float = 0.99
    tau: float = 0.005
    random_process: dict = field(default_factory=lambda: {'func': 'OrnsteinUhlenbeckProcess', 'std': {'func': 'LinearSchedule', 'args': 0.2}})
    train_interval: int = 100
    train_batch_size: int = 64
    actor_lr: float = 0.001
    critic_lr: float = 0.001
    max_env_steps: int = 1000000
    warm_up_steps: int = 10000
    rollout_batch_size: int = 4
    max_buffer_size: int = 1000000
    extra: dict = field(default_factory=dict)


# ---------------------------------------------------------------------------------------------------------------- agent
class DDPGAgent(FlatAgent):
    OPTIMIZERS = ('actor_opt', 'critic_opt')
    LOSS_NAMES = ('policy_loss', 'critic_loss')
    ACTOR_KIND = 'ddpg'
    DETERMINISTIC_ACT = 'act'

    def __init__(self, obs_dim, act_dim, low, high, cfg: DDPGConfig, device):
        self.cfg, self.obs_dim, self.act_dim = cfg, obs_dim, act_dim
        dev = torch.device(device)
        low = torch.as_tensor(low, dtype=torch.float32, device=dev).reshape(-1)
        high = torch.as_tensor(high, dtype=torch.float32, device=dev).reshape(-1)
        self._adopt(MLPActorCritic(obs_dim, act_dim, low, high, [cfg.hidden_dim] * 2, cfg.activation).to(dev))
        # Fused gradient step (csrc/scg_ddpg.hip): the whole DDPGAgent.update as 8 launches on flat parameter vectors, replayed as a HIP
        # graph.  Chosen here, visibly: GPU runs of shapes the library serves; everything else is the eager PyTorch update below.
        from safe_control_gym_amd import _ddpg
        want = dev.type == 'cuda' and bool(cfg.extra.get('fused_update', True))
        self.use_fused = want and _ddpg.supported(obs_dim, cfg.hidden_dim, act_dim, cfg.activation)
        if want and not self.use_fused:
            warnings.warn(f'DDPG: no fused update for obs {obs_dim} hidden {cfg.hidden_dim} act {act_dim} {cfg.activation}: eager PyTorch update')
        if self.use_fused and parallel.world_size() > 1:
            raise ValueError('the fused DDPG update is single-GPU only: pass fused_update=False for data-parallel training')
        self._flat = self._flatten(low, high) if self.use_fused else None
        self._fused = None
        if self.use_fused:          # one-time kernel attributes now (not a stream operation: must not fall into a later graph capture)
            with torch.cuda.device(dev):
                D = _ddpg.lib(obs_dim, cfg.hidden_dim, act_dim, cfg.activation)
                _ddpg.check(D, D.scg_ddpg_prepare())
        self.actor_opt = torch.optim.Adam(self.ac.actor.parameters(), cfg.actor_lr)
        self.critic_opt = torch.optim.Adam(self.ac.q.parameters(), cfg.critic_lr)

    # ---- eager update (ddpg_utils.py:96-121)
    def compute_policy_loss(self, batch):
        obs = batch['obs']
        return -self.ac.q(obs, self.ac.actor(obs)).mean()

    def compute_q_loss(self, batch):
        obs, act, rew, next_obs, mask = batch['obs'], batch['act'], batch['rew'], batch['next_obs'], batch['mask']
        q = self.ac.q(obs, act)
        with torch.no_grad():
            q_targ = rew + self.cfg.gamma * mask * self.ac_targ.q(next_obs, self.ac.actor(next_obs))
        return (q - q_targ).pow(2).mean()

    def update(self, batch):
        policy_loss = self.compute_policy_loss(batch)
        self.actor_opt.zero_grad()
        policy_loss.backward()
        self._reduce(list(self.ac.actor.parameters()), '_ab')
        self.actor_opt.step()
        critic_loss = self.compute_q_loss(batch)
        self.critic_opt.zero_grad()
        critic_loss.backward()
        self._reduce(list(self.ac.q.parameters()), '_cb')
        self.critic_opt.step()
        with torch.no_grad():
            for p, pt in zip(self.ac.parameters(), self.ac_targ.parameters()):
                pt.mul_(1.0 - self.cfg.tau).add_(p, alpha=self.cfg.tau)
        return {'policy_loss': float(policy_loss.detach()), 'critic_loss': float(critic_loss.detach())}

    # ---- fused update
    def _flatten(self, low, high):
        """All trainable tensors as views of ONE flat vector [actor | q] (+ target vector, gradient, Adam moments); the torch
        modules keep working on the views (acting, evaluation, checkpoints)."""
        from safe_control_gym_amd._learn import MlpLayout

        def order(ac):
            return [p for f in ac.actor.net.fcs for p in (f.weight, f.bias)] + [p for f in ac.q.q_net.fcs for p in (f.weight, f.bias)]
        if len(self.ac.actor.net.fcs) != 3 or len(self.ac.q.q_net.fcs) != 3:
            raise ValueError('the fused DDPG update serves two hidden layers')
        fl, offs = self._flat_views(order(self.ac), order(self.ac_targ), low, high)
        lay = lambda k: MlpLayout(*offs[k:k + 6])      # noqa: E731
        return dict(fl, n_actor=offs[6], actor=lay(0), q=lay(6))

    def _fused_args(self, buffer, batch_size, idx=None):
        import ctypes as C
        from safe_control_gym_amd import _ddpg
        fl, cfg = self._flat, self.cfg
        D = _ddpg.lib(self.obs_dim, cfg.hidden_dim, self.act_dim, cfg.activation)
        dev = fl['p'].device
        ws = torch.empty(D.scg_ddpg_workspace_bytes(int(batch_size)), dtype=torch.uint8, device=dev)
        stats, acc = torch.zeros(2, device=dev), torch.zeros(2, device=dev)
        p = lambda t: t.data_ptr() if t is not None else None          # noqa: E731
        a = _ddpg.DdpgArgs(d_params=p(fl['p']), d_target=p(fl['targ']), d_grad=p(fl['g']), d_m=p(fl['m']), d_v=p(fl['v']), d_steps=p(fl['steps']),
                           actor=fl['actor'], q=fl['q'], n_actor=fl['n_actor'], n_params=fl['n'], d_obs=p(buffer.obs), d_act=p(buffer.act),
                           d_rew=p(buffer.rew), d_next_obs=p(buffer.next_obs), d_mask=p(buffer.mask), d_ring_size=p(buffer.size_i32),
                           batch=int(batch_size), gamma=float(cfg.gamma), tau=float(cfg.tau), actor_lr=float(cfg.actor_lr),
                           critic_lr=float(cfg.critic_lr), seed=fl['seed'], d_counter=p(fl['counter']), d_idx_in=p(idx), d_workspace=p(ws),
                           d_stats=p(stats), d_stats_acc=p(acc))
        for j in range(self.act_dim):
            a.act_low[j], a.act_high[j] = fl['low'][j], fl['high'][j]
        return {'D': D, 'args': a, 'ws': ws, 'stats': stats, 'acc': acc, 'C': C, 'keep': (idx, buffer)}

    def fused_step(self, F, n_steps=1):
        """Enqueue n_steps whole gradient steps (scg_ddpg_update / scg_ddpg_update_n) on the current stream."""
        from safe_control_gym_amd import _ddpg
        st = F['C'].c_void_p(torch.cuda.current_stream(self._flat['p'].device).cuda_stream)
        if n_steps == 1:
            _ddpg.check(F['D'], F['D'].scg_ddpg_update(F['C'].byref(F['args']), st))
        else:
            _ddpg.check(F['D'], F['D'].scg_ddpg_update_n(F['C'].byref(F['args']), int(n_steps), st))

    def _update_fused(self, buffer, batch_size, n_updates, lazy=False):
        if batch_size % 32:
            raise ValueError('the fused DDPG update needs train_batch_size to be a multiple of 32')
        c = self.cfg
        key = (id(buffer), batch_size, float(c.gamma), float(c.tau), float(c.actor_lr), float(c.critic_lr))
        if self._fused is None or self._fused['key'] != key:
            self._fused = dict(self._fused_args(buffer, batch_size), key=key, graphs={})
        F = self._fused
        F['acc'].zero_()
        dev = self._flat['p'].device
        g = F['graphs'].get(n_updates)
        if g is None:                               # n_updates steps as one HIP graph (7 n + 1 launches)
            with torch.cuda.device(dev):
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    self.fused_step(F, n_updates)
            F['graphs'][n_updates] = g
        g.replay()
        return self._fused_stats(F, n_updates, lazy)

    # ---- acting
    @torch.no_grad()
    def act(self, obs):
        """ac.act(obs) (ddpg_utils.py:168-170).  Fused path: one launch of the library's batched actor (scg_ddpg_act)."""
        if not self.use_fused or obs.dtype != torch.float32 or obs.dim() != 2:
            return self.ac.act(obs)
        import ctypes as C
        from safe_control_gym_amd import _ddpg
        D = _ddpg.lib(self.obs_dim, self.cfg.hidden_dim, self.act_dim, self.cfg.activation)
        lo, hi = self.act_bounds()
        x = obs.contiguous()
        out = torch.empty(x.shape[0], self.act_dim, device=x.device, dtype=torch.float32)
        with torch.cuda.device(x.device):
            _ddpg.check(D, D.scg_ddpg_act(self._flat['p'].data_ptr(), C.byref(self._flat['actor']), lo, hi,
                                          x.data_ptr(), x.shape[0], out.data_ptr(), C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)))
        return out

    def load_state_dict(self, sd, with_optimizers=True):
        """The reference's keys (ddpg_utils.py:58-72), strictly: upstream's state dict has no bounds, and neither has MLPActor's."""
        self.ac.load_state_dict(sd['ac'])
        self.ac_targ.load_state_dict(sd['ac_targ'])
        if with_optimizers:
            self._load_optimizers(sd)


# ---------------------------------------------------------------------------------------------------------------- device noise
class DeviceNoise:
    """The reference's noise process as device state for scg_ddpg_noisy_act: x_prev, the schedule position (sample() calls so far),
    the staging words a noisy launch leaves for the push's commit.  state_dict() has the reference's keys."""

    def __init__(self, random_process, act_dim, device):
        from safe_control_gym_amd import _ddpg
        self.act_dim = act_dim
        proc = make_action_noise_process(random_process, act_dim)
        self.kind = _ddpg.NOISE_OU if isinstance(proc, OrnsteinUhlenbeckProcess) else _ddpg.NOISE_GAUSSIAN
        sch = proc.std
        self.start, self.end, self.inc = float(sch.start), float(sch.end), float(sch.inc)
        self.theta, self.dt = float(getattr(proc, 'theta', 0.0)), float(getattr(proc, 'dt', 1.0))
        f = dict(device=device, dtype=torch.float64)
        self.x_prev, self.x_next = torch.zeros(4, **f), torch.zeros(4, **f)
        self.calls = torch.zeros(1, dtype=torch.int64, device=device)
        self.pending = torch.zeros(1, dtype=torch.int32, device=device)
        self.struct = _ddpg.DdpgNoise(kind=self.kind, theta=self.theta, dt=self.dt, std_start=self.start, std_end=self.end, std_inc=self.inc,
                                      d_x_prev=self.x_prev.data_ptr(), d_x_next=self.x_next.data_ptr(), d_calls=self.calls.data_ptr(),
                                      d_pending=self.pending.data_ptr())

    def reset_states(self):
        self.x_prev.zero_()
        self.x_next.zero_()
        self.pending.zero_()

    def _current(self, calls):
        v = self.start + calls * self.inc
        return min(v, self.end) if self.end > self.start else max(v, self.end)

    def state_dict(self):
        from safe_control_gym_amd import _ddpg
        if self.kind != _ddpg.NOISE_OU:             # (GaussianProcess.state_dict is empty upstream)
            return {}
        return {'x_prev': self.x_prev[:self.act_dim].cpu().numpy().copy(), 'std': {'current': self._current(int(self.calls.item()))}}

    def load_state_dict(self, sd):
        if 'x_prev' in sd:
            self.x_prev[:self.act_dim].copy_(torch.as_tensor(np.asarray(sd['x_prev'], dtype=np.float64)))
        cur = sd.get('std', {}).get('current')
        if cur is not None and self.inc != 0.0:
            self.calls.fill_(int(round((float(cur) - self.start) / self.inc)))
        self.pending.zero_()


# ---------------------------------------------------------------------------------------------------------------- controller core
class DDPG(OffPolicyTrainer):
    """DDPG.train_step / learn on a HipVecEnv (ddpg.py:164-341): OffPolicyTrainer with the actor's action plus the noise process —
    the reference's on the host (NumPy draws) for the PyTorch collector, which therefore is not captured in a HIP graph, DeviceNoise
    for the fused one (scg_ddpg_noisy_act + the env kernel + scg_ddpg_push)."""
    AGENT = DDPGAgent

    def __init__(self, env, cfg: DDPGConfig, seed=0):
        super().__init__(env, cfg, seed)
        self.noise_process = None
        if cfg.random_process:
            self.noise_process = (DeviceNoise(cfg.random_process, self.act_dim, self.device) if self._fused_collect
                                  else make_action_noise_process(cfg.random_process, self.act_dim))

    def _seed(self, seed):
        super()._seed(seed)
        np.random.seed(seed)

    def reset_noise(self):
        """noise_process.reset_states() of the reference's DDPG.reset() in training mode (ddpg.py:100-102)."""
        if self.noise_process is not None:
            self.noise_process.reset_states()

    def _explore(self):
        act = self.agent.ac.act(self.obs)
        if self.noise_process is not None:      # one sample() per env, in env order (ddpg.py:283-286)
            nz = np.stack([self.noise_process.sample() for _ in range(self.N)])
            act = (act.double() + torch.as_tensor(nz, device=self.device)).float()
        return act

    def _fused_act(self, warm, eps_in, st):
        import ctypes as C
        from safe_control_gym_amd import _ddpg
        D = _ddpg.lib(self.obs_dim, self.cfg.hidden_dim, self.act_dim, self.cfg.activation)
        fl, (lo, hi) = self.agent._flat, self.agent.act_bounds()
        nz = C.byref(self.noise_process.struct) if self.noise_process is not None else None
        p = lambda t: t.data_ptr() if t is not None else None          # noqa: E731
        _ddpg.check(D, D.scg_ddpg_noisy_act(p(fl['p']), C.byref(fl['actor']), lo, hi, p(self.obs), self.N, fl['seed'], p(self._collect_counter),
                                            int(bool(warm)), nz, p(eps_in), p(self._act), st))

    def _fused_push(self, out, st):
        import ctypes as C
        from safe_control_gym_amd import _ddpg
        D = _ddpg.lib(self.obs_dim, self.cfg.hidden_dim, self.act_dim, self.cfg.activation)
        nz = C.byref(self.noise_process.struct) if self.noise_process is not None else None
        p = lambda t: t.data_ptr()                      # noqa: E731
        _ddpg.check(D, D.scg_ddpg_push(C.byref(self._ring), nz, p(self.obs), p(self._act), p(out.reward), p(out.obs), p(out.terminal_obs),
                                       p(out.done), p(out.flags), self.N, st))

    # ---- checkpoints: the NumPy generator (the host noise draws) and the noise process travel too (ddpg.py:116-162)
    def _save_extra(self, state):
        state['random_state']['numpy'] = np.random.get_state()
        if self.noise_process is not None:
            state['noise_process'] = self.noise_process.state_dict()

    def _load_extra(self, state):
        rs = state.get('random_state') or {}
        if rs.get('numpy') is not None:
            np.random.set_state(rs['numpy'])
        if self.noise_process is not None and 'noise_process' in state:
            self.noise_process.load_state_dict(state['noise_process'])


__all__ = ['DDPG', 'DDPGAgent', 'DDPGConfig', 'DeviceNoise', 'GaussianProcess', 'LinearSchedule', 'OrnsteinUhlenbeckProcess',
           'make_action_noise_process']

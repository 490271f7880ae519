"""SAC on the HIP rollout engine.

Mirrors the reference's SAC (paths relative to /root/reference/safe_control_gym/controllers/sac):
  sac.py:269-335        train_step: one vectorised env step per call (uniform actions during warm-up), time-limit fix-up of
                        next_obs / mask (a truncated transition bootstraps from the TERMINAL observation with mask 1),
                        `train_interval` gradient updates every `train_interval` collected transitions
  sac_utils.py:110-170  losses: policy  (alpha * logp - min(q1,q2)).mean(),  twin-Q regression on
                        rew + gamma * mask * (min target-q - alpha * next_logp),  optional entropy tuning, Polyak update
  sac_utils.py:178-252  tanh-Gaussian actor (log_std clamp [-20, 2], logp -= 2 (log 2 - u - softplus(-2u))), rescaling
                        to the action space, twin MLPQFunction on [obs, act]
  sac_utils.py:301-413  SACBuffer: ring buffer (obs, act, rew, next_obs, mask), uniform sampling
  sac_utils.py:421-424  soft_update

MI355X-first differences: the replay ring lives in HBM (288 GB: 10^7 transitions of the 3-D quadrotor are 2.1 GB), the
step kernel's outputs are copied into it on device, sampling is `torch.randint` on device, and gradients travel in one
flat RCCL all-reduce per update when several ranks train (env + replay shards per rank).

What SAC shares with DDPG — the replay ring, the flat-parameter bookkeeping, the collectors, train_step / learn and the checkpoint
format — lives in offpolicy.py (FlatAgent, OffPolicyTrainer); this module holds the networks, the config, the losses, the update
paths and the hooks in which SAC differs.
"""
import math
import warnings
from dataclasses import dataclass, field

import torch
import torch.nn as nn
import torch.nn.functional as F

from safe_control_gym_amd import parallel
from safe_control_gym_amd.offpolicy import DeviceReplay, FlatAgent, OffPolicyConfig, OffPolicyTrainer  # noqa: F401 (DeviceReplay: re-exported)
from safe_control_gym_amd.ppo import MLP

LOG2 = math.log(2.0)
LOG_SQRT_2PI = 0.5 * math.log(2.0 * math.pi)


class MLPActor(nn.Module):
    def __init__(self, obs_dim, act_dim, hidden_dims, activation, low, high):
        super().__init__()
        self.net = MLP(obs_dim, hidden_dims[-1], hidden_dims[:-1], activation)
        self.mu_layer = nn.Linear(hidden_dims[-1], act_dim)
        self.log_std_layer = nn.Linear(hidden_dims[-1], act_dim)
        self.register_buffer('low', torch.as_tensor(low, dtype=torch.float32))
        self.register_buffer('high', torch.as_tensor(high, dtype=torch.float32))
        self.log_std_min, self.log_std_max = -20, 2

    def forward(self, obs, deterministic=False, with_logprob=True):
        h = self.net(obs)      # NB upstream MLP applies no activation after its last layer (neural_networks.py:50-54)
        mu = self.mu_layer(h)
        log_std = torch.clamp(self.log_std_layer(h), self.log_std_min, self.log_std_max)
        u = mu if deterministic else mu + log_std.exp() * torch.randn_like(mu)
        logp = None
        if with_logprob:
            z = (u - mu) * torch.exp(-log_std)
            logp = (-0.5 * z * z - log_std - LOG_SQRT_2PI).sum(-1, keepdim=True)
            logp = logp - (2 * (LOG2 - u - F.softplus(-2 * u))).sum(dim=1, keepdim=True)
        a = torch.tanh(u)
        return self.low + 0.5 * (a + 1.0) * (self.high - self.low), logp


class MLPQFunction(nn.Module):
    def __init__(self, obs_dim, act_dim, hidden_dims, activation):
        super().__init__()
        self.q_net = MLP(obs_dim + act_dim, 1, hidden_dims, activation)

    def forward(self, obs, act):
        return self.q_net(torch.cat([obs, act], dim=-1))


class MLPActorCritic(nn.Module):
    """state_dict layout of the reference (actor.net.fcs.*, actor.mu_layer, actor.log_std_layer, q1.q_net.fcs.*, q2...)."""

    def __init__(self, obs_dim, act_dim, low, high, hidden_dims=(64, 64), activation='relu'):
        super().__init__()
        self.actor = MLPActor(obs_dim, act_dim, list(hidden_dims), activation, low, high)
        self.q1 = MLPQFunction(obs_dim, act_dim, list(hidden_dims), activation)
        self.q2 = MLPQFunction(obs_dim, act_dim, list(hidden_dims), activation)

    @torch.no_grad()
    def act(self, obs, deterministic=False):
        return self.actor(obs, deterministic, False)[0]


@dataclass
class SACConfig(OffPolicyConfig):
    # names and defaults of controllers/sac/sac.yaml
    hidden_dim: int = 256
    activation: str = 'relu'
    gamma: float = 0.99
    tau: float = 0.005
    init_temperature: float = 0.2
    use_entropy_tuning: bool = False
    target_entropy: float = None
    train_interval: int = 100
    train_batch_size: int = 64
    actor_lr: float = 0.001
    critic_lr: float = 0.001
    entropy_lr: float = 0.001
    max_env_steps: int = 1000000
    warm_up_steps: int = 1000
    rollout_batch_size: int = 4
    max_buffer_size: int = 1000000
    extra: dict = field(default_factory=dict)


class SACAgent(FlatAgent):
    OPTIMIZERS = ('actor_opt', 'critic_opt', 'alpha_opt')
    LOSS_NAMES = ('policy_loss', 'critic_loss', 'entropy_loss')
    ACTOR_KIND = 'sac'
    DETERMINISTIC_ACT = 'act_deterministic'

    def __init__(self, obs_dim, act_dim, low, high, cfg: SACConfig, device):
        self.cfg = cfg
        self._adopt(MLPActorCritic(obs_dim, act_dim, low, high, [cfg.hidden_dim] * 2, cfg.activation).to(device))
        self.log_alpha = torch.tensor(math.log(cfg.init_temperature), device=device, requires_grad=cfg.use_entropy_tuning)
        self.target_entropy = -float(act_dim) if cfg.target_entropy is None else cfg.target_entropy
        # One HIP graph per gradient step (sample + three Adam steps + Polyak) on a single GPU: the update is ~100 tiny
        # kernels on 128-wide MLPs, i.e. launch-bound.  With several ranks the all-reduces sit between backward and step,
        # and the update stays eager.
        self.use_graphs = (torch.device(device).type == 'cuda' and bool(cfg.extra.get('cuda_graphs', True))
                           and parallel.world_size() == 1)
        # Fused gradient step (csrc/scg_sac.hip, include/scg_sac.h): the whole SACAgent.update — sampling, the five network
        # passes on the matrix cores, both Adam steps, temperature, Polyak — as 9 launches on flat parameter vectors instead
        # of ~100 PyTorch kernels.  Chosen here, visibly: single-rank GPU runs of shapes the library serves.
        from safe_control_gym_amd import _sac
        self.obs_dim, self.act_dim = obs_dim, act_dim
        self.use_fused = (torch.device(device).type == 'cuda' and bool(cfg.extra.get('cuda_graphs', True))
                          and bool(cfg.extra.get('fused_update', True))
                          and _sac.supported(obs_dim, cfg.hidden_dim, act_dim, cfg.activation))
        self._flat = self._flatten(low, high) if self.use_fused else None
        self._fused = None
        self.dp_path, self.dp_capture_error = None, None       # how the last data-parallel update ran (_update_fused)
        if self.use_fused:          # one-time kernel attributes NOW (not a stream operation: must not fall into a later graph capture)
            with torch.cuda.device(self.log_alpha.device):
                D = _sac.lib(obs_dim, cfg.hidden_dim, act_dim, cfg.activation)
                _sac.check(D, D.scg_sac_prepare())
        kw = {'capturable': True} if self.use_graphs else {}
        self.actor_opt = torch.optim.Adam(self.ac.actor.parameters(), cfg.actor_lr, **kw)
        self.critic_opt = torch.optim.Adam(list(self.ac.q1.parameters()) + list(self.ac.q2.parameters()), cfg.critic_lr, **kw)
        self.alpha_opt = torch.optim.Adam([self.log_alpha], cfg.entropy_lr, **kw)
        self._graph = None

    @property
    def alpha(self):
        return self.log_alpha.exp()

    # ---- fused update ------------------------------------------------------------------------------------------
    def _flatten(self, low, high):
        """All trainable tensors as views of ONE flat vector [actor | q1 | q2 | log_alpha] (+ a target vector in the same
        order, gradient scratch, Adam moments); the actor's two heads are stored as one [2 act_dim][H] matrix / [2 act_dim]
        bias (scg_sac.h).  The torch modules keep working on the views (acting, evaluation, checkpoints)."""
        from safe_control_gym_amd._learn import MlpLayout

        def order(ac):
            act = ac.actor
            return ([act.net.fcs[0].weight, act.net.fcs[0].bias, act.net.fcs[1].weight, act.net.fcs[1].bias, act.mu_layer.weight,
                     act.log_std_layer.weight, act.mu_layer.bias, act.log_std_layer.bias],
                    [p for f in ac.q1.q_net.fcs for p in (f.weight, f.bias)], [p for f in ac.q2.q_net.fcs for p in (f.weight, f.bias)])
        if len(self.ac.actor.net.fcs) != 2 or len(self.ac.q1.q_net.fcs) != 3:
            raise ValueError('the fused SAC update serves two hidden layers')
        params, targ_params = ([p for g in order(ac) for p in g] for ac in (self.ac, self.ac_targ))
        fl, offs = self._flat_views(params, targ_params, low, high, tail=[self.log_alpha])
        self.log_alpha.data = fl['p'][fl['n']:fl['n'] + 1].view(())
        lay = lambda k: MlpLayout(*offs[k:k + 6])      # noqa: E731
        # (actor: W3 = [mu; log_std] rows, b3 = [mu; log_std]; offs[8] is where q1 starts)
        return dict(fl, n_actor=offs[8], actor=MlpLayout(offs[0], offs[1], offs[2], offs[3], offs[4], offs[6]), q1=lay(8), q2=lay(14))

    def _fused_args(self, buffer, batch_size, idx=None, eps=None, eps_next=None):
        import ctypes as C
        from safe_control_gym_amd import _sac
        fl, cfg = self._flat, self.cfg
        D = _sac.lib(self.obs_dim, cfg.hidden_dim, self.act_dim, cfg.activation)
        dev = fl['p'].device
        with torch.cuda.device(dev):            # kernel attributes are per device (csrc/scg_once.h)
            _sac.check(D, D.scg_sac_prepare())
        ws = torch.empty(D.scg_sac_workspace_bytes(int(batch_size)), dtype=torch.uint8, device=dev)
        stats, acc = torch.zeros(4, device=dev), torch.zeros(4, device=dev)
        p = lambda t: t.data_ptr() if t is not None else None          # noqa: E731
        a = _sac.SacArgs(d_params=p(fl['p']), d_target=p(fl['targ']), d_grad=p(fl['g']), d_m=p(fl['m']), d_v=p(fl['v']), d_steps=p(fl['steps']),
                         actor=fl['actor'], q1=fl['q1'], q2=fl['q2'], n_actor=fl['n_actor'], n_params=fl['n'], d_obs=p(buffer.obs),
                         d_act=p(buffer.act), d_rew=p(buffer.rew), d_next_obs=p(buffer.next_obs), d_mask=p(buffer.mask),
                         d_ring_size=p(buffer.size_i32), batch=int(batch_size), gamma=float(cfg.gamma), tau=float(cfg.tau),
                         actor_lr=float(cfg.actor_lr), critic_lr=float(cfg.critic_lr), entropy_lr=float(cfg.entropy_lr),
                         use_entropy_tuning=int(bool(cfg.use_entropy_tuning)), target_entropy=float(self.target_entropy),
                         seed=fl['seed'], d_counter=p(fl['counter']), d_idx_in=p(idx), d_eps_in=p(eps), d_eps_next_in=p(eps_next),
                         d_workspace=p(ws), d_stats=p(stats), d_stats_acc=p(acc))
        for j in range(self.act_dim):
            a.act_low[j], a.act_high[j] = fl['low'][j], fl['high'][j]
        return {'D': D, 'args': a, 'ws': ws, 'stats': stats, 'acc': acc, 'C': C, 'keep': (idx, eps, eps_next, buffer)}

    def _fused_step(self, F, phases=0):
        """Enqueue ONE gradient step (or the given part of it, scg_sac.h: SCG_SAC_*) on the current stream."""
        from safe_control_gym_amd import _sac
        st = F['C'].c_void_p(torch.cuda.current_stream(self._flat['p'].device).cuda_stream)
        F['args'].phases = int(phases)
        _sac.check(F['D'], F['D'].scg_sac_update(F['C'].byref(F['args']), st))

    def _fused_step_dp(self, F):
        """One data-parallel gradient step: every rank samples its own minibatch; the actor's (+ temperature's) gradient and
        the critics' gradient are averaged over the ranks where sac_utils.py's update would call backward() — two all-reduces of
        the flat gradient vector per step (RCCL; latency-bound at 246 KB), everything else stays the fused kernels."""
        from safe_control_gym_amd import _sac
        g, world = self._flat['g'], max(parallel.world_size(), 1)
        self._fused_step(F, _sac.ACTOR_GRAD)
        parallel.all_reduce_sum_(g)
        g.div_(world)
        self._fused_step(F, _sac.CRITIC_GRAD)
        parallel.all_reduce_sum_(g)
        g.div_(world)
        self._fused_step(F, _sac.FINISH)

    def _update_fused(self, buffer, batch_size, n_updates, lazy=False):
        """lazy=True: enqueue only — the loss sums stay on the device ('stats_dev': policy, critic, entropy loss summed over the
        n_updates steps; valid until the next update's kernels run), nothing is read back and the call does not wait for the GPU."""
        if batch_size % 32:
            raise ValueError('the fused SAC update needs train_batch_size to be a multiple of 32')
        c = self.cfg                # (every value the argument block — and with it the captured graphs — carries BY VALUE: a changed cfg rebuilds)
        key = (id(buffer), batch_size, float(c.gamma), float(c.tau), float(c.actor_lr), float(c.critic_lr), float(c.entropy_lr),
               bool(c.use_entropy_tuning), float(c.target_entropy) if getattr(c, 'target_entropy', None) is not None else None)
        if self._fused is None or self._fused['key'] != key:
            self._fused = dict(self._fused_args(buffer, batch_size), key=key, graphs={})
        F = self._fused
        F['acc'].zero_()
        dev = self._flat['p'].device
        if parallel.world_size() > 1 or self.cfg.extra.get('force_data_parallel'):
            # Collectives between the parts of a step.  Over RCCL the n_updates steps (two all-reduces each) are ONE HIP-graph replay —
            # the first call runs eagerly (it warms the communicator up), the second captures; over gloo, or if the capture fails, the
            # steps are enqueued one by one (`dp_path` says which ran).
            with torch.cuda.device(dev):
                key = ('dp', n_updates)
                state = F['graphs'].get(key)
                if parallel.collectives_capturable() and self.cfg.extra.get('graph_collectives', True) and state != 'eager':
                    if state is None:
                        F['graphs'][key] = 'warm'
                    elif state == 'warm':
                        try:
                            torch.cuda.synchronize(dev)
                            g = torch.cuda.CUDAGraph()
                            # (thread_local: ProcessGroupNCCL's watchdog thread must not invalidate this thread's capture)
                            with torch.cuda.graph(g, capture_error_mode='thread_local'):
                                for _ in range(n_updates):
                                    self._fused_step_dp(F)
                            F['graphs'][key] = state = g
                        except Exception as exc:                    # noqa: BLE001
                            F['graphs'][key] = state = 'eager'
                            self.dp_capture_error = repr(exc)[:200]
                            warnings.warn(f'SAC data-parallel update: HIP-graph capture failed, staying on the eager loop ({self.dp_capture_error})')
                    if isinstance(state, torch.cuda.CUDAGraph):
                        state.replay()
                        self.dp_path = f'one graph replay per vector step ({n_updates} gradient steps, {2 * n_updates} all-reduces)'
                        return self._fused_stats(F, n_updates, lazy)
                self.dp_path = 'eager'
                for _ in range(n_updates):
                    self._fused_step_dp(F)
            return self._fused_stats(F, n_updates, lazy)
        g = F['graphs'].get(n_updates)
        if g is None:                               # n_updates steps as one HIP graph (7 launches each + 1: host-launch bound otherwise)
            from safe_control_gym_amd import _sac
            with torch.cuda.device(dev):
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    # scg_sac_update_n: step k + 1's first launch rides in step k's target-action launch (bit-identical to n calls)
                    F['args'].phases = 0
                    st = F['C'].c_void_p(torch.cuda.current_stream(dev).cuda_stream)
                    _sac.check(F['D'], F['D'].scg_sac_update_n(F['C'].byref(F['args']), int(n_updates), st))
            F['graphs'][n_updates] = g
        g.replay()
        return self._fused_stats(F, n_updates, lazy)

    # ---- deterministic actions for evaluation
    @torch.no_grad()
    def act_deterministic(self, obs):
        """`ac.act(obs, deterministic=True)` (sac_utils.py:209-215: tanh of the mean, rescaled to the action space).  On the fused path ONE
        launch of the library's batched actor on the flat parameter vector (scg_sac_act, exact-f32 MFMA) instead of ~9 PyTorch kernels:
        the evaluation loop is 250 sequential (policy, env step) pairs on a 256-env batch, i.e. launch-bound."""
        if not self.use_fused or obs.dtype != torch.float32 or obs.dim() != 2:
            return self.ac.act(obs, deterministic=True)
        import ctypes as C
        from safe_control_gym_amd import _sac
        fl = self._flat
        D = _sac.lib(self.obs_dim, self.cfg.hidden_dim, self.act_dim, self.cfg.activation)
        lo, hi = self.act_bounds()
        x = obs.contiguous()
        out = torch.empty(x.shape[0], self.act_dim, device=x.device, dtype=torch.float32)
        with torch.cuda.device(x.device):
            _sac.check(D, D.scg_sac_act(fl['p'].data_ptr(), C.byref(fl['actor']), lo, hi, x.data_ptr(), x.shape[0], out.data_ptr(),
                                        C.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)))
        return out

    # same keys as the reference's SACAgent (sac_utils.py:85-108), so its checkpoints load directly; the action bounds are
    # buffers here (not in upstream's state dict), hence strict=False
    def state_dict(self):
        sd = super().state_dict()
        return {'ac': sd.pop('ac'), 'log_alpha': self.log_alpha.detach().clone(), **sd}

    def load_state_dict(self, sd, with_optimizers=True):
        self.ac.load_state_dict(sd['ac'], strict=False)
        if 'ac_targ' in sd:
            self.ac_targ.load_state_dict(sd['ac_targ'], strict=False)
        if 'log_alpha' in sd:
            with torch.no_grad():
                self.log_alpha.copy_(torch.as_tensor(sd['log_alpha'], dtype=self.log_alpha.dtype).reshape(()))
        if with_optimizers and 'actor_opt' in sd:
            self._load_optimizers(sd)
            self._graph = None              # the captured update graph aliases the replaced Adam state: re-captured on the next update

    def policy_loss(self, batch):
        obs = batch['obs']
        act, logp = self.ac.actor(obs)
        q = torch.min(self.ac.q1(obs, act), self.ac.q2(obs, act))
        policy_loss = (self.alpha.detach() * logp - q).mean()
        entropy_loss = torch.zeros((), device=obs.device)
        if self.cfg.use_entropy_tuning:
            entropy_loss = -(self.log_alpha * (logp + self.target_entropy).detach()).mean()
        return policy_loss, entropy_loss

    def q_loss(self, batch):
        obs, act, rew, next_obs, mask = batch['obs'], batch['act'], batch['rew'], batch['next_obs'], batch['mask']
        q1, q2 = self.ac.q1(obs, act), self.ac.q2(obs, act)
        with torch.no_grad():
            next_act, next_logp = self.ac.actor(next_obs)
            nq = torch.min(self.ac_targ.q1(next_obs, next_act), self.ac_targ.q2(next_obs, next_act))
            q_targ = rew + self.cfg.gamma * mask * (nq - self.alpha * next_logp)
        return (q1 - q_targ).pow(2).mean() + (q2 - q_targ).pow(2).mean()

    def update(self, batch):
        """sac_utils.py:143-170: actor step, optional temperature step, critic step, Polyak update."""
        policy_loss, entropy_loss = self.policy_loss(batch)
        self.actor_opt.zero_grad(set_to_none=False)
        policy_loss.backward()
        self._reduce(list(self.ac.actor.parameters()), '_ab')
        self.actor_opt.step()
        if self.cfg.use_entropy_tuning:
            self.alpha_opt.zero_grad()
            entropy_loss.backward()
            if parallel.world_size() > 1:
                parallel.all_reduce_sum_(self.log_alpha.grad).div_(parallel.world_size())
            self.alpha_opt.step()
        critic_loss = self.q_loss(batch)
        self.critic_opt.zero_grad(set_to_none=False)
        critic_loss.backward()
        self._reduce(list(self.ac.q1.parameters()) + list(self.ac.q2.parameters()), '_cb')
        self.critic_opt.step()
        with torch.no_grad():       # soft_update (sac_utils.py:421-424)
            for p, pt in zip(self.ac.parameters(), self.ac_targ.parameters()):
                pt.mul_(1.0 - self.cfg.tau).add_(p, alpha=self.cfg.tau)
        return {'policy_loss': policy_loss.detach(), 'critic_loss': critic_loss.detach(), 'entropy_loss': entropy_loss.detach()}


    def update_from_buffer(self, buffer, batch_size, n_updates, lazy=False):
        """As FlatAgent's; the eager update replays one captured graph per step when HIP graphs are on."""
        if self.use_fused or not self.use_graphs:
            return super().update_from_buffer(buffer, batch_size, n_updates, lazy=lazy)
        if self._graph is None or self._graph['key'] != (id(buffer), batch_size):
            dev = buffer.obs.device
            stats = torch.zeros(3, device=dev)

            def one():
                res = self.update(buffer.sample_static(batch_size))
                stats.add_(torch.stack([res['policy_loss'], res['critic_loss'], res['entropy_loss']]))

            s = torch.cuda.Stream(dev)
            s.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(s):
                for _ in range(3):                      # warm-up = three real gradient steps
                    one()
            torch.cuda.current_stream(dev).wait_stream(s)
            for opt in (self.actor_opt, self.critic_opt, self.alpha_opt):
                opt.zero_grad(set_to_none=True)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                one()
            self._graph = {'key': (id(buffer), batch_size), 'g': g, 'stats': stats}
        G = self._graph
        G['stats'].zero_()
        for _ in range(n_updates):
            G['g'].replay()
        st = (G['stats'] / n_updates).tolist()
        return {'policy_loss': st[0], 'critic_loss': st[1], 'entropy_loss': st[2]}


class SAC(OffPolicyTrainer):
    """SAC.train_step / learn on a HipVecEnv (sac.py:162-335): OffPolicyTrainer with a sampled action."""
    AGENT = SACAgent
    _graph_eager_collector = True       # sampling is torch.randn_like on the device: the PyTorch collector is capturable
    # extra['collect_steps'] = K: up to K vector steps per launch into the replay ring (scg_rollout_sac_collect through
    # OffPolicyTrainer._collect_chunk), on the stepwise update schedule (offpolicy.chunk_steps).  The chunked collector draws its
    # action noise from the envs' Philox streams, the stepwise one from the agent's counter stream: the two train on different
    # samples at the same seed
    CHUNKED_COLLECT = True

    def _explore(self):
        return self.agent.ac.act(self.obs)

    def _fused_act(self, warm, eps_in, st):
        """scg_sac_sample: the uniform warm-up action or a sample of the policy."""
        import ctypes as C
        from safe_control_gym_amd import _sac
        D = _sac.lib(self.obs_dim, self.cfg.hidden_dim, self.act_dim, self.cfg.activation)
        fl, (lo, hi) = self.agent._flat, self.agent.act_bounds()
        p = lambda t: t.data_ptr() if t is not None else None          # noqa: E731
        _sac.check(D, D.scg_sac_sample(p(fl['p']), C.byref(fl['actor']), lo, hi, p(self.obs), self.N, fl['seed'], p(self._collect_counter),
                                       int(bool(warm)), p(eps_in), p(self._act), st))

    def _fused_push(self, out, st):
        import ctypes as C
        from safe_control_gym_amd import _sac
        D = _sac.lib(self.obs_dim, self.cfg.hidden_dim, self.act_dim, self.cfg.activation)
        p = lambda t: t.data_ptr()                      # noqa: E731
        _sac.check(D, D.scg_sac_push(C.byref(self._ring), p(self.obs), p(self._act), p(out.reward), p(out.obs), p(out.terminal_obs), p(out.done),
                                     p(out.flags), self.N, st))

    def _resumed_without_ring(self):
        warnings.warn('SAC checkpoint without replay buffer (save_buffer=False): training resumes past warm-up with an '
                      'EMPTY buffer — the first updates sample only the transitions collected since the resume')

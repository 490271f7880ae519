"""What the off-policy learners (sac.py, ddpg.py) share: the device replay ring, the agent on flat parameter vectors and the trainer.

  DeviceReplay      the replay ring in HBM
  OffPolicyConfig   `from_dict` of the config dataclasses
  FlatAgent         base of SACAgent / DDPGAgent: target network, gradient all-reduce, the flat vector the fused kernels step (views,
                    offsets, padded bounds, actor struct), the two Adam layouts, the statistics read-out, the eager update loop
  OffPolicyTrainer  base of SAC / DDPG: constructor, the PyTorch and the fused collector, their HIP-graph capture, train_step, learn,
                    save, load (ONE checkpoint format)

An algorithm keeps its networks, config, losses, eager `update`, `_flatten` order, `_fused_args` and `_update_fused`, and says where it
differs from the other one through the class attributes and the small hooks named below — nowhere else.
"""
import ctypes as C
import os
import time
import warnings
from copy import deepcopy

import torch

from safe_control_gym_amd import _shapelib, parallel


def chunk_steps(total_steps, since_update, n_envs_times_world, warm_up_steps, train_interval, k_max):
    """Vector steps of the chunked collector's next launch, so that OffPolicyTrainer.train_step's schedule is the stepwise one whatever
    k_max is.  The stepwise loop, per vector step: the action is uniform while total_steps < warm_up_steps; then total_steps and
    since_update grow by n_envs_times_world; then an update of since_update gradient steps is owed if total_steps > warm_up_steps and
    since_update >= train_interval.  A chunk ends at the earliest of: k_max steps; the last warm-up step (one launch has one mode); the
    first step after which an update is owed (the update must see exactly the transitions the stepwise trainer's would).  >= 1."""
    nw = int(n_envs_times_world)
    k = max(int(k_max), 1)
    if total_steps < warm_up_steps:                     # steps j = 0 .. with total_steps + j nw < warm_up_steps
        k = min(k, -(-(warm_up_steps - total_steps) // nw))
    past_warm_up = max((warm_up_steps - total_steps) // nw + 1, 1)         # first j >= 1 with total_steps + j nw > warm_up_steps
    interval_full = max(-(-(train_interval - since_update) // nw), 1)      # first j >= 1 with since_update + j nw >= train_interval
    return max(min(k, max(past_warm_up, interval_full)), 1)


class OffPolicyConfig:
    """Mixin of the config dataclasses: keys that are no field travel in `extra`."""

    @classmethod
    def from_dict(cls, d):
        known = {k: v for k, v in d.items() if k in cls.__dataclass_fields__}
        return cls(**known, extra={k: v for k, v in d.items() if k not in cls.__dataclass_fields__})


class DeviceReplay:
    """SACBuffer (sac_utils.py:301-413) as device tensors; a push appends a whole vectorised step.  The write position lives on the
    device as well (`pos_t`), so a push is a fixed sequence of static-shape device operations — capturable in a HIP graph together with
    the policy forward and the env step (OffPolicyTrainer._collect); `pos` / `size` are the host's mirror of it, advanced arithmetically."""

    def __init__(self, capacity, obs_dim, act_dim, device):
        f = dict(device=device, dtype=torch.float32)
        self.capacity = int(capacity)
        self.obs = torch.zeros(self.capacity, obs_dim, **f)
        self.next_obs = torch.zeros(self.capacity, obs_dim, **f)
        self.act = torch.zeros(self.capacity, act_dim, **f)
        self.rew = torch.zeros(self.capacity, 1, **f)
        self.mask = torch.ones(self.capacity, 1, **f)
        self.pos, self.size = 0, 0
        self.pos_t = torch.zeros((), dtype=torch.int64, device=device)          # `pos` on the device
        self.size_t = torch.zeros((), device=device)         # `size` as a device scalar: sampling inside a captured graph
        self.size_i32 = torch.zeros(1, dtype=torch.int32, device=device)       # (the fused update samples in its own kernel)
        self._ar = None

    def push_device(self, obs, act, rew, next_obs, mask):
        """The device side of a push: rows pos .. pos + n - 1 (mod capacity) of the ring, then pos / size advance — no host value."""
        n = obs.shape[0]
        if n > self.capacity:
            raise ValueError('replay capacity smaller than one vectorised step')
        if self._ar is None or self._ar.shape[0] != n:
            self._ar = torch.arange(n, device=self.obs.device)
        idx = (self._ar + self.pos_t) % self.capacity
        self.obs.index_copy_(0, idx, obs)
        self.act.index_copy_(0, idx, act)
        self.next_obs.index_copy_(0, idx, next_obs)
        self.rew.index_copy_(0, idx, rew.reshape(n, 1))
        self.mask.index_copy_(0, idx, mask.reshape(n, 1))
        self.pos_t.add_(n).remainder_(self.capacity)
        self.size_t.add_(float(n)).clamp_(max=float(self.capacity))
        self.size_i32.add_(n).clamp_(max=self.capacity)

    def advance_host(self, n):
        self.pos = (self.pos + n) % self.capacity
        self.size = min(self.size + n, self.capacity)

    def push(self, obs, act, rew, next_obs, mask):
        self.push_device(obs, act, rew, next_obs, mask)
        self.advance_host(obs.shape[0])

    def state_dict(self):
        """SACBuffer.state_dict (sac_utils.py:330-338): the filled part of the ring + the write position."""
        n = self.size
        return {'obs': self.obs[:n].cpu(), 'act': self.act[:n].cpu(), 'rew': self.rew[:n].cpu(), 'next_obs': self.next_obs[:n].cpu(),
                'mask': self.mask[:n].cpu(), 'pos': self.pos, 'size': self.size}

    def load_state_dict(self, sd):
        n = int(sd['size'])
        if n > self.capacity:
            raise ValueError(f'checkpointed replay holds {n} transitions, capacity is {self.capacity}')
        for k in ('obs', 'act', 'rew', 'next_obs', 'mask'):
            getattr(self, k)[:n].copy_(sd[k].to(self.obs.device))
        self.pos, self.size = int(sd['pos']) % self.capacity, n
        self.pos_t.fill_(self.pos)
        self.size_t.fill_(float(n))
        self.size_i32.fill_(n)

    def sample_static(self, batch_size):
        """Uniform sample with static shapes and no host value: usable under HIP-graph capture."""
        idx = (torch.rand(batch_size, device=self.obs.device) * self.size_t).long().clamp_(min=0)
        idx = torch.minimum(idx, (self.size_t - 1).clamp(min=0).long())
        return {'obs': self.obs[idx], 'act': self.act[idx], 'rew': self.rew[idx], 'next_obs': self.next_obs[idx],
                'mask': self.mask[idx]}

    def sample(self, batch_size, generator=None):
        idx = torch.randint(0, self.size, (batch_size,), device=self.obs.device, generator=generator)
        return {'obs': self.obs[idx], 'act': self.act[idx], 'rew': self.rew[idx], 'next_obs': self.next_obs[idx],
                'mask': self.mask[idx]}


class FlatAgent:
    """An actor-critic `ac` with its target copy `ac_targ`, torch.optim Adam optimisers and, on the fused path (`use_fused`), `_flat`:
    every trainable tensor as a view of one flat vector that the library's kernels step."""
    OPTIMIZERS = ()             # attribute names of the optimisers; position = index into the flat `steps` vector
    LOSS_NAMES = ()             # names of the leading words of the fused update's statistics
    ACTOR_KIND = None           # key of _lib.ACTOR_KINDS
    DETERMINISTIC_ACT = None    # name of the method deterministic_policy() serves

    def _adopt(self, ac):
        """`ac` (rank 0's weights on every rank) and its frozen target copy."""
        self.ac = ac
        parallel.broadcast_parameters([self.ac])
        self.ac_targ = deepcopy(self.ac)
        for p in self.ac_targ.parameters():
            p.requires_grad = False
        self._ab = self._cb = None

    def _reduce(self, params, attr):
        if parallel.world_size() > 1:
            b = getattr(self, attr)
            if b is None:
                b = parallel.FlatBucket(params)
                setattr(self, attr, b)
            b.pack()
            b.all_reduce_mean()
            b.unpack()

    # ---- the flat vectors
    def _flat_views(self, params, targ_params, low, high, tail=()):
        """`params` become views of ONE flat vector (followed by the one-word tensors `tail`, which the caller re-points), `targ_params`
        views of a target vector in the same order; with them gradient scratch, Adam moments and step counts, the bounds, the sampling
        counter and seed of the update kernels.  Returns that dict and the offsets of `params`; the torch modules keep working on the
        views (acting, evaluation, checkpoints)."""
        dev = params[0].device
        flat = torch.cat([p.data.reshape(-1) for p in params] + [t.data.reshape(1) for t in tail]).contiguous()
        offs, off = [], 0
        for p in params:
            offs.append(off)
            p.data = flat[off:off + p.numel()].view_as(p)
            off += p.numel()
        n = off
        targ = torch.empty(n, device=dev)
        off = 0
        for p in targ_params:
            targ[off:off + p.numel()].copy_(p.data.reshape(-1))
            p.data = targ[off:off + p.numel()].view_as(p)
            off += p.numel()
        z = lambda: torch.zeros(flat.numel(), device=dev)          # noqa: E731
        return {'p': flat, 'targ': targ, 'g': z(), 'm': z(), 'v': z(), 'steps': torch.zeros(len(self.OPTIMIZERS), device=dev), 'n': n,
                'low': [float(x) for x in low.reshape(-1)], 'high': [float(x) for x in high.reshape(-1)],
                'counter': torch.zeros(1, dtype=torch.int32, device=dev), 'seed': int(torch.initial_seed()) & 0xFFFFFFFFFFFFFFFF}, offs

    def _flat_offset(self, p):
        fl = self._flat['p']
        return (p.data_ptr() - fl.data_ptr()) // fl.element_size()

    def act_bounds(self):
        """(low, high) as the float[4] arrays the library calls take, padded with zeros."""
        fl = self._flat
        if '_act_bounds' not in fl:
            pad = [0.0] * (4 - self.act_dim)
            fl['_act_bounds'] = ((C.c_float * 4)(*(fl['low'] + pad)), (C.c_float * 4)(*(fl['high'] + pad)))
        return fl['_act_bounds']

    def packed_actor(self):
        """The actor's six tensors as ONE packed float32 vector, for agents off the fused path (no flat parameter vector), laid out as
        the fused agent's actor block: W1, b1, W2, b2, W3, b3 in nn.Linear layout, SAC's W3 / b3 the stacked [2 act_dim][H] head whose
        first act_dim rows are the mean's.  A persistent buffer on the parameters' device (its pointer never changes), refreshed in
        place from the module's parameters on every call.  Returns {'p': the vector, 'offsets': {'W1': ..., ..., 'b3': ...} in floats,
        'low' / 'high': the float[4] bounds}."""
        a = self.ac.actor
        fcs = a.net.fcs
        if hasattr(a, 'mu_layer'):                  # SAC: trunk of two layers, the two heads stacked (mean rows first)
            parts = {'W1': [fcs[0].weight], 'b1': [fcs[0].bias], 'W2': [fcs[1].weight], 'b2': [fcs[1].bias],
                     'W3': [a.mu_layer.weight, a.log_std_layer.weight], 'b3': [a.mu_layer.bias, a.log_std_layer.bias]}
        else:                                       # DDPG: the output layer is the third of the trunk
            parts = {n + str(k + 1): [getattr(fcs[k], attr)] for k in range(3) for n, attr in (('W', 'weight'), ('b', 'bias'))}
        order = ('W1', 'b1', 'W2', 'b2', 'W3', 'b3')
        pk = getattr(self, '_packed_actor', None)
        if pk is None:
            if len(fcs) != (2 if hasattr(a, 'mu_layer') else 3):
                raise ValueError('the packed actor vector serves two hidden layers')
            offsets, off = {}, 0
            for name in order:
                offsets[name] = off
                off += sum(t.numel() for t in parts[name])
            pad = [0.0] * (4 - self.act_dim)
            low, high = ([float(x) for x in torch.as_tensor(b).reshape(-1)] for b in (a.low, a.high))
            pk = self._packed_actor = {'p': torch.empty(off, dtype=torch.float32, device=fcs[0].weight.device), 'offsets': offsets,
                                       'low': (C.c_float * 4)(*(low + pad)), 'high': (C.c_float * 4)(*(high + pad))}
        with torch.no_grad():
            for name in order:
                off = pk['offsets'][name]
                for t in parts[name]:
                    pk['p'][off:off + t.numel()].copy_(t.detach().reshape(-1))
                    off += t.numel()
        return pk

    def actor_struct(self):
        """The scg_actor (_lib.Actor, include/scg_actor_rollout.h) of the deterministic actor for the fused rollout (HipVecEnv.rollout_actor):
        the flat vector's actor layout (SAC: W3 / b3 the stacked head, whose first act_dim rows are the mean's) and the padded bounds.
        An agent off its fused path (hidden width 256, fused_update off) has no flat vector: the struct then points at packed_actor()'s
        copy, refreshed by this call."""
        from safe_control_gym_amd import _lib as L
        if not self.use_fused:
            pk = self.packed_actor()
            return L.Actor(d_params=pk['p'].data_ptr(), **pk['offsets'], hidden=self.cfg.hidden_dim, activation=L.POLICY_ACTS[self.cfg.activation],
                           kind=L.ACTOR_KINDS[self.ACTOR_KIND], act_low=pk['low'], act_high=pk['high'])
        fl, lay = self._flat, self._flat['actor']
        lo, hi = self.act_bounds()
        return L.Actor(d_params=fl['p'].data_ptr(), W1=lay.W1, b1=lay.b1, W2=lay.W2, b2=lay.b2, W3=lay.W3, b3=lay.b3, hidden=self.cfg.hidden_dim,
                       activation=L.POLICY_ACTS[self.cfg.activation], kind=L.ACTOR_KINDS[self.ACTOR_KIND], act_low=lo, act_high=hi)

    def deterministic_policy(self):
        """An object with `.act(obs)` for ppo.evaluate / the controllers (one per agent: evaluate caches its captured graph per policy object)."""
        if getattr(self, '_det_policy', None) is None:
            agent = self

            class _Det:
                ac = agent.ac

                @staticmethod
                def act(obs):
                    return getattr(agent, agent.DETERMINISTIC_ACT)(obs)
            self._det_policy = _Det()
        return self._det_policy

    # ---- updates
    def _fused_stats(self, F, n_updates, lazy):
        """lazy: the loss sums stay on the device ('stats_dev': summed over the n_updates steps, valid until the next update's kernels
        run) and nothing is read back; else their means as floats."""
        if lazy:
            return {'stats_dev': F['acc'], 'stats_updates': n_updates}
        return dict(zip(self.LOSS_NAMES, (F['acc'] / n_updates).tolist()))

    def update_from_buffer(self, buffer, batch_size, n_updates, lazy=False):
        """n_updates gradient steps on fresh uniform samples: the fused library (lazy: see _fused_stats), else the eager `update`."""
        if self.use_fused:
            return self._update_fused(buffer, batch_size, n_updates, lazy=lazy)
        acc = None
        for _ in range(n_updates):
            res = self.update(buffer.sample(batch_size))
            acc = res if acc is None else {k: acc[k] + v for k, v in res.items()}
        return {k: float(v) / n_updates for k, v in acc.items()}

    # ---- the two Adam layouts: torch.optim per-parameter state <-> the fused update's flat m / v / steps
    def _opt_groups(self):
        return tuple((getattr(self, name), which) for which, name in enumerate(self.OPTIMIZERS))

    def _adam_flat_to_torch(self):
        """Write the flat moments into the torch optimisers' state (what their state_dict() then carries): a checkpoint of a fused
        agent resumes in an agent that steps torch.optim (CPU, unsupported shape, fused_update off) and in the reference's agent."""
        fl = self._flat
        steps = fl['steps'].tolist()
        for opt, which in self._opt_groups():
            if steps[which] <= 0:
                continue
            for p in opt.param_groups[0]['params']:
                o, k = self._flat_offset(p), p.numel()
                st = opt.state[p]
                st['exp_avg'] = fl['m'][o:o + k].view_as(p).clone()
                st['exp_avg_sq'] = fl['v'][o:o + k].view_as(p).clone()
                st['step'] = torch.tensor(float(steps[which]), device=p.device if opt.defaults.get('capturable') else 'cpu')

    def _adam_torch_to_flat(self):
        """The converse: per-parameter torch.optim state (the reference's training checkpoints, or one saved with fused_update off)
        scattered into the flat moments the fused kernels step."""
        fl = self._flat
        for opt, which in self._opt_groups():
            n_steps = 0.0
            for p in opt.param_groups[0]['params']:
                st = opt.state.get(p)
                o, k = self._flat_offset(p), p.numel()
                if not st:                      # no state for this parameter (zero-step checkpoint): a load is a full overwrite
                    fl['m'][o:o + k].zero_()
                    fl['v'][o:o + k].zero_()
                    continue
                fl['m'][o:o + k].copy_(st['exp_avg'].reshape(-1))
                fl['v'][o:o + k].copy_(st['exp_avg_sq'].reshape(-1))
                n_steps = float(st['step'])
            fl['steps'][which] = n_steps

    # ---- checkpoints: the reference's keys (sac_utils.py:85-108, ddpg_utils.py:58-72); the fused Adam moments travel in torch.optim's layout
    def state_dict(self):
        if self._flat is not None:
            self._adam_flat_to_torch()
        sd = {'ac': self.ac.state_dict(), 'ac_targ': self.ac_targ.state_dict()}
        sd.update({name: getattr(self, name).state_dict() for name in self.OPTIMIZERS})
        if self._flat is not None:          # fused mode: the sampling counter of the update kernels
            sd['flat_adam'] = {'counter': self._flat['counter'].clone()}
        return sd

    def _load_optimizers(self, sd):
        """(also with HIP graphs on: capturable Adam keeps its state in device tensors, which load_state_dict replaces — a captured
        update graph aliases the old ones and must be re-captured)"""
        for name in self.OPTIMIZERS:
            opt = getattr(self, name)
            opt.load_state_dict(sd[name])
            if not opt.defaults.get('capturable'):      # (a checkpoint mapped onto the GPU: eager Adam keeps its step counts on the host)
                for st in opt.state.values():
                    if torch.is_tensor(st.get('step')):
                        st['step'] = st['step'].cpu()
        if self._flat is not None:      # in place: captured graphs alias the flat buffers
            self._adam_torch_to_flat()
            for k, t in sd.get('flat_adam', {}).items():        # (early checkpoints carry m / v / steps here as well: same values)
                self._flat[k].copy_(t.to(self._flat[k].device))


class OffPolicyTrainer:
    """train_step / learn / save / load on a HipVecEnv (sac.py:119-335, ddpg.py:116-341 of the reference: same keys)."""
    AGENT = None                        # the FlatAgent subclass
    _graph_eager_collector = False      # whether the PyTorch collector is captured in a HIP graph too (the fused one always is)

    def __init__(self, env, cfg, seed=0):
        self.env, self.cfg = env, cfg
        self.device = env.device
        if env.dtype != torch.float32:
            raise ValueError(f'the {type(self).__name__} collector runs on float32 environments')
        # sac.yaml:6-9 / sac.py:75-81: running normalisers around env.step (defaults off), device-resident (normalization.py)
        from safe_control_gym_amd.normalization import BaseNormalizer, MeanStdNormalizer, RewardStdNormalizer
        x = cfg.extra
        self.obs_normalizer = (MeanStdNormalizer((env.spec.obs_dim,), self.device, clip=x.get('clip_obs', 10.0)) if x.get('norm_obs')
                               else BaseNormalizer())
        self.reward_normalizer = (RewardStdNormalizer(cfg.gamma, self.device, clip=x.get('clip_reward', 10.0)) if x.get('norm_reward')
                                  else BaseNormalizer())
        self._normalise = bool(x.get('norm_obs') or x.get('norm_reward'))
        if x.get('norm_reward'):        # eager: graphs captured later (and checkpoint loads, in place) share this storage
            self.reward_normalizer.ret = torch.zeros(env.num_envs, dtype=torch.float64, device=self.device)
        spec = env.spec
        self.N, self.obs_dim, self.act_dim = env.num_envs, spec.obs_dim, spec.nu
        rank = torch.distributed.get_rank() if parallel.world_size() > 1 else 0
        self._seed(seed + 7919 * rank)
        self.low = torch.as_tensor(spec.action_space.low, dtype=torch.float32, device=self.device)
        self.high = torch.as_tensor(spec.action_space.high, dtype=torch.float32, device=self.device)
        # (the order below is the order the seeded generator is consumed in, and the agent's _flatten reads torch.initial_seed())
        self.agent = self.AGENT(self.obs_dim, self.act_dim, self.low, self.high, cfg, self.device)
        self.buffer = DeviceReplay(cfg.max_buffer_size, self.obs_dim, self.act_dim, self.device)
        self.obs = self.obs_normalizer(env.reset_tensors()).clone()         # sac.py:103-104; persistent storage (captured graphs alias it)
        self.total_steps = 0
        self._since_update = 0
        self._graph_collect = self.device.type == 'cuda' and bool(cfg.extra.get('graph_collect', cfg.extra.get('cuda_graphs', True)))
        self._collect_graphs = {}
        # fused collector: the exploratory action in ONE launch on the flat parameter vector (in-kernel Philox noise) and the time-limit
        # fix-up + five ring writes + position bookkeeping in two, in place of ~40 PyTorch kernels per vector step.  Needs the fused agent
        # and no running normalisers; extra['fused_collect'] = False keeps the PyTorch collector (A/B, tests) — chosen here, visibly.
        self._fused_collect = bool(self.agent.use_fused and not self._normalise and cfg.extra.get('fused_collect', True))
        # evaluation as ONE scg_rollout_actor launch: set by the controller's extension key `fused_rollout` (controllers.py)
        self._fused_rollout = False
        self._ring = self._ring_of = None
        if self._fused_collect:
            self._act = torch.zeros(self.N, self.act_dim, device=self.device)
            self._collect_counter = torch.zeros(1, dtype=torch.int32, device=self.device)       # counter word of the action noise
        self._collect_k = self._chunked_collect_steps()
        self._chunk = None

    def _chunked_collect_steps(self):
        """K of the chunked collector (extension key `collect_steps`, controllers.py), or 0: the stepwise collector.  A config error
        raises; a need that is unmet at run time warns once and keeps the stepwise collector."""
        k = int(self.cfg.extra.get('collect_steps') or 0)
        if k <= 0:
            return 0
        if not self.CHUNKED_COLLECT:
            raise ValueError(f'{type(self).__name__}: collect_steps is served for SAC only')
        if k * self.N > self.cfg.max_buffer_size:
            raise ValueError(f'collect_steps x envs = {k * self.N} exceeds max_buffer_size = {self.cfg.max_buffer_size}: a launch may not '
                             f'overwrite its own rows')
        unmet = [why for ok, why in ((self._fused_collect, 'the agent on its fused path without running normalisers'),
                                     (parallel.world_size() == 1, 'one rank'),
                                     (getattr(self.env, 'sac_collect_supported', False),
                                      "an env built with policy=(hidden_dim <= 128, activation, 'sac') (fused_rollout=True)")) if not ok]
        if unmet:
            warnings.warn(f'collect_steps={k} needs {"; ".join(unmet)}: keeping the stepwise collector')
            return 0
        return k

    # ---- hooks: every difference between the algorithms' trainers
    CHUNKED_COLLECT = False             # whether `collect_steps` is served (SAC: scg_rollout_sac_collect)

    def _seed(self, seed):
        torch.manual_seed(seed)

    def _explore(self):
        """The PyTorch collector's exploratory action on `self.obs` after warm-up."""
        raise NotImplementedError

    def _fused_act(self, warm, eps_in, st):
        """The fused collector's action launch on stream `st`: into `self._act`, uniform during warm-up; eps_in: [N][act_dim] N(0, 1)
        draws in place of the in-kernel Philox ones (replaying a recorded run)."""
        raise NotImplementedError

    def _fused_push(self, out, st):
        """The fused collector's push of (self.obs, self._act, the env's outputs `out`) into `self._ring`."""
        raise NotImplementedError

    def _save_extra(self, state):
        """Training state only this algorithm has, into the checkpoint `state`."""

    def _load_extra(self, state):
        pass

    def _resumed_without_ring(self):
        """A training checkpoint without the replay ring was loaded past warm-up."""

    # ---- one vectorised env step into the replay ring (sac.py:273-311, ddpg.py:273-316)
    def uniform_action(self):
        """The warm-up's action_space.sample() per env (sac.py:276-277), for the PyTorch collector."""
        return self.low + (self.high - self.low) * torch.rand(self.N, self.act_dim, device=self.device)

    def _policy_struct(self, deterministic=True):
        """The actor for the fused evaluation (ppo.evaluate(policy=)): deterministic only."""
        return self.agent.actor_struct()

    @torch.no_grad()
    def _collect_body(self, warm):
        """Static-shape device operations only: action (uniform during warm-up, else the exploratory one), env step kernel,
        time-limit fix-up, normalisers, ring push, the next observation into the persistent `self.obs`."""
        if self._fused_collect:
            return self._collect_body_fused(warm)
        act = self.uniform_action() if warm else self._explore()
        out = self.env.step_tensors(act)
        done = out.done.bool()
        trunc = (out.flags & 1).bool() & done
        if self._normalise:
            # sac.py:281-297, in upstream's order: next_obs, then the reward (running returns, its index-array reset), then the
            # terminal observations of the TRUNCATED envs only — each call updates the running statistics
            self.obs_normalizer.unset_read_only()
            obs_n = self.obs_normalizer(out.obs)
            rew = self.reward_normalizer(out.reward, done)
            term_n = self.obs_normalizer(out.terminal_obs, mask=trunc)
        else:
            obs_n, rew, term_n = out.obs, out.reward, out.terminal_obs
        # time truncation is not termination: the stored next state is the terminal observation, mask 1 (sac.py:287-305)
        next_obs = torch.where(trunc[:, None], term_n, obs_n)
        mask = torch.where(trunc, torch.ones_like(out.reward), 1.0 - done.to(torch.float32))
        self.buffer.push_device(self.obs, act, rew, next_obs, mask)
        self.obs.copy_(obs_n)

    def _collect_body_fused(self, warm, eps_in=None):
        """The same vector step as three library calls / four launches: the action (_fused_act), the env step kernel, the push
        (_fused_push: fix-up, ring rows, current observation, position / size / noise counter)."""
        buf = self.buffer
        if self._ring_of is not buf:
            p = lambda t: t.data_ptr()                      # noqa: E731
            self._ring = _shapelib.Ring(d_obs=p(buf.obs), d_act=p(buf.act), d_rew=p(buf.rew), d_next_obs=p(buf.next_obs), d_mask=p(buf.mask),
                                        capacity=buf.capacity, d_pos=p(buf.pos_t), d_size_f=p(buf.size_t), d_size_i32=p(buf.size_i32),
                                        d_counter=p(self._collect_counter))
            self._ring_of = buf
        if self.N > buf.capacity:
            raise ValueError('replay capacity smaller than one vectorised step')
        with torch.cuda.device(self.device):
            st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            self._fused_act(warm, eps_in, st)
            self._fused_push(self.env.step_tensors(self._act), st)

    def _collect(self, warm):
        """Eager, or (GPU, cfg.extra['cuda_graphs'] not off) ONE HIP-graph replay per vector step: the PyTorch collector is ~45 small
        launches per step — policy MLP, sampling, env kernel, fix-up, five ring writes — i.e. host-launch bound (0.7 ms of a 2.7 ms
        vector step at 2048 envs x 16 gradient steps).  One graph per phase (warm-up / policy), captured after two eager steps of
        that phase and re-captured after env.seed() (the Philox key is a kernel argument)."""
        if not self._graph_collect or not (self._fused_collect or self._graph_eager_collector):
            self._collect_body(warm)
            return
        key = (bool(warm), getattr(self.env, 'seed_epoch', 0), id(self.buffer))
        st = self._collect_graphs.get(key)
        if st is None:
            st = self._collect_graphs[key] = {'eager': 0, 'g': None}
        if st['g'] is None:
            if st['eager'] < 2:
                st['eager'] += 1
                self._collect_body(warm)
                return
            torch.cuda.current_stream(self.device).synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._collect_body(warm)
            st['g'] = g
        st['g'].replay()

    def _collect_chunk(self, k, warm):
        """The chunked collector: k vector steps in ONE launch (HipVecEnv.rollout_sac_collect), launched directly — there is nothing
        for a graph to join.  Its action noise is addressed by the envs' own episode / step counters (which env_random_state carries):
        `collect_counter` is neither read nor advanced here."""
        buf = self.buffer
        if self._chunk is None or self._chunk['of'] is not buf:
            self._chunk = {'of': buf, 'actor': self.agent.actor_struct(),
                           'c': {u: self.env.sac_collect_struct(buf, self.obs, uniform=u) for u in (False, True)}}
        self.env.rollout_sac_collect(self._chunk['actor'], k, buf, self.obs, struct=self._chunk['c'][bool(warm)])

    def train_step(self, lazy=False):
        """One vectorised env step (+ the gradient steps it owes) — or, with the chunked collector (`collect_steps`), the vector steps
        up to the next point at which the stepwise schedule changes mode or owes an update (chunk_steps), in one launch.  lazy=True: the
        fused update's statistics are not read back ('stats_dev' instead of floats) — with the graph-replayed collector the call then
        never waits for the GPU."""
        cfg = self.cfg
        t0 = time.perf_counter()
        world = parallel.world_size()
        warm = self.total_steps < cfg.warm_up_steps
        k = 1
        if self._collect_k and cfg.train_interval > self.N * world:        # (else every chunk has length 1: the stepwise path)
            k = chunk_steps(self.total_steps, self._since_update, self.N * world, cfg.warm_up_steps, cfg.train_interval, self._collect_k)
            self._collect_chunk(k, warm)
        else:
            self._collect(warm)
        self.buffer.advance_host(k * self.N)
        self.total_steps += k * self.N * world
        self._since_update += k * self.N * world
        results = {}
        if self.total_steps > cfg.warm_up_steps and self._since_update >= cfg.train_interval:
            # the reference locks the ratio of gradient steps to env steps to 1 (sac.py:323-331); with N envs per
            # vectorised step that is N updates per step — `updates_per_step` caps it (documented deviation knob)
            n_updates = int(cfg.extra.get('updates_per_step', self._since_update))
            self._since_update = 0
            results = self.agent.update_from_buffer(self.buffer, cfg.train_batch_size, n_updates, lazy=lazy)
            results['updates'] = n_updates
        results.update({'step': self.total_steps, 'elapsed_time': time.perf_counter() - t0})
        return results

    def learn(self, max_env_steps=None, log=None):
        max_env_steps = max_env_steps or self.cfg.max_env_steps
        hist = []
        while self.total_steps < max_env_steps:
            res = self.train_step()
            hist.append(res)
            if log:
                log(res)
        return hist

    # ---- checkpoint / resume
    def save(self, path, training=True, save_buffer=False):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        state = {'agent': self.agent.state_dict(), 'obs_normalizer': self.obs_normalizer.state_dict(),
                 'reward_normalizer': self.reward_normalizer.state_dict()}            # sac.py:124-128
        for name, nz in (('obs', self.obs_normalizer), ('reward', self.reward_normalizer)):
            if hasattr(nz, 'rms'):              # (upstream's state dict drops the count: a resumed run would re-weight new batches)
                state[f'{name}_normalizer_count'] = float(nz.rms.count)
        if getattr(self.reward_normalizer, 'ret', None) is not None:        # (and the running returns)
            state['reward_normalizer_ret'] = self.reward_normalizer.ret.cpu()
        if training:
            if self._fused_collect:             # counter word of the fused collector's action noise
                state['collect_counter'] = int(self._collect_counter.item())
            state.update({'total_steps': self.total_steps, 'since_update': self._since_update, 'obs': self.obs.cpu(),
                          'random_state': {'torch': torch.get_rng_state(),
                                           'torch_cuda': torch.cuda.get_rng_state(self.device) if self.device.type == 'cuda' else None},
                          'env_random_state': self.env.get_env_random_state()})
            if save_buffer:                     # (upstream's default is off, sac.py:119: the ring is large; on for an exact experiment restore)
                state['buffer'] = self.buffer.state_dict()
            self._save_extra(state)
        torch.save(state, path)

    def load(self, path, training=True):
        state = torch.load(path, map_location=self.device, weights_only=False)
        self.agent.load_state_dict(state['agent'], with_optimizers=training)
        for name, nz in (('obs', self.obs_normalizer), ('reward', self.reward_normalizer)):         # sac.py:147-149
            if state.get(f'{name}_normalizer') and hasattr(nz, 'rms'):
                nz.load_state_dict(state[f'{name}_normalizer'])
                if f'{name}_normalizer_count' in state:
                    nz.rms.count.fill_(state[f'{name}_normalizer_count'])
        if 'reward_normalizer_ret' in state and hasattr(self.reward_normalizer, 'rms'):
            ret = state['reward_normalizer_ret'].to(self.device)
            if self.reward_normalizer.ret is not None and self.reward_normalizer.ret.shape == ret.shape:
                self.reward_normalizer.ret.copy_(ret)               # in place: the collector's graphs alias this tensor
            else:
                self.reward_normalizer.ret = ret
                self._collect_graphs = {}
        if training and 'total_steps' in state:
            self.total_steps = int(state['total_steps'])
            self._since_update = int(state.get('since_update', 0))
            if 'obs' in state:
                self.obs.copy_(state['obs'].to(self.device))              # in place: the collector's graphs alias this tensor
            if self._fused_collect and 'collect_counter' in state:
                self._collect_counter.fill_(int(state['collect_counter']))
            if 'env_random_state' in state:
                self.env.set_env_random_state(state['env_random_state'])
            rs = state.get('random_state')
            if rs:
                torch.set_rng_state(rs['torch'].cpu())
                if rs.get('torch_cuda') is not None and self.device.type == 'cuda':
                    torch.cuda.set_rng_state(rs['torch_cuda'].cpu(), self.device)
            if 'buffer' in state:
                self.buffer.load_state_dict(state['buffer'])
            elif self.total_steps > self.cfg.warm_up_steps:
                self._resumed_without_ring()
            self._load_extra(state)
        return state

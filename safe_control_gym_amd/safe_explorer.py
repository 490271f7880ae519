"""Safe-Explorer PPO (safety layer of Dalal et al. 2018) on the HIP rollout engine.

Mirrors /root/reference/safe_control_gym/controllers/safe_explorer/:
  safe_explorer_utils.py:15-176   SafetyLayer: one MLP g_i(obs) per state constraint with  c_i' ~ c_i + g_i(obs)·a ,
                                  closed-form projection  a* = a - lambda* g_i*  for the most violated constraint
  safe_explorer_utils.py:179-299  ConstraintBuffer
  safe_ppo.py:196-296,425-449     pre-training on random-action transitions (c, c_next with the TERMINAL constraint values
                                  for finished episodes)
  safe_ppo.py:299-345             train_step: the constraint values `c` of the current state are a policy input; the
                                  layer filters the MEAN of the action distribution (safe_ppo_utils.py:88-110)
What the env kernel provides: `c_values` of every step (pre-reset values where the episode ended — exactly upstream's
`terminal_info['constraint_values']`); the constraint values of a freshly reset env are evaluated from the returned state
by `EnvSpec.state_constraint_values`.

Fused collector (opt-in with cfg.extra['fused_rollout']): on an env built with HipVecEnv(..., policy=(hidden, activation),
safety_layer=Hc) the T control steps — actor mean, safety-layer projection, sampling, env step and the next step's constraint values —
are ONE scg_rollout_safe launch, followed by one batched critic pass and the usual bootstrap / GAE.  `evaluate` runs the deterministic
kernel on an evaluation env that carries the same shape.  Unservable shapes and running normalisers warn and keep the eager path.
"""
import time
import warnings

import torch
import torch.nn as nn
import torch.nn.functional as F

from safe_control_gym_amd import parallel
from safe_control_gym_amd.ppo import MLP, PPO, PPOConfig, normalise_advantages


class SafetyLayer:
    def __init__(self, obs_dim, act_dim, num_constraints, hidden_dim=64, lr=1e-3, slack=0.05, device='cpu'):
        hidden = [hidden_dim] if isinstance(hidden_dim, int) else list(hidden_dim)
        self.num_constraints = int(num_constraints)
        self.device = torch.device(device)
        self.constraint_models = nn.ModuleList([MLP(obs_dim, act_dim, hidden) for _ in range(self.num_constraints)]).to(self.device)
        if isinstance(slack, (int, float)):
            slack = [slack] * self.num_constraints
        self.slack = torch.as_tensor(slack, dtype=torch.float32, device=self.device)
        self.optimizers = [torch.optim.Adam(m.parameters(), lr=lr) for m in self.constraint_models]
        self._flat = None                        # flat storage of the fused update (flatten()); None: the plain eager layer

    # ---- flat storage + the fused update (include/scg_safe_pretrain.h): opt-in, the eager methods keep working on the same parameters
    def flatten(self, lib=None):
        """Move the parameters into ONE [C][P] float32 buffer (per constraint: W1 | b1 | W2 | b2, the optimisers' parameter order) with the
        nn.Parameters as views into it, next to flat Adam moments and step counts: what scg_safety_update reads and writes.  `lib` is the
        bound saferoll library of this shape (update_fused needs it).  One hidden layer only."""
        models = self.constraint_models
        if any(len(m.fcs) != 2 for m in models):
            raise ValueError('flat storage serves safety layers with one hidden layer')
        if self._flat is None:
            P = sum(p.numel() for p in models[0].parameters())
            f = dict(dtype=torch.float32, device=self.device)
            buf = torch.zeros(self.num_constraints, P, **f)
            with torch.no_grad():
                for i, m in enumerate(models):
                    o = 0
                    for p in m.parameters():                     # fcs.0.weight, fcs.0.bias, fcs.1.weight, fcs.1.bias
                        k = p.numel()
                        buf[i, o:o + k].copy_(p.detach().reshape(-1))
                        p.data = buf[i, o:o + k].view(p.shape)
                        o += k
            self._flat = {'p': buf, 'm': torch.zeros_like(buf), 'v': torch.zeros_like(buf), 'steps': torch.zeros(self.num_constraints, **f),
                          'lib': None, 'moments': 'opt'}         # 'moments': which side holds the current Adam state
        if lib is not None:
            self._flat['lib'] = lib
        return self

    def _offsets(self, i):
        o = 0
        for p in self.constraint_models[i].parameters():
            yield p, o, p.numel()
            o += p.numel()

    def _moments_to_optimizers(self):
        """torch.optim's `state` filled from the flat moments (upstream's checkpoint keys; an optimiser that never stepped stays empty)."""
        fl = self._flat
        steps = fl['steps'].tolist()
        for i, opt in enumerate(self.optimizers):
            if steps[i] <= 0:
                opt.state.clear()
                continue
            for p, o, k in self._offsets(i):
                opt.state[p] = {'step': torch.tensor(float(steps[i])), 'exp_avg': fl['m'][i, o:o + k].view(p.shape).clone(),
                                'exp_avg_sq': fl['v'][i, o:o + k].view(p.shape).clone()}

    def _moments_from_optimizers(self):
        fl = self._flat
        for i, opt in enumerate(self.optimizers):
            n_steps = 0.0
            for p, o, k in self._offsets(i):
                st = opt.state.get(p)
                if not st:
                    fl['m'][i, o:o + k].zero_()
                    fl['v'][i, o:o + k].zero_()
                    continue
                fl['m'][i, o:o + k].copy_(st['exp_avg'].reshape(-1))
                fl['v'][i, o:o + k].copy_(st['exp_avg_sq'].reshape(-1))
                n_steps = float(st['step'])
            fl['steps'][i] = n_steps

    def update_fused(self, buffer, rows, batch, train=True, grad=None, check_rows=True):
        """rows.numel() // batch minibatches of update() (train) or compute_loss() (not train) in ONE scg_safety_update launch: `buffer` a
        ConstraintBuffer (or its dict of ring tensors), `rows` an int32 device tensor of ring rows, minibatch k = rows[k * batch:(k + 1) *
        batch].  Every entry must be a valid ring row: the kernel does not check, so this method does (one read-back) unless the caller
        vouches for them with check_rows=False (a permutation of the filled rows).  Returns the losses [n_batches, C], each under the
        parameters before that minibatch's step.  grad: an optional [C, P] float32 tensor for the last minibatch's gradient."""
        import ctypes as C
        from safe_control_gym_amd import _lib as L
        from safe_control_gym_amd import _safe_explorer
        fl = self._flat
        if fl is None or fl['lib'] is None:
            raise L.ScgError('SafetyLayer.update_fused needs flatten(lib) with the bound saferoll library of this shape')
        data = buffer.data if hasattr(buffer, 'data') else buffer
        batch = int(batch)
        if rows.dtype != torch.int32 or not rows.is_contiguous() or rows.device != fl['p'].device or batch < 1 or rows.numel() < batch:
            raise ValueError('rows must be a contiguous int32 tensor on the layer device holding at least one minibatch')
        n_batches = rows.numel() // batch
        if check_rows and not (0 <= int(rows.min()) and int(rows.max()) < data['obs'].shape[0]):
            raise ValueError(f'rows must lie in [0, {data["obs"].shape[0]})')
        if not (data['act'].shape[0] == data['c'].shape[0] == data['c_next'].shape[0] == data['obs'].shape[0]):
            raise ValueError('the ring arrays must have the same number of rows')
        obs_dim, act_dim = data['obs'].shape[1], data['act'].shape[1]
        shape = _safe_explorer.shape_of(fl['lib'])
        hc = self.constraint_models[0].fcs[0].out_features
        if (shape[0], shape[1], shape[4], shape[5]) != (self.num_constraints, hc, act_dim, obs_dim) or \
                fl['p'].shape[1] != _safe_explorer.flat_words(obs_dim, act_dim, hc) or data['c'].shape[1] != self.num_constraints:
            raise ValueError('the bound library was built for another (C, Hc, act_dim, obs_dim)')
        for t in (data['obs'], data['act'], data['c'], data['c_next']) + ((grad,) if grad is not None else ()):
            if t.dtype != torch.float32 or not t.is_contiguous() or t.device != fl['p'].device:
                raise ValueError('the ring arrays (and grad) must be contiguous float32 tensors on the layer device')
        if grad is not None and grad.shape != fl['p'].shape:
            raise ValueError(f'grad must be {tuple(fl["p"].shape)}')
        if train and fl['moments'] == 'opt':
            self._moments_from_optimizers()
        loss = torch.empty(n_batches, self.num_constraints, dtype=torch.float32, device=fl['p'].device)
        a = _safe_explorer.SafetyUpdateArgs()
        p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
        a.d_params, a.d_m, a.d_v, a.d_steps = p(fl['p']), p(fl['m']), p(fl['v']), p(fl['steps'])
        a.d_obs, a.d_act, a.d_c, a.d_c_next, a.d_rows = p(data['obs']), p(data['act']), p(data['c']), p(data['c_next']), p(rows)
        a.n_batches, a.batch, a.lr, a.train = n_batches, batch, float(self.optimizers[0].param_groups[0]['lr']), int(bool(train))
        a.d_loss, a.d_grad = p(loss), (p(grad) if grad is not None else None)
        with torch.cuda.device(fl['p'].device):
            L.check(fl['lib'].scg_safety_update(C.byref(a), C.c_void_p(torch.cuda.current_stream(fl['p'].device).cuda_stream)), fl['lib'])
        if train:
            fl['moments'] = 'flat'
        return loss

    def g(self, obs):
        """[B, C, A]: the learned sensitivities of every constraint to the action."""
        return torch.stack([m(obs) for m in self.constraint_models], dim=1)

    def compute_loss(self, batch):
        """Per-constraint L2 loss of the one-step linear model (safe_explorer_utils.py:89-108)."""
        pred = batch['c'] + (self.g(batch['obs']) * batch['act'][:, None, :]).sum(-1)
        return ((batch['c_next'] - pred) ** 2).mean(0)                    # [C]

    def update(self, batch):
        if self._flat is not None and self._flat['moments'] == 'flat':      # fused steps came first: the optimisers continue from them
            self._moments_to_optimizers()
            self._flat['moments'] = 'opt'
        losses = self.compute_loss(batch)
        for opt in self.optimizers:
            opt.zero_grad()
        losses.sum().backward()                  # disjoint parameters: the same gradients as C separate backward passes
        for opt in self.optimizers:
            opt.step()
        return losses.detach()

    def get_safe_action(self, obs, act, c):
        """Eq. (5)-(6) of Dalal et al. 2018 for the constraint with the largest multiplier (safe_explorer_utils.py:120-176)."""
        g = self.g(obs)                                                    # [B, C, A]
        numer = (g * act[:, None, :]).sum(-1) + c + self.slack             # [B, C]
        denom = (g * g).sum(-1) + 1e-8
        mult = F.relu(numer / denom)
        max_mult, max_idx = mult.max(dim=-1)                               # (topk(., 1))
        max_g = g[torch.arange(g.shape[0], device=g.device), max_idx]      # [B, A]
        return act - max_mult[:, None] * max_g

    def state_dict(self):
        """Upstream's keys either way: with flat storage the fused Adam moments travel in torch.optim's layout (ddpg.DDPGAgent's precedent),
        so that a fused run resumes eagerly and an eager run resumes fused."""
        if self._flat is not None and self._flat['moments'] == 'flat':
            self._moments_to_optimizers()
        return {'constraint_models': self.constraint_models.state_dict(), 'optimizers': [o.state_dict() for o in self.optimizers]}

    def load_state_dict(self, sd):
        self.constraint_models.load_state_dict(sd['constraint_models'])      # (in place: the flat buffer, when there is one, follows)
        for o, s in zip(self.optimizers, sd.get('optimizers', [])):
            o.load_state_dict(s)
            for st in o.state.values():
                if torch.is_tensor(st.get('step')):
                    st['step'] = st['step'].cpu()
        if self._flat is not None and sd.get('optimizers'):
            self._flat['moments'] = 'opt'                                    # read back into the flat moments by the next fused update


class ConstraintBuffer:
    """Device ring of (obs, act, c, c_next) transitions."""

    def __init__(self, capacity, obs_dim, act_dim, num_constraints, device):
        f = dict(device=device, dtype=torch.float32)
        self.capacity = int(capacity)
        self.data = {'obs': torch.zeros(self.capacity, obs_dim, **f), 'act': torch.zeros(self.capacity, act_dim, **f),
                     'c': torch.zeros(self.capacity, num_constraints, **f), 'c_next': torch.zeros(self.capacity, num_constraints, **f)}
        self.pos, self.size = 0, 0

    def push(self, **items):
        n = items['obs'].shape[0]
        idx = (torch.arange(n, device=items['obs'].device) + self.pos) % self.capacity
        for k, v in items.items():
            self.data[k][idx] = v
        self.pos = (self.pos + n) % self.capacity
        self.size = min(self.size + n, self.capacity)

    def sampler(self, batch_size, generator=None):
        """Shuffled minibatches, drop last (ppo_utils.random_sample)."""
        perm = torch.randperm(self.size, device=self.data['obs'].device, generator=generator)
        for k in range(self.size // batch_size):
            idx = perm[k * batch_size:(k + 1) * batch_size]
            yield {name: t[idx] for name, t in self.data.items()}


class SafeExplorerPPO(PPO):
    def __init__(self, env, cfg: PPOConfig, seed=0, constraint_hidden_dim=64, constraint_lr=1e-3, constraint_slack=0.05,
                 constraint_batch_size=4096, constraint_buffer_size=1_000_000):
        self.C = env.spec.n_state_con_rows
        if self.C == 0:
            raise ValueError('Safe-Explorer needs an env with state constraints')
        cfg.extra = dict(cfg.extra, cuda_graphs=False)        # the safety layer sits inside the actor: collected eagerly
        super().__init__(env, cfg, seed)
        self.safety_layer = SafetyLayer(self.obs_dim, self.act_dim, self.C, constraint_hidden_dim, constraint_lr,
                                        constraint_slack, self.device)
        self.agent.ac.actor.action_modifier = self.safety_layer.get_safe_action
        self.constraint_batch_size = int(constraint_batch_size)
        self.constraint_buffer = ConstraintBuffer(constraint_buffer_size, self.obs_dim, self.act_dim, self.C, self.device)
        self.c_buf = torch.zeros(self.T, self.N, self.C, device=self.device)
        # per-step outputs incl. the env.state copy (needed for the constraint values of freshly reset envs)
        self._slots = [env.bind_outputs(obs=self.obs[t + 1], reward=self.rew[t], done=self.done[t], flags=self.flags[t],
                                        terminal_obs=self.term_obs[t], noisy_action=None, mse=None) for t in range(self.T)]
        self.obs[0].copy_(self.obs_normalizer(env.reset_tensors()))
        self.c = self._reset_c(env.out)
        self._setup_fused(constraint_hidden_dim)
        self._setup_fused_pretrain(constraint_hidden_dim)

    def _setup_fused_pretrain(self, hidden_c):
        """The fused pre-training phase when cfg.extra['fused_pretrain'] is set: one scg_collect_constraints launch per
        collection, one scg_safety_update launch for all minibatches of an epoch.  Needs an env on the saferoll library of this shape, a
        servable safety layer, no running normaliser and a ring that holds at least one step of every env; otherwise (when asked for) one
        warning and the eager path."""
        from safe_control_gym_amd import _safe_explorer
        self._fused_pretrain = False
        if not self.cfg.extra.get('fused_pretrain'):
            return
        hc = hidden_c[0] if isinstance(hidden_c, (list, tuple)) and len(hidden_c) == 1 else hidden_c
        shape = getattr(self.env, 'safety_shape', None)
        ok = (isinstance(hc, int) and shape is not None and shape[2] == hc and not self._normalise
              and self.env.dtype == torch.float32 and self.constraint_buffer.capacity >= self.N
              and _safe_explorer.supported_pretrain(self.obs_dim, self.act_dim, self.C, hc))
        if not ok:
            warnings.warn(f'SafeExplorerPPO: no fused pre-training for env shape {shape} / safety hidden width {hidden_c} (normalisers: '
                          f'{bool(self._normalise)}, ring {self.constraint_buffer.capacity} rows for {self.N} envs); using the eager '
                          'pre-training', RuntimeWarning, stacklevel=3)
            return
        self.safety_layer.flatten(self.env._lib)
        self._fused_pretrain = True
        self._pre_last_obs = torch.zeros(self.N, self.obs_dim, device=self.device)

    def _collect_constraint_data_fused(self, num_steps):
        """collect_constraint_data as ONE scg_collect_constraints launch (more only when the ring holds fewer rows than the request)."""
        env, buf = self.env, self.constraint_buffer
        env.reset_tensors()
        self.c = self._reset_c(env.out)
        carry = self._carry()
        left = -(-int(num_steps) // (self.N * parallel.world_size()))
        per = buf.capacity // self.N
        while left > 0:
            k = min(left, per)
            env.collect_constraints(k, buf.data, buf.pos, carry, self._pre_last_obs)
            buf.pos = (buf.pos + k * self.N) % buf.capacity
            buf.size = min(buf.size + k * self.N, buf.capacity)
            left -= k
        self.obs[0].copy_(self._pre_last_obs)

    def _fused_minibatches(self, batch_size, train):
        """One pass of shuffled minibatches over the buffer (ConstraintBuffer.sampler's permutation, last partial minibatch dropped) as
        ONE scg_safety_update launch.  Returns the mean per-constraint losses as a [C] tensor."""
        buf = self.constraint_buffer
        bs = min(int(batch_size), buf.size)
        k = buf.size // bs if bs > 0 else 0
        if k == 0:
            return torch.zeros(self.C, device=self.device)
        perm = torch.randperm(buf.size, device=self.device)
        losses = self.safety_layer.update_fused(buf, perm[:k * bs].to(torch.int32).contiguous(), bs, train=train, check_rows=False)
        if train:                                   # kernel writes do not bump the parameters' version counters
            self._safety_packed = None
        return losses.sum(0) / k

    def _setup_fused(self, hidden_c):
        """The fused collector when cfg.extra['fused_rollout'] is set, the env carries the matching (hidden, activation, Hc) shape and
        no running normaliser is on; otherwise (when asked for) a warning and the eager collector."""
        from safe_control_gym_amd import _safe_explorer
        self._fused_safe = None
        if not self.cfg.extra.get('fused_rollout'):
            return
        hc = hidden_c[0] if isinstance(hidden_c, (list, tuple)) and len(hidden_c) == 1 else hidden_c
        shape = (self.cfg.hidden_dim, self.cfg.activation, hc) if isinstance(hc, int) else None
        ok = (shape is not None and getattr(self.env, 'safety_shape', None) == shape and not self._normalise
              and _safe_explorer.supported(self.obs_dim, self.cfg.hidden_dim, self.act_dim, self.cfg.activation, self.C, hc))
        if not ok:
            warnings.warn(f'SafeExplorerPPO: no fused collector for env shape {getattr(self.env, "safety_shape", None)} / wanted '
                          f'{(self.cfg.hidden_dim, self.cfg.activation, hidden_c)} (normalisers: {bool(self._normalise)}); using the eager '
                          'collector', RuntimeWarning, stacklevel=3)
            return
        self._fused_safe = shape
        self._f_episode_acc = torch.zeros(self.N, 8, device=self.device)
        self._safety_packed = None
        self._safety_version = None

    def _packed_safety(self):
        """The packed safety layer (_safe_explorer.pack_safety_layer), re-packed whenever a parameter of the layer has changed since."""
        from safe_control_gym_amd import _safe_explorer
        params = list(self.safety_layer.constraint_models.parameters())
        version = tuple((p.data_ptr(), p._version) for p in params)
        if self._safety_packed is None or version != self._safety_version:
            self._safety_packed = _safe_explorer.pack_safety_layer(self.safety_layer.constraint_models, self.obs_dim, self.act_dim,
                                                                   self._fused_safe[2])
            self._safety_version = version
        return self._safety_packed

    def _carry(self):
        """self.c as the kernel's in/out carry: a contiguous float32 [N, C] tensor on the env device."""
        if self.c.dtype != torch.float32 or not self.c.is_contiguous() or self.c.device != self.device:
            self.c = self.c.to(self.device, torch.float32).contiguous()
        return self.c

    @torch.no_grad()
    def _collect_fused(self, count_steps=True):
        """One scg_rollout_safe launch for the T control steps (obs / act / logp / rew / done / flags / term_obs / c_buf, self.c carried),
        then one batched critic pass for the values; the bootstrap and GAE follow in _returns_body."""
        from safe_control_gym_amd import _adversarial
        T, N = self.T, self.N
        self.env.rollout_safe(_adversarial.actor_ptrs(self.agent.ac.actor), self._packed_safety(), self.safety_layer.slack, T, self.obs,
                              self.act, self.logp, self.rew, self.done, self.flags, self.c_buf, self._carry(), terminal_obs=self.term_obs,
                              episode_acc=self._f_episode_acc)
        self._ep_tot += self._f_episode_acc[:, :4].sum(0)
        self._f_episode_acc.zero_()
        self.v.copy_(self.agent.ac.critic(self.obs[:T].reshape(T * N, self.obs_dim)).reshape(T, N))
        if count_steps:
            self.total_steps += T * N * parallel.world_size()

    def _reset_c(self, out, env=None):
        return (env or self.env).spec.state_constraint_values(out.state.t()).to(torch.float32)

    def _next_c(self, out, env=None):
        """c of the NEXT policy step and c_next of THIS transition (terminal values where the episode ended)."""
        c_step = out.c_values[:self.C].t().to(torch.float32)
        done = out.done.bool()
        c_now = torch.where(done[:, None], self._reset_c(out, env), c_step) if bool((env or self.env).auto_reset) else c_step
        return c_now, c_step

    # ---- pre-training of the constraint models (safe_ppo.py:196-296, :425-449)
    def collect_constraint_data(self, num_steps):
        if self._fused_pretrain:
            return self._collect_constraint_data_fused(num_steps)
        env = self.env
        low = torch.as_tensor(env.spec.action_space.low, dtype=torch.float32, device=self.device)
        high = torch.as_tensor(env.spec.action_space.high, dtype=torch.float32, device=self.device)
        obs = self.obs_normalizer(env.reset_tensors()).clone()
        c = self._reset_c(env.out)
        steps = 0
        while steps < num_steps:
            act = low + (high - low) * torch.rand(self.N, self.act_dim, device=self.device)
            out = env.step_tensors(act)
            c_now, c_next = self._next_c(out)
            self.constraint_buffer.push(obs=obs, act=act, c=c, c_next=c_next)
            obs, c = self.obs_normalizer(out.obs).clone(), c_now
            steps += self.N * parallel.world_size()
        self.obs[0].copy_(obs)
        self.c = c

    def pretrain_step(self, steps_per_epoch, batch_size=None):
        """One epoch of upstream's pre-training (safe_ppo.py:281-297): fresh random-action transitions, one pass of shuffled
        minibatches over them, buffer cleared.  Returns the mean per-constraint losses."""
        self.obs_normalizer.unset_read_only()
        self.collect_constraint_data(steps_per_epoch)
        if self._fused_pretrain:
            mean = self._fused_minibatches(batch_size or self.constraint_batch_size, train=True)
            self.constraint_buffer.pos = self.constraint_buffer.size = 0
            return mean.tolist()
        bs = min(int(batch_size or self.constraint_batch_size), self.constraint_buffer.size)
        acc, k = torch.zeros(self.C, device=self.device), 0
        for batch in self.constraint_buffer.sampler(bs):
            acc += self.safety_layer.update(batch)
            k += 1
        self.constraint_buffer.pos = self.constraint_buffer.size = 0
        return (acc / max(k, 1)).tolist()

    @torch.no_grad()
    def eval_constraint_models(self, num_steps, batch_size=None):
        """safe_ppo.py:451-466: mean per-constraint loss on freshly collected random-action data, statistics frozen, no update."""
        frozen = self.obs_normalizer.read_only
        self.obs_normalizer.set_read_only()
        self.collect_constraint_data(num_steps)
        self.obs_normalizer.read_only = frozen
        if self._fused_pretrain:
            mean = self._fused_minibatches(batch_size or self.constraint_batch_size, train=False)
            self.constraint_buffer.pos = self.constraint_buffer.size = 0
            return mean.tolist()
        bs = min(int(batch_size or self.constraint_batch_size), self.constraint_buffer.size)
        acc, k = torch.zeros(self.C, device=self.device), 0
        for batch in self.constraint_buffer.sampler(bs):
            acc += self.safety_layer.compute_loss(batch)
            k += 1
        self.constraint_buffer.pos = self.constraint_buffer.size = 0
        return (acc / max(k, 1)).tolist()

    @torch.no_grad()
    def evaluate(self, env, episodes_per_env=1):
        """SafeExplorerPPO.run (safe_ppo.py:230-279) batched: the deterministic, safety-filtered policy on every env of `env` with
        the constraint values of the current state as its second input; per-env totals of the first `episodes_per_env` episodes."""
        N, dev = env.num_envs, env.device
        if self._fused_safe is not None and getattr(env, 'safety_shape', None) == self._fused_safe:
            return self._evaluate_fused(env, episodes_per_env)
        acc = {k: torch.zeros(N, device=dev) for k in ('count', 'ret', 'length', 'viol', 'mse')}
        nz = self.obs_normalizer
        frozen = nz.read_only
        nz.set_read_only()
        obs = nz(env.reset_tensors())
        c = self._reset_c(env.out, env)
        for _ in range(env.spec.max_episode_steps * episodes_per_env):
            out = env.step_tensors(self.agent.ac.act(obs, c))
            df = (out.done.bool() & (acc['count'] < episodes_per_env)).to(torch.float32)
            acc['ret'] += out.fin_return * df
            acc['length'] += out.fin_length * df
            acc['viol'] += out.fin_violation * df
            acc['mse'] += out.fin_mse * df
            acc['count'] += df
            c, _ = self._next_c(out, env)
            obs = nz(out.obs)
        nz.read_only = frozen
        return acc

    @torch.no_grad()
    def _evaluate_fused(self, env, episodes_per_env=1):
        """evaluate() as ONE scg_rollout_safe launch with the filtered mean (deterministic=1); per-env totals of the first
        `episodes_per_env` episodes accumulated in the kernel."""
        from safe_control_gym_amd import _adversarial
        N, dev = env.num_envs, env.device
        steps = env.spec.max_episode_steps * episodes_per_env
        buf = getattr(env, '_eval_safe', None)
        if buf is None or buf['rew'].shape[0] != steps:
            f = dict(device=dev, dtype=torch.float32)
            u8 = dict(device=dev, dtype=torch.uint8)
            buf = {'obs': torch.zeros(steps + 1, N, self.obs_dim, **f), 'act': torch.zeros(steps, N, self.act_dim, **f),
                   'logp': torch.zeros(steps, N, **f), 'rew': torch.zeros(steps, N, **f), 'done': torch.zeros(steps, N, **u8),
                   'flags': torch.zeros(steps, N, **u8), 'c_rows': torch.zeros(steps, N, self.C, **f), 'acc': torch.zeros(N, 8, **f)}
            env._eval_safe = buf
        env.reset_tensors()
        carry = self._reset_c(env.out, env).contiguous()
        buf['acc'].zero_()
        env.rollout_safe(_adversarial.actor_ptrs(self.agent.ac.actor), self._packed_safety(), self.safety_layer.slack, steps, buf['obs'],
                         buf['act'], buf['logp'], buf['rew'], buf['done'], buf['flags'], buf['c_rows'], carry, deterministic=True,
                         episode_acc=buf['acc'], max_episodes=episodes_per_env)
        a = buf['acc']
        return {'count': a[:, 0], 'ret': a[:, 1], 'length': a[:, 2], 'viol': a[:, 3], 'mse': a[:, 4]}

    # ---- checkpoints with upstream's keys (safe_ppo.py:146-176): agent, safety_layer, normalisers
    def checkpoint_state(self, training=True):
        state = super().checkpoint_state(training)
        state['safety_layer'] = self.safety_layer.state_dict()
        if training:
            state['c'] = self.c.cpu()
            # upstream saves `total_steps`, which in the pre-training phase IS the epoch count (safe_ppo.py:146-160, :178-213);
            # here total_steps counts env steps of the PPO phase, so the pre-training progress travels under its own key
            state['pretrain_steps'] = int(getattr(self, 'pretrain_steps', 0))
        return state

    def load(self, path, training=True):
        state = torch.load(path, map_location='cpu', weights_only=False)
        super().load(path, training)
        self.load_safety_layer(state)
        if training and 'c' in state:
            self.c = state['c'].to(self.device)
        if training:
            self.pretrain_steps = int(state.get('pretrain_steps', 0))

    def load_safety_layer(self, state_or_path):
        """The `pretrained` hand-over of the second phase (safe_ppo.py:96-100): only the safety layer of a checkpoint."""
        import os
        if isinstance(state_or_path, (str, os.PathLike)):
            p = os.fspath(state_or_path)
            if os.path.isdir(p):
                p = os.path.join(p, 'model_latest.pt')
            state_or_path = torch.load(p, map_location='cpu', weights_only=False)
        self.safety_layer.load_state_dict(state_or_path['safety_layer'])

    def pretrain(self, num_steps, epochs=5):
        self.collect_constraint_data(num_steps)
        hist = []
        for _ in range(epochs):
            if self._fused_pretrain:
                hist.append(self._fused_minibatches(self.constraint_batch_size, train=True).tolist())
                continue
            acc, k = torch.zeros(self.C, device=self.device), 0
            for batch in self.constraint_buffer.sampler(min(self.constraint_batch_size, self.constraint_buffer.size)):
                acc += self.safety_layer.update(batch)
                k += 1
            hist.append((acc / max(k, 1)).tolist())
        return hist

    # ---- rollout with the constraint values as policy input (safe_ppo.py:299-345)
    def _collect_body(self):
        ac, env = self.agent.ac, self.env
        c = self.c
        for t in range(self.T):
            self.c_buf[t] = c
            act, v, logp = ac.step(self.obs[t], c)
            self.act[t], self.v[t], self.logp[t] = act, v, logp
            out, c_out = self._slots[t]
            env.step_tensors(self.act[t], out=out, c_out=c_out)
            if self._normalise:
                self.obs[t + 1].copy_(self.obs_normalizer(self.obs[t + 1]))
                self.rew[t].copy_(self.reward_normalizer(self.rew[t], self.done[t]))
            c, _ = self._next_c(out)
            d = self.done[t].to(torch.float32)
            self.ep_count += d.sum()
            self.ep_return_sum += (out.fin_return * d).sum()
            self.ep_length_sum += (out.fin_length * d).sum()
            self.ep_violation_sum += (out.fin_violation * d).sum()
        self.c = c

    def train_step(self):
        t0 = time.perf_counter()
        if self._fused_safe is not None:
            self._collect_fused()
        else:
            self.collect()
        ret, adv, moments = self._returns_body(dense=False)
        with torch.no_grad():
            parallel.all_reduce_sum_(moments)
            adv = normalise_advantages(adv, moments)
        M = self.T * self.N
        data = {'obs': self.obs[:self.T].reshape(M, self.obs_dim), 'act': self.act.reshape(M, self.act_dim),
                'logp': self.logp.reshape(M), 'adv': adv.reshape(M), 'ret': ret.reshape(M), 'v': self.v.reshape(M),
                'c': self.c_buf.reshape(M, self.C)}
        res = self.agent.update(data)
        self.obs[0].copy_(self.obs[self.T])
        res.update({'step': self.total_steps, 'elapsed_time': time.perf_counter() - t0})
        return res

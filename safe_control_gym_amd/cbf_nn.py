"""The reference's CBF-QP safety filter with a learned Lie-derivative residual (safety_filters/cbf/cbf_nn.py) on the HIP engine.

    sf = make('cbf_nn', env_func, **sf_config)                     # registration.py; defaults = safety_filters/cbf/cbf_nn.yaml
    sf.uncertified_controller = ctrl                               # a `ppo` controller, or None: action_space.sample()
    sf.learn(num_envs=256)
    certified, success = sf.certify_action(state, uncertified_action)
    ctrl.run(safety_filter=sf)

With (a_nn, b_nn) = mlp(X) the reference's barrier row is  -slope h - LfV(X, u) - (a_nn u + b_nn) <= s.  LfV is affine in u, so this is
the plain filter's QP with k' = k + b_nn and b' = b + a_nn and the same closed-form minimiser (include/scg_cbf_nn.h).  The residual
network's forward pass and the QP are ONE kernel: `scg_cbf_nn_certify` serves a batch of rows (certify_action, certify_tensors, is_cbf,
extract_a_b), `scg_rollout_cbf_nn` puts both between PPO's actor and the env step (learn's episodes, evaluation).  The update of the
network is upstream's: `train_iterations` small Adam steps of `compute_loss` per episode, in PyTorch — or, with the extension key
`fused_update=True` (not a YAML default, off by default), one `scg_cbf_nn_update` call per episode (include/scg_cbf_nn_update.h): the
same minibatches and the same Adam rule on the device, whose float32 sums run in another order than PyTorch's, so that the same seed
gives weights that differ in the last places.

Differences from upstream a caller can see, beyond cbf.py's:
  * `hidden_dims` must be [256, 256] (the shape the kernels serve); anything else raises NotImplementedError.
  * `learn(num_envs=n)` runs every episode on n envs side by side (an extension key, not a YAML default; n = 1 is upstream's sample
    count): each env contributes its own max_num_steps - 2 rows, env after env.
  * upstream blends the controller's raw action (the env's action space) with the certified PHYSICAL input (cbf_nn.py:349) and hands
    the sum to env.step; the two live in different spaces when the action space is normalised.  Here the blend is formed in the env's
    action space, (1 - w) a + w u* / act_scale, and the buffer's `act` and the Lie derivative receive the physical input act_scale x
    that.  With normalized_rl_action_space False (the reference example) all of these coincide with upstream's.
  * the buffer keeps CBFBuffer's bookkeeping, including `buffer_size = min(max_size, pos + n)` taken AFTER `pos` has advanced
    (cbf_utils.py:193-195): after a first push of n rows, 2 n rows count as filled and the zero rows among them are sampled.
  * batches are drawn from a generator seeded with the filter's seed (upstream: NumPy's global state).
"""
import os

import numpy as np

from safe_control_gym_amd import _lib as L
from safe_control_gym_amd.cbf import CBF, CBF_DEFAULTS

# safety_filters/cbf/cbf_nn.yaml
CBF_NN_DEFAULTS = dict(CBF_DEFAULTS, max_num_steps=250, hidden_dims=[256, 256], learning_rate=0.001, num_episodes=20, max_buffer_size=1.0e6,
                       train_batch_size=64, train_iterations=200)
SERVED_HIDDEN_DIMS = [256, 256]


def barrier_terms(X, limits, prior):
    """(h, a, b) of float64 device states [n, 4]: the barrier, LfV(X, 0) and LfV(X, 1) - LfV(X, 0) of AnalyticModel's cartpole
    (symbolic.py; cbf_utils.cbf_cartpole); prior = (l, m, M, g)."""
    import torch
    L_ = torch.as_tensor(np.asarray(limits, dtype=np.float64), device=X.device)
    l, m, M, g = (float(v) for v in prior)
    q = X / L_
    h = 1.0 - (q * q).sum(dim=1)
    gr = -2.0 * X / (L_ * L_)
    sn, cs = torch.sin(X[:, 2]), torch.cos(X[:, 2])
    Mm, ml = m + M, m * l
    tmp0 = ml * X[:, 3] * X[:, 3] * sn / Mm
    den = l * (4.0 / 3.0 - m * cs * cs / Mm)
    thdd0 = (g * sn - cs * tmp0) / den
    xdd0 = tmp0 - ml * thdd0 * cs / Mm
    dtmp = 1.0 / Mm
    dthdd = -cs * dtmp / den
    dxdd = dtmp - ml * dthdd * cs / Mm
    a = gr[:, 0] * X[:, 1] + gr[:, 1] * xdd0 + gr[:, 2] * X[:, 3] + gr[:, 3] * thdd0
    b = gr[:, 1] * dxdd + gr[:, 3] * dthdd
    return h, a, b


def pushed_arrays(states, inputs, limits, prior, ctrl_freq):
    """The four arrays cbf_nn.py:357-380 push for a trace, on the device in float64: `states` [K, n, 4] the state AFTER each step,
    `inputs` [K, n] the physical input that produced it.  Upstream's indexing: the first and the last step are dropped, the symmetric
    difference of the barrier over 2 / CTRL_FREQ pairs with the middle step.  Returns state [n (K - 2), 4], act, barrier_dot,
    barrier_dot_approx [n (K - 2), 1], env after env."""
    import torch
    K, n = inputs.shape
    X = states.to(torch.float64).reshape(K * n, 4)
    u = inputs.to(torch.float64).reshape(K * n)
    h, a, b = barrier_terms(X, limits, prior)
    h, lie = h.reshape(K, n), (a + b * u).reshape(K, n)
    approx = (h[2:] - h[:-2]) / (2 * 1 / ctrl_freq)
    env_major = lambda t: t.transpose(0, 1).reshape(n * (K - 2), -1)        # noqa: E731
    return (env_major(states[1:-1].to(torch.float64)), env_major(inputs[1:-1].to(torch.float64).unsqueeze(-1)),
            env_major(lie[1:-1].unsqueeze(-1)), env_major(approx.unsqueeze(-1)))


class DeviceCBFBuffer:
    """cbf_utils.CBFBuffer as a device ring: the same keys, `pos` / `buffer_size` bookkeeping and wrap-around.  `state` and `act` are
    float32 (upstream's dtype), `barrier_dot` and `barrier_dot_approx` float64 (what learn() forms; a batch is cast to float32)."""
    KEYS = ('state', 'act', 'barrier_dot', 'barrier_dot_approx')

    def __init__(self, obs_dim, act_dim, max_size, device, batch_size, seed=0):
        self.max_size, self.batch_size, self.device = int(max_size), int(batch_size), device
        self.widths = {'state': int(obs_dim), 'act': int(act_dim), 'barrier_dot': 1, 'barrier_dot_approx': 1}
        self.rng = np.random.RandomState(seed)
        self.reset()

    def reset(self):
        import torch
        for k, w in self.widths.items():
            dt = torch.float32 if k in ('state', 'act') else torch.float64
            setattr(self, k, torch.zeros(self.max_size, w, dtype=dt, device=self.device))
        self.pos = 0
        self.buffer_size = 0

    def __len__(self):
        return self.buffer_size

    def state_dict(self):
        state = dict(pos=self.pos, buffer_size=self.buffer_size)
        for k in self.KEYS:
            state[k] = getattr(self, k).cpu().numpy()
        return state

    def load_state_dict(self, state):
        import torch
        self.pos, self.buffer_size = int(state['pos']), int(state['buffer_size'])
        for k in self.KEYS:
            t = getattr(self, k)
            t.copy_(torch.as_tensor(np.asarray(state[k])).reshape(t.shape).to(t.dtype))

    def push(self, batch):
        import torch
        n = int(batch[self.KEYS[0]].shape[0])
        if n > self.max_size:
            raise ValueError(f'a push of {n} rows exceeds the buffer ({self.max_size})')
        idx = (self.pos + torch.arange(n, device=self.device)) % self.max_size
        for k in self.KEYS:
            t = getattr(self, k)
            t[idx] = batch[k].reshape(n, t.shape[1]).to(t.dtype)
        self.pos = (self.pos + n) % self.max_size
        if self.buffer_size < self.max_size:
            self.buffer_size = min(self.max_size, self.pos + n)                  # (cbf_utils.py:193-195, kept as it is)

    def sample_indices(self, batch_size=None):
        return self.rng.randint(0, len(self), size=batch_size or self.batch_size)

    def gather(self, indices):
        import torch
        idx = torch.as_tensor(np.asarray(indices), device=self.device, dtype=torch.long)
        return {k: getattr(self, k)[idx].to(torch.float32) for k in self.KEYS}

    def sample(self, batch_size=None):
        return self.gather(self.sample_indices(batch_size))


class CBF_NN(CBF):
    """Neural-network based Control Barrier Function safety filter (cbf_nn.py:19-385)."""

    def __init__(self, env_func, slope=0.1, soft_constrained=True, slack_weight=10000.0, slack_tolerance=1.0e-3, max_num_steps=250,
                 hidden_dims=None, learning_rate=0.001, num_episodes=20, max_buffer_size=1.0e6, train_batch_size=64, train_iterations=200,
                 fused_update=False, **kwargs):
        """fused_update: the Adam steps run in scg_cbf_nn_update (one call per episode).  The flat float32 vector behind residual() is
        then the master copy of the weights and `self.mlp`'s parameters are views into it; the Adam moments and the step count live
        beside it.  They are not checkpointed (save / load carry the weights and the buffer, as upstream's do) and reset() and load()
        leave them alone, as upstream's leave its optimiser."""
        import torch
        from safe_control_gym_amd.ppo import MLP
        hidden_dims = list(SERVED_HIDDEN_DIMS if hidden_dims is None else hidden_dims)
        if [int(v) for v in hidden_dims] != SERVED_HIDDEN_DIMS:
            raise NotImplementedError(f'cbf_nn serves hidden_dims = {SERVED_HIDDEN_DIMS} (the residual network the kernels are built for), got '
                                      f'{hidden_dims}')
        super().__init__(env_func, slope, soft_constrained, slack_weight, slack_tolerance, **kwargs)
        self.max_num_steps, self.hidden_dims, self.learning_rate, self.num_episodes = int(max_num_steps), hidden_dims, learning_rate, int(num_episodes)
        self.max_buffer_size, self.train_batch_size, self.train_iterations = max_buffer_size, int(train_batch_size), int(train_iterations)
        self.fused_update = bool(fused_update)
        if self.fused_update:
            from safe_control_gym_amd import _cbf_nn_update
            if not 1 <= self.train_batch_size <= _cbf_nn_update.MAX_BATCH:
                raise ValueError(f'fused_update serves train_batch_size in [1, {_cbf_nn_update.MAX_BATCH}], got {self.train_batch_size}')
        state = torch.random.get_rng_state()
        torch.manual_seed(self.seed)
        self.mlp = MLP(self.model.nx, self.model.nu + 1, self.hidden_dims, 'relu')
        torch.random.set_rng_state(state)
        self.opt = None if self.fused_update else torch.optim.Adam(self.mlp.parameters(), self.learning_rate)
        self._upd, self.last_losses = None, None             # fused_update: the moments, step count and scratch beside the master vector
        self.buffer = None                                   # allocated on the env's device at first use
        self.uncertified_controller = None
        self._flat = None
        self._learn_env = None
        self.blend_weights, self.sampled_indices, self.last_trace = [], [], None

    # ---- the residual network on the device
    def attach(self, venv):
        """Certify through `venv`'s library (a HipVecEnv built with cbf_nn=True) instead of an env of this filter's own."""
        if getattr(venv, 'cbf_nn_shape', None) is None:
            raise L.ScgError('attach() needs a HipVecEnv built with policy=(hidden, activation), cbf_nn=True')
        self._venv = venv
        return self

    def _env(self):
        if self._venv is None:
            from safe_control_gym_amd.vec_env import HipVecEnv
            self._venv, self._own_venv = HipVecEnv(self.env_id, 1, seed=self.seed, return_numpy=False, policy=self.policy_shape, cbf_nn=True,
                                                   **self.task_config), True
        return self._venv

    def _tensors(self):
        return [t for fc in self.mlp.fcs for t in (fc.weight, fc.bias)]

    def residual(self, device=None):
        """The _cbf_nn.Residual of the current weights: a persistent flat float32 copy (stable pointer), refreshed in place on every call.
        fused_update: the flat vector IS the weights (the network's parameters are views into it); nothing is copied."""
        import torch
        from safe_control_gym_amd import _cbf_nn
        device = self._env().device if device is None else device
        if self.fused_update:
            return _cbf_nn.residual_of(self._master(device))
        if self._flat is None or self._flat.device != device:
            self.mlp.to(device)
            self._flat = torch.empty(sum(_cbf_nn.residual_sizes()), dtype=torch.float32, device=device)
        with torch.no_grad():
            torch.cat([t.detach().reshape(-1) for t in self._tensors()], out=self._flat)
        return _cbf_nn.residual_of(self._flat)

    def _master(self, device):
        """fused_update: the master vector on `device`, the network's six parameters re-pointed into it (once per device)."""
        import torch
        from safe_control_gym_amd import _cbf_nn
        device = torch.empty(0, device=device).device        # ('cuda' and 'cuda:0' are one device: the pointer must stay)
        if self._flat is None or self._flat.device != device:
            with torch.no_grad():
                flat = torch.cat([t.detach().reshape(-1).to(device=device, dtype=torch.float32) for t in self._tensors()])
                off = 0
                for t in self._tensors():
                    t.data = flat[off:off + t.numel()].view(t.shape)
                    off += t.numel()
            assert off == sum(_cbf_nn.residual_sizes())
            self._flat = flat
            if self._upd is not None:
                self._upd = {k: (v.to(device) if hasattr(v, 'to') else v) for k, v in self._upd.items()}
        return self._flat

    def _update_state(self, device):
        """fused_update: Adam's moments and step count (zero at first use) and the kernels' scratch, beside the master vector."""
        import torch
        from safe_control_gym_amd import _cbf_nn_update as U
        flat = self._master(device)
        if self._upd is None:
            D = U.lib()
            self._upd = {'m': torch.zeros_like(flat), 'v': torch.zeros_like(flat), 'step': torch.zeros(1, dtype=torch.float32, device=flat.device),
                         'work': torch.empty(U.work_bytes(D, U.MAX_BATCH) // 4, dtype=torch.float32, device=flat.device)}
        return self._upd

    def _fused_call(self, state, act, barrier_dot, barrier_dot_approx, rows, train=True):
        """One scg_cbf_nn_update call on four ring arrays and an int32 device tensor of rows [n, batch]; returns the n losses."""
        import ctypes as C
        import torch
        from safe_control_gym_amd import _cbf_nn_update as U
        dev = state.device
        up = self._update_state(dev)
        D = U.lib()
        n, batch = int(rows.shape[0]), int(rows.shape[1])
        if not 1 <= batch <= U.MAX_BATCH or n < 1:
            raise ValueError(f'fused_update serves minibatches of 1 to {U.MAX_BATCH} rows, got {n} x {batch}')
        loss = torch.empty(n, dtype=torch.float32, device=dev)
        a = U.UpdateArgs(d_params=self._flat.data_ptr(), d_m=up['m'].data_ptr(), d_v=up['v'].data_ptr(), d_step=up['step'].data_ptr(),
                         d_state=state.data_ptr(), d_act=act.data_ptr(), d_barrier_dot=barrier_dot.data_ptr(),
                         d_barrier_dot_approx=barrier_dot_approx.data_ptr(), d_rows=rows.data_ptr(), n_batches=n, batch=batch,
                         lr=float(self.learning_rate), train=int(bool(train)), d_loss=loss.data_ptr(), d_grad=None, d_work=up['work'].data_ptr())
        U.check(D, D.scg_cbf_nn_update(C.byref(a), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        return loss

    def update_rows(self, indices):
        """fused_update: one Adam step per row of `indices` (int [n, batch] rows of the buffer, duplicates counted as often as they
        occur) in ONE scg_cbf_nn_update call on the buffer's arrays; returns the n losses (each under the weights before its step) as a
        device tensor.  An index outside [0, len(buffer)) raises ValueError before anything is launched."""
        import torch
        if not self.fused_update:
            raise L.ScgError('update_rows() needs a filter made with fused_update=True')
        buf = self.buffer
        if buf is None or getattr(buf.state, 'is_cuda', False) is False:
            raise L.ScgError('update_rows() needs the buffer on the device (learn() or load() after the first launch puts it there)')
        idx = np.asarray(indices)
        if idx.ndim != 2 or idx.size == 0 or not np.issubdtype(idx.dtype, np.integer):
            raise ValueError(f'indices must be a non-empty int array [n, batch], got {idx.dtype} {idx.shape}')
        if idx.min() < 0 or idx.max() >= len(buf):
            raise ValueError(f'indices must lie in [0, {len(buf)}), got [{idx.min()}, {idx.max()}]')
        rows = torch.as_tensor(np.ascontiguousarray(idx, dtype=np.int32)).to(buf.device)
        return self._fused_call(buf.state, buf.act, buf.barrier_dot, buf.barrier_dot_approx, rows)

    def _ensure_buffer(self, device):
        if self.buffer is None or self.buffer.device != device:
            old = self.buffer
            self.buffer = DeviceCBFBuffer(self.model.nx, self.model.nu, self.max_buffer_size, device, self.train_batch_size, self.seed)
            if old is not None:
                self.buffer.load_state_dict(old.state_dict())
        return self.buffer

    # ---- batched certify
    def certify_tensors(self, states, actions, with_ab=False):
        """(certified [n], slack [n], feasible uint8 [n]) device tensors of float32 states [n, 4] and physical actions [n]; with_ab: also
        (a_nn, b_nn) [n, 2]."""
        venv = self._env()
        cert, slack, feas, ab = venv.certify_nn_tensors(self.params(), self.residual(venv.device), states, actions)
        return (cert, slack, feas, ab) if with_ab else (cert, slack, feas)

    # (certify_action and is_cbf are CBF's: they go through certify_tensors, i.e. scg_cbf_nn_certify; the 456 976-state grid is one launch)

    def extract_a_b(self, current_state):
        """cbf_nn.py:206-225: (a [nu], b) of one state — or (a [n, nu], b [n]) of a batch — read from scg_cbf_nn_certify's d_ab."""
        import torch
        venv = self._env()
        s = torch.as_tensor(np.asarray(current_state, dtype=np.float64)).to(device=venv.device, dtype=torch.float32)
        single = s.dim() == 1
        s = s.reshape(-1, 4).contiguous()
        ab = self.certify_tensors(s, torch.zeros(s.shape[0], device=venv.device), with_ab=True)[3].cpu().numpy()
        nu = self.model.nu
        return (ab[0, :nu], ab[0, -1]) if single else (ab[:, :nu], ab[:, -1])

    # ---- the update (cbf_nn.py:227-264)
    def compute_loss(self, batch):
        import torch
        state, act, barrier_dot, barrier_dot_approx = batch['state'], batch['act'], batch['barrier_dot'], batch['barrier_dot_approx']
        a_b = self.mlp(state)
        a = torch.unsqueeze(a_b[:, 0], 1)
        b = torch.unsqueeze(a_b[:, 1], 1)
        h_dot_estimate = barrier_dot + a * act + b
        return (h_dot_estimate - barrier_dot_approx).pow(2).mean()

    def update(self, batch):
        if self.fused_update:                                # (the batch as a ring of its own, rows 0 .. n - 1: the same kernels, the same Adam state)
            import torch
            st = batch['state'].to(torch.float32).reshape(-1, 4).contiguous()
            self.residual(st.device)
            cols = [batch[k].reshape(-1).contiguous() for k in ('act', 'barrier_dot', 'barrier_dot_approx')]
            rows = torch.arange(st.shape[0], dtype=torch.int32, device=st.device).reshape(1, -1)
            self._fused_call(st, cols[0].to(torch.float32), cols[1].to(torch.float64), cols[2].to(torch.float64), rows)
            return
        loss = self.compute_loss(batch)
        self.opt.zero_grad()
        loss.backward()
        self.opt.step()

    # ---- episodes
    def _actor_of(self, controller):
        """ActorPtrs of the uncertified controller's PPO actor (the controller keeps the parameters alive)."""
        from safe_control_gym_amd import _cbf
        if isinstance(controller, L.Policy):                 # (a policy struct: its owner keeps the flat parameters alive)
            pol = controller
        else:
            impl = getattr(controller, 'impl', None)
            if impl is None or not hasattr(impl, '_policy_struct') or getattr(controller, 'norm_obs', False):
                raise L.ScgError('cbf_nn serves a `ppo` controller without observation normalisation in front of the filter: no SAC / DDPG '
                                 'actor (a 256-wide actor and the residual network do not share a register file)')
            pol = impl._policy_struct(True)
        shape = (int(pol.hidden), {v: k for k, v in L.POLICY_ACTS.items()}[int(pol.activation)])
        return _cbf.actor_ptrs_of_policy(pol), shape, pol

    def rollout(self, venv, k_steps, actor=None, deterministic=True, uniform=False, blend=-1.0, episode_acc=None, max_episodes=0):
        """One scg_rollout_cbf_nn launch of k_steps on `venv` with the current weights; returns the trace dict (obs [k + 1, N, nobs], act,
        logp, rew, done, flags, rows [k, N, 4], applied [k, N], ab [k, N, 2])."""
        import torch
        n, nobs, nu = venv.num_envs, venv.spec.obs_dim, venv.spec.nu
        f = dict(device=venv.device, dtype=torch.float32)
        u8 = dict(device=venv.device, dtype=torch.uint8)
        o = {'obs': torch.zeros(k_steps + 1, n, nobs, **f), 'act': torch.zeros(k_steps, n, nu, **f), 'logp': torch.zeros(k_steps, n, **f),
             'rew': torch.zeros(k_steps, n, **f), 'done': torch.zeros(k_steps, n, **u8), 'flags': torch.zeros(k_steps, n, **u8),
             'rows': torch.zeros(k_steps, n, 4, **f), 'applied': torch.zeros(k_steps, n, **f), 'ab': torch.zeros(k_steps, n, 2, **f)}
        venv.rollout_cbf_nn(actor, self.params(), self.residual(venv.device), k_steps, o['obs'], o['act'], o['logp'], o['rew'], o['done'],
                            o['flags'], o['rows'], o['applied'], o['ab'], deterministic=deterministic, uniform=uniform, blend=blend,
                            episode_acc=episode_acc, max_episodes=max_episodes)
        return o

    def learn(self, env=None, num_envs=1, **kwargs):
        """cbf_nn.py:310-385: num_episodes sequential episodes with the blend weight i / (num_episodes - 1); an episode is a reset of all
        envs and ONE launch of max_num_steps control steps (auto_reset off: upstream's loop ignores `done`), then the push of the four
        arrays and train_iterations Adam steps.  env: a HipVecEnv built with policy=(hidden, activation), cbf_nn=True, auto_reset=False
        (default: one of this filter's own with `num_envs` envs)."""
        import torch
        from safe_control_gym_amd.vec_env import HipVecEnv
        if self.max_num_steps < 3:
            raise ValueError('max_num_steps must be at least 3 (the first and the last step are dropped)')
        actor, uniform, keep = None, self.uncertified_controller is None, None
        shape = self.policy_shape
        if not uniform:
            actor, shape, keep = self._actor_of(self.uncertified_controller)
        if env is None:
            if self._learn_env is None or self._learn_env.num_envs != int(num_envs) or self._learn_env.cbf_nn_shape != shape:
                if self._learn_env is not None:
                    self._learn_env.close()
                self._learn_env = HipVecEnv(self.env_id, int(num_envs), seed=self.seed, return_numpy=False, policy=shape, cbf_nn=True,
                                            auto_reset=False, **self.task_config)
            env = self._learn_env
        if getattr(env, 'cbf_nn_shape', None) is None:
            raise L.ScgError('learn() needs a HipVecEnv built with policy=(hidden, activation), cbf_nn=True')
        if env.auto_reset:
            raise L.ScgError('learn() needs an env built with auto_reset=False: upstream\'s episode loop ignores `done`')
        if not uniform and env.cbf_nn_shape != shape:
            raise L.ScgError(f'the env was built for an actor of shape {env.cbf_nn_shape}, the uncertified controller has {shape}')
        buf = self._ensure_buffer(env.device)
        self.residual(env.device)                            # (moves the network to the env's device)
        weights = np.arange(self.num_episodes) / (self.num_episodes - 1) if self.num_episodes > 1 else np.zeros(1)
        scale = float(env.spec.action_scale) if env.spec.NORMALIZED_RL_ACTION_SPACE else 1.0
        prior = (self.model.params['length'], self.model.params['m'], self.model.params['M'], self.model.params['g'])
        self.blend_weights, self.sampled_indices = [], []
        for i in range(self.num_episodes):
            env.reset_tensors()
            o = self.rollout(env, self.max_num_steps, actor=actor, deterministic=True, uniform=uniform, blend=float(weights[i]))
            self.blend_weights.append(float(np.float32(weights[i])))
            self.last_trace = o
            states = o['obs'][1:, :, :4]                     # the state AFTER step c pairs with the input that produced it
            inputs = o['applied'].to(torch.float64) * scale
            state, act, barrier_dot, approx = pushed_arrays(states, inputs, self.state_limits, prior, env.spec.CTRL_FREQ)
            buf.push({'state': state, 'act': act, 'barrier_dot': barrier_dot, 'barrier_dot_approx': approx})
            if self.fused_update:                            # the same draws in the same order, then ONE call for the episode's steps
                rows = [buf.sample_indices(self.train_batch_size) for _ in range(self.train_iterations)]
                self.sampled_indices += rows
                if rows:
                    self.last_losses = self.update_rows(np.stack(rows))
                continue
            for _ in range(self.train_iterations):
                idx = buf.sample_indices(self.train_batch_size)
                self.sampled_indices.append(idx)
                self.update(buf.gather(idx))
        del keep

    # ---- checkpoints (cbf_nn.py:272-308)
    def reset(self):
        super().reset()
        if getattr(self, 'buffer', None) is not None:
            self.buffer.reset()

    def save(self, path):
        import torch
        path_dir = os.path.dirname(path)
        if path_dir:
            os.makedirs(path_dir, exist_ok=True)
        state_dict = {'agent': {k: v.detach().cpu() for k, v in self.mlp.state_dict().items()}}
        if self.training:
            buf = self.buffer if self.buffer is not None else DeviceCBFBuffer(self.model.nx, self.model.nu, 1, 'cpu', self.train_batch_size)
            state_dict['buffer'] = buf.state_dict()
        torch.save(state_dict, path)

    def load(self, path):
        import torch
        state = torch.load(path, map_location='cpu', weights_only=False)
        self.mlp.load_state_dict(state['agent'])
        if self.training and 'buffer' in state:
            rows = int(np.asarray(state['buffer']['state']).shape[0])
            if self.buffer is None or self.buffer.max_size != rows:
                dev = self.buffer.device if self.buffer is not None else (self._flat.device if self._flat is not None else 'cpu')
                self.buffer = DeviceCBFBuffer(self.model.nx, self.model.nu, rows, dev, self.train_batch_size, self.seed)
            self.buffer.load_state_dict(state['buffer'])

    def close(self):
        if self._learn_env is not None:
            self._learn_env.close()
            self._learn_env = None
        super().close()

"""RARL and RAP (robust adversarial RL, single adversary / adversary population) on the HIP rollout engine.

Mirrors /root/reference/safe_control_gym/controllers/rarl/rarl.py and rap.py:
  rarl.py:267-281   train_step = update_agent (agent_iterations x [collect, PPO update]) then update_adversary
  rarl.py:349-428   collect_rollouts: BOTH policies act on every control step; the adversary's action goes through
                    `set_adversary_control` (benchmark_env.py:216-228: clip to [-1, 1], scale, offset) into the env's action
                    or dynamics disturbance channel; the protagonist learns from +reward, the adversary from -reward
  rarl.py:430-467   update_agent / update_adversary
  rap.py:257-281    train_step = ONE collection, then the protagonist's update and one update per sampled adversary
  rap.py:349-470    collect_rollouts: env reset, a SORTED adversary index per env (contiguous groups), every adversary acts on
                    its group, advantages normalised over the whole batch, the adversary rollout split by group
The env needs `adversary_disturbance: 'action' | 'dynamics'` in its task config (the kernel's adversary channel).

Both collectors are HIP-graph captured (static shapes): T x (protagonist step, adversary step(s), env kernel with the
adversary channel, statistics) + both agents' bootstrap / GAE — one replay per collection.  RAP evaluates every member of
the population on the whole batch and selects per env by index (population sizes are 2-4: rap.yaml:7), which keeps the
shapes static while the groups are re-drawn every iteration.

Fused collector (`_collect_fused_both`): on an env built with HipVecEnv(..., policy=(hidden, activation),
adversaries=n) the T control steps of both sides are ONE scg_rollout_adversarial launch (both actors on the matrix cores inside
the env kernel; RAP: each env's own adversary), followed by batched critic passes of both sides and both GAE passes — the same
quantities as the PyTorch collector, captured in the same graph.
"""
import warnings

import time

import numpy as np
import torch

from safe_control_gym_amd import parallel
from safe_control_gym_amd.ppo import PPO, PPOAgent, PPOConfig, advantage_moments, normalise_advantages


def _normalised(adv, moments):
    parallel.all_reduce_sum_(moments)
    return normalise_advantages(adv, moments)


class _TwoSided(PPO):
    """Shared by RARL and RAP: a second set of (action, value, log-prob) buffers for the adversary side and the captured
    collection of both sides."""

    def __init__(self, env, cfg: PPOConfig, seed=0):
        if env.spec.adversary_disturbance is None:
            raise ValueError(f'{type(self).__name__} needs an env with adversary_disturbance set (benchmark_env.py:216-228)')
        cfg.extra = dict(cfg.extra, fused_rollout=False)      # two policies act per step: the torch-policy collector
        super().__init__(env, cfg, seed)
        self.adv_dim = env.spec.adversary_dim
        f = dict(device=self.device, dtype=torch.float32)
        self.act_adv = torch.zeros(self.T, self.N, self.adv_dim, **f)
        self.v_adv = torch.zeros(self.T, self.N, **f)
        self.logp_adv = torch.zeros(self.T, self.N, **f)
        self._two_graph = None
        self._fused_two_sided = False           # decided by the subclass once its adversaries exist (_setup_fused)

    def _setup_fused(self, n_adversaries):
        """The fused collector when the env carries the matching adversary shape, the library serves it, the protagonist has its flat
        parameter vector and no running normaliser is on; an env that asked for adversaries it cannot get warns and keeps the PyTorch
        collector."""
        from safe_control_gym_amd import _adversarial
        cfg, env = self.cfg, self.env
        want = getattr(env, 'adversaries_requested', None)
        if want is None:
            return
        shape = (cfg.hidden_dim, cfg.activation, int(n_adversaries))
        ok = (getattr(env, 'adversary_shape', None) == shape and self.agent._flat is not None and not self._normalise
              and _adversarial.supported(self.obs_dim, cfg.hidden_dim, self.act_dim, self.adv_dim, cfg.activation, int(n_adversaries)))
        if not ok:
            warnings.warn(f'{type(self).__name__}: no fused adversarial collector for env adversary shape '
                          f'{getattr(env, "adversary_shape", None)} / wanted {shape} (normalisers: {self._normalise}); '
                          'using the PyTorch collector', RuntimeWarning, stacklevel=3)
            return
        f = dict(device=self.device, dtype=torch.float32)
        T, N = self.T, self.N
        self._fused_two_sided = True
        self._fv = (torch.zeros(T + 1, N, **f), torch.zeros(T + 1, N, **f))            # critic values of obs[0..T]: protagonist, adversary
        self._ftv = (torch.zeros(T, N, **f), torch.zeros(T, N, **f))                    # ... of the terminal observations
        self._f_episode_acc = torch.zeros(N, 8, **f)
        self._f_adv_index = torch.zeros(N, dtype=torch.int32, device=self.device)

    def _adversary_step(self, obs):
        raise NotImplementedError

    def _adversary_critic(self, x):
        raise NotImplementedError

    def _collect_body(self):
        ac, env = self.agent.ac, self.env
        for t in range(self.T):
            act, v, logp = ac.step(self.obs[t])
            a_adv, v_adv, logp_adv = self._adversary_step(self.obs[t])
            self.act[t], self.v[t], self.logp[t] = act, v, logp
            self.act_adv[t], self.v_adv[t], self.logp_adv[t] = a_adv, v_adv, logp_adv
            env.set_adversary_control(self.act_adv[t])        # clip, scale, offset -> env._adv
            out, c_out = self._slots[t]
            env.step_tensors(self.act[t], env._adv, out=out, c_out=c_out)
            env._adv = None
            if self._normalise:
                self.obs[t + 1].copy_(self.obs_normalizer(self.obs[t + 1]))
                self.rew[t].copy_(self.reward_normalizer(self.rew[t], self.done[t]))
            d = self.done[t].to(torch.float32)
            self.ep_count += d.sum()
            self.ep_return_sum += (out.fin_return * d).sum()
            self.ep_length_sum += (out.fin_length * d).sum()
            self.ep_violation_sum += (out.fin_violation * d).sum()

    # ---- fused collector ----------------------------------------------------------------------------------------
    def _adversary_agents(self):
        raise NotImplementedError

    def _critic_rows(self, agent, x, out):
        """out[m] = agent's critic(x[m]): the MFMA forward kernel (scg_mlp_forward, the protagonist's learner library — a critic's
        shape does not depend on the action width) where the agent has a flat parameter vector, else the PyTorch critic."""
        from safe_control_gym_amd import _learn
        cfg = self.cfg
        if agent._flat is not None and _learn.supported(self.obs_dim, cfg.hidden_dim, self.act_dim, cfg.activation):
            import ctypes as C
            D = _learn.lib(self.obs_dim, cfg.hidden_dim, self.act_dim, cfg.activation)
            _, c_lay, _, _ = agent._layouts()
            st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
            with torch.cuda.device(self.device):
                _learn.check(D, D.scg_mlp_forward(agent._flat['p'].data_ptr(), C.byref(c_lay), 1, x.data_ptr(), int(x.shape[0]),
                                                  out.data_ptr(), None, st))
        else:
            out.copy_(agent.ac.critic(x).squeeze(-1))

    def _fused_values(self, side, agents):
        """Critic values of obs[0..T] and of the terminal observations for one side; a population evaluates every member on all rows
        and selects each env's own (static shapes)."""
        T, N = self.T, self.N
        v_all, tv = self._fv[side], self._ftv[side]
        x, xt = self.obs.view((T + 1) * N, self.obs_dim), self.term_obs.view(T * N, self.obs_dim)
        if len(agents) == 1:
            self._critic_rows(agents[0], x, v_all.view(-1))
            self._critic_rows(agents[0], xt, tv.view(-1))
        else:
            vs, ts = [], []
            for a in agents:
                vs.append(torch.empty((T + 1) * N, device=self.device))
                ts.append(torch.empty(T * N, device=self.device))
                self._critic_rows(a, x, vs[-1])
                self._critic_rows(a, xt, ts[-1])
            v_all.view(-1).copy_(self._select(vs))
            tv.view(-1).copy_(self._select(ts))
        return v_all, tv

    def _fused_returns(self, v_all, tv, rew_buf):
        """ppo_utils.py:374-402 on [T, N] buffers: time truncation bootstraps with the terminal observation's value (= _returns_body)."""
        cfg, T = self.cfg, self.T
        mask = 1.0 - self.done.to(torch.float32)
        trunc = (self.flags & 1).bool() & self.done.bool()
        terminal_v = torch.where(trunc, tv, torch.zeros_like(tv))
        ret, adv = self._gae(rew_buf.clone(), v_all[:T].contiguous(), mask, terminal_v, v_all[T].contiguous(), cfg.gamma, cfg.gae_lambda,
                             cfg.use_gae)
        return ret, adv, advantage_moments(adv)

    @torch.no_grad()
    def _collect_fused_both(self):
        """One scg_rollout_adversarial launch for the T control steps of both sides, the batched critic passes of both sides, both
        sides' bootstrap and GAE (the adversary's on -reward).  Device work only: _collect_both captures it in _two_graph."""
        from safe_control_gym_amd import _adversarial
        T = self.T
        advs = self._adversary_agents()
        n = len(advs)
        if n > 1:
            self._f_adv_index.copy_(self.adv_index)
        self.env.rollout_adversarial(self._policy_struct(), [_adversarial.actor_ptrs(a.ac.actor) for a in advs], T, self.obs, self.act,
                                     self.logp, self.rew, self.done, self.flags, self.act_adv, self.logp_adv,
                                     adv_index=self._f_adv_index if n > 1 else None, terminal_obs=self.term_obs,
                                     episode_acc=self._f_episode_acc)
        # finished episodes (count, return, length, violation steps) of this collection, once
        self._ep_tot += self._f_episode_acc[:, :4].sum(0)
        self._f_episode_acc.zero_()
        v_all, tv = self._fused_values(0, [self.agent])
        self.v.copy_(v_all[:T])
        va_all, tva = self._fused_values(1, advs)
        self.v_adv.copy_(va_all[:T])
        return self._fused_returns(v_all, tv, self.rew), self._fused_returns(va_all, tva, -self.rew)

    def _both_returns(self, dense):
        ag = self._returns_body(dense)
        ad = self._returns_body(dense, self._adversary_critic, -self.rew, self.v_adv)
        return ag, ad

    def _collect_both(self):
        """One collection + the (returns, advantages, moments) of both sides; a graph replay when graphs are on."""
        if self._fused_two_sided:
            res = self._collect_fused_two_graph()
        elif self._graph_rollout:
            epoch = getattr(self.env, 'seed_epoch', 0)
            if self._two_graph is None or self._two_graph[2] != epoch:
                dev = self.device
                s = torch.cuda.Stream(dev)
                s.wait_stream(torch.cuda.current_stream(dev))
                with torch.cuda.stream(s):
                    for _ in range(3):          # warm up the torch ops only (no env step: the simulation must not advance)
                        self.agent.ac.step(self.obs[0])
                        self._adversary_step(self.obs[0])
                        self._both_returns(True)
                torch.cuda.current_stream(dev).wait_stream(s)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    self._collect_body()
                    out = self._both_returns(True)
                self._two_graph = (g, out, epoch)
            self._two_graph[0].replay()
            (r0, a0, m0), (r1, a1, m1) = self._two_graph[1]
            res = (r0, a0, m0.clone()), (r1, a1, m1.clone())
        else:
            self._collect_body()
            res = self._both_returns(False)
        self.total_steps += self.T * self.N * parallel.world_size()
        return res

    def _collect_fused_two_graph(self):
        """The fused collection: eagerly the first time after a (re)seed (libraries load, kernel attributes are set), captured the
        second time, replayed from then on; eagerly every time without graphs."""
        if not self._graph_rollout:
            return self._collect_fused_both()
        epoch = getattr(self.env, 'seed_epoch', 0)
        st = self._two_graph
        if st is None or st[2] != epoch:
            self._two_graph = (None, None, epoch)
            return self._collect_fused_both()
        if st[0] is None:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, capture_error_mode='thread_local'):
                out = self._collect_fused_both()
            self._two_graph = st = (g, out, epoch)
        st[0].replay()
        (r0, a0, m0), (r1, a1, m1) = st[1]
        return (r0, a0, m0.clone()), (r1, a1, m1.clone())

    def _data(self, adversary, ret, adv, lo=0, hi=None):
        hi = self.N if hi is None else hi
        n = hi - lo
        M = self.T * n
        sl = lambda t: t[:, lo:hi]                          # noqa: E731
        return {'obs': sl(self.obs[:self.T]).reshape(M, self.obs_dim),
                'act': sl(self.act_adv if adversary else self.act).reshape(M, -1),
                'logp': sl(self.logp_adv if adversary else self.logp).reshape(M), 'adv': sl(adv).reshape(M),
                'ret': sl(ret).reshape(M), 'v': sl(self.v_adv if adversary else self.v).reshape(M)}


class RARL(_TwoSided):
    def __init__(self, env, cfg: PPOConfig, seed=0, agent_iterations=1, adversary_iterations=1):
        super().__init__(env, cfg, seed)
        self.agent_iterations, self.adversary_iterations = int(agent_iterations), int(adversary_iterations)
        self.adversary = PPOAgent(self.obs_dim, self.adv_dim, cfg, self.device)
        self._setup_fused(1)

    def _adversary_agents(self):
        return [self.adversary]

    def _adversary_step(self, obs):
        return self.adversary.ac.step(obs)

    def _adversary_critic(self, x):
        return self.adversary.ac.critic(x)

    def collect(self):
        return self._collect_both()

    def _one_update(self, adversary):
        (ret, adv, moments) = self._collect_both()[1 if adversary else 0]
        with torch.no_grad():
            adv = _normalised(adv, moments)
        res = (self.adversary if adversary else self.agent).update(self._data(adversary, ret, adv))
        self.obs[0].copy_(self.obs[self.T])
        return res

    def train_step(self):
        t0 = time.perf_counter()
        out = {}
        for name, n, adversary in (('', self.agent_iterations, False), ('_adv', self.adversary_iterations, True)):
            acc = {}
            for _ in range(n):
                for k, v in self._one_update(adversary).items():
                    acc[k] = acc.get(k, 0.0) + v / n
            out.update({k + name: v for k, v in acc.items()})
        out.update({'step': self.total_steps, 'elapsed_time': time.perf_counter() - t0})
        return out


class RAP(_TwoSided):
    """rap.py: a population of adversaries; every collection re-draws which adversary faces which env."""

    def __init__(self, env, cfg: PPOConfig, seed=0, num_adversaries=2):
        super().__init__(env, cfg, seed)
        self.num_adversaries = int(num_adversaries)
        # the groups change size every iteration: the adversaries' minibatch updates run on the PyTorch path (no captured
        # shapes); the protagonist, whose batch is the whole rollout, keeps the fused / graphed update
        adv_cfg = PPOConfig(**{**cfg.__dict__, 'extra': dict(cfg.extra, cuda_graphs=False)})
        self.adversaries = [PPOAgent(self.obs_dim, self.adv_dim, adv_cfg, self.device) for _ in range(self.num_adversaries)]
        self._rng = np.random.RandomState(seed)               # rap.py:356 draws from NumPy's global stream
        self.adv_index = torch.zeros(self.N, dtype=torch.long, device=self.device)
        self.groups = []
        self._setup_fused(self.num_adversaries)

    def _adversary_agents(self):
        return self.adversaries

    def _select(self, per_adv):
        """per_adv: list (one per adversary) of [N, ...] tensors (or [T*N, ...], time-major) -> rows of each env's adversary."""
        st = torch.stack(per_adv, 0)
        idx = self.adv_index.repeat(st.shape[1] // self.N)
        idx = idx.view(1, -1, *([1] * (st.dim() - 2))).expand(1, *st.shape[1:])
        return st.gather(0, idx)[0]

    def _adversary_step(self, obs):
        outs = [a.ac.step(obs) for a in self.adversaries]
        return tuple(self._select([o[k] for o in outs]) for k in range(3))

    def _adversary_critic(self, x):
        return self._select([a.ac.critic(x) for a in self.adversaries])

    def _both_returns(self, dense):
        return super()._both_returns(True)                  # (the per-env selection needs whole [T x N] batches)

    def collect(self):
        # rap.py:356-357: sorted adversary indices, one per env -> contiguous groups
        idx = np.sort(self._rng.randint(self.num_adversaries, size=self.N))
        groups, starts = np.unique(idx, return_index=True)
        ends = np.concatenate([starts[1:], [self.N]])
        self.groups = [(int(g), int(s), int(e)) for g, s, e in zip(groups, starts, ends)]
        self.adv_index.copy_(torch.as_tensor(idx, device=self.device))
        self.obs[0].copy_(self.obs_normalizer(self.env.reset_tensors()))      # rap.py:361: every collection starts from a reset
        return self._collect_both()

    def train_step(self):
        t0 = time.perf_counter()
        (ret, adv, mom), (ret_a, adv_a, mom_a) = self.collect()
        with torch.no_grad():
            adv, adv_a = _normalised(adv, mom), _normalised(adv_a, mom_a)       # both over the whole batch (rap.py:425,448)
        out = dict(self.agent.update(self._data(False, ret, adv)))
        for k, s, e in self.groups:
            res = self.adversaries[k].update(self._data(True, ret_a, adv_a, s, e))
            out.update({f'{name}_adv{k}': v for name, v in res.items()})
        out.update({'step': self.total_steps, 'elapsed_time': time.perf_counter() - t0, 'adv_indices': [g[0] for g in self.groups]})
        return out

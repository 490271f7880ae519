"""Controller-level drop-in: the reference's controller ids and constructor / method surface on the HIP engine.

    ctrl = make('ppo', env_func, training=True, checkpoint_path=..., output_dir=..., seed=..., **algo_config)
    ctrl.reset(); ctrl.learn(); ctrl.save(path); results = ctrl.run(n_episodes=10); ctrl.close()

is how examples/rl/train_rl_controller.py:32-60 and experiments drive every RL controller
(/root/reference/safe_control_gym/controllers/__init__.py:29-47 registers 'ppo', 'sac', 'rarl', 'rap', 'safe_explorer_ppo';
base_controller.py:12-140 is the surface).  `env_func` is the reference's `partial(make, task, **task_config)`; algo_config
keys and defaults are those of controllers/<algo>/<algo>.yaml (get_config(idx) returns them).

These classes are thin: they resolve env_func to (task id, YAML keys), build the batched HipVecEnv (training env of
`rollout_batch_size` envs, evaluation env of `eval_batch_size`), and delegate to ppo.PPO / sac.SAC / rarl.RARL / rarl.RAP /
safe_explorer.SafeExplorerPPO.  Differences from upstream that a caller can see: logging is a dict per `log_interval`
(no tensorboard / text logger), `run()` evaluates `n_episodes` episodes in parallel (one per eval env) instead of one after
another, and there is no CPU path (`use_gpu=False` raises).
"""
import os

import numpy as np
import torch

from safe_control_gym_amd import _lib as L
from safe_control_gym_amd.record_episode_statistics import resolve_env_func
from safe_control_gym_amd.vec_env import HipVecEnv

_RUNNER = {'max_env_steps': 1000000, 'num_workers': 1, 'rollout_batch_size': 4, 'deque_size': 10, 'eval_batch_size': 10,
           'log_interval': 0, 'save_interval': 0, 'num_checkpoints': 0, 'eval_interval': 0, 'eval_save_best': False,
           'tensorboard': False}
PPO_DEFAULTS = dict(hidden_dim=64, activation='tanh', norm_obs=False, norm_reward=False, clip_obs=10, clip_reward=10, gamma=0.99,
                    use_gae=False, gae_lambda=0.95, use_clipped_value=False, clip_param=0.2, target_kl=0.01, entropy_coef=0.01,
                    opt_epochs=10, mini_batch_size=64, actor_lr=0.0003, critic_lr=0.001, max_grad_norm=0.5, rollout_steps=100,
                    **_RUNNER)                                                  # controllers/ppo/ppo.yaml
SAC_DEFAULTS = dict(hidden_dim=256, activation='relu', norm_obs=False, norm_reward=False, clip_obs=10., clip_reward=10., gamma=0.99,
                    tau=0.005, init_temperature=0.2, use_entropy_tuning=False, target_entropy=None, train_interval=100,
                    train_batch_size=64, actor_lr=0.001, critic_lr=0.001, entropy_lr=0.001, warm_up_steps=1000,
                    max_buffer_size=1000000, **_RUNNER)                         # controllers/sac/sac.yaml
# controllers/ddpg/ddpg.yaml
DDPG_DEFAULTS = dict(hidden_dim=256, norm_obs=False, norm_reward=False, clip_obs=10., clip_reward=10., gamma=0.99, tau=0.005,
                     random_process={'func': 'OrnsteinUhlenbeckProcess', 'std': {'func': 'LinearSchedule', 'args': 0.2}},
                     train_interval=100, train_batch_size=64, actor_lr=0.001, critic_lr=0.001, warm_up_steps=10000,
                     max_buffer_size=1000000, **_RUNNER)
# controllers/rarl/rarl.yaml (its `pretrained`, `train_protagonist`, `train_adversary` keys are read by nothing upstream either)
RARL_DEFAULTS = dict(PPO_DEFAULTS, agent_iterations=10, adversary_iterations=10, pretrained=None, train_protagonist=True,
                     train_adversary=True)
RARL_DEFAULTS.pop('activation')                                                         # (rarl.yaml / rap.yaml have no such key)
RAP_DEFAULTS = dict({k: v for k, v in RARL_DEFAULTS.items() if k not in ('pretrained', 'train_protagonist', 'train_adversary')},
                    num_adversaries=2)                                                  # controllers/rarl/rap.yaml


# controllers/safe_explorer/safe_ppo.yaml
SAFE_EXPLORER_PPO_DEFAULTS = dict({k: v for k, v in PPO_DEFAULTS.items() if k != 'activation'}, pretraining=True, pretrained=None,
                                  constraint_hidden_dim=10, constraint_lr=0.0001, constraint_batch_size=256,
                                  constraint_steps_per_epoch=6000, constraint_epochs=25, constraint_eval_steps=1500,
                                  constraint_eval_interval=5, constraint_buffer_size=1000000, constraint_slack=None)


class _Deterministic:
    def __init__(self, ac):
        self.ac = ac

    def act(self, obs):
        return self.ac.act(obs, deterministic=True)


class HipController:
    """base_controller.py:12-140 for the RL family."""
    DEFAULTS = {}

    def __init__(self, env_func, training=True, checkpoint_path='model_latest.pt', output_dir='temp', use_gpu=True, seed=0, **kwargs):
        if not use_gpu or not torch.cuda.is_available():
            raise L.ScgError('the HIP engine has no CPU path (use_gpu=False / no HIP device)')
        self.env_func, self.training, self.checkpoint_path, self.output_dir, self.seed = env_func, training, checkpoint_path, output_dir, seed
        self.use_gpu, self.device = True, torch.device('cuda', torch.cuda.current_device())
        cfg = dict(self.DEFAULTS)
        cfg.update(kwargs)
        self.algo_config = cfg
        for k, v in cfg.items():                    # base_controller.py:40-41: algo args become attributes
            setattr(self, k, v)
        self.env_id, self.task_config = resolve_env_func(env_func)
        # keys of the reference's task YAMLs that are HipVecEnv's own named parameters or moot here: every
        # examples/rl/config_overrides/*/*.yaml carries `seed:` inside task_config, and env_func is
        # partial(make, task, output_dir=..., **task_config) — the controller's `seed` argument wins, as upstream
        # (make_vec_envs(env_func, None, n, workers, seed), ppo.py:48)
        for k in ('output_dir', 'seed', 'num_envs', 'return_numpy', 'policy', 'device'):
            self.task_config.pop(k, None)
        self.results_dict = {}
        self._build()

    # -- construction helpers
    def _vec(self, n, seed, policy=None, **over):
        return HipVecEnv(self.env_id, n, seed=seed, return_numpy=False, policy=policy, **dict(self.task_config, **over))

    def _policy_shape(self):
        return None

    def _build(self):
        raise NotImplementedError

    # -- the reference surface
    @property
    def total_steps(self):
        return self.impl.total_steps

    @property
    def agent(self):
        return self.impl.agent

    def reset(self):
        """ppo.py:96-110: (re)initialise for training or evaluation.  The batched env was reset at construction and keeps its
        episode statistics on the device; nothing else to do."""
        self.results_dict = {}

    def reset_before_run(self, obs=None, info=None, env=None):
        self.results_dict = {}

    def close(self):
        self.env.close()
        if getattr(self, 'eval_env', None) is not None:
            self.eval_env.close()
        if getattr(self, '_run_env_cbf', None) is not None:
            self._run_env_cbf.close()

    def save(self, path):
        self.impl.save(path)

    def load(self, path):
        self.impl.load(path, training=self.training)

    def train_step(self):
        return self.impl.train_step()

    def _act_module(self):
        return self.impl.agent.ac

    def select_action(self, obs, info=None):
        with torch.inference_mode():
            o = torch.as_tensor(np.asarray(obs), dtype=torch.float32, device=self.device)
            nz = getattr(self.impl, 'obs_normalizer', None)
            if nz is not None and getattr(self, 'norm_obs', False):
                frozen = nz.read_only
                nz.set_read_only()
                o = nz(o)
                nz.read_only = frozen
            return self._act_module().act(o).cpu().numpy()

    def run(self, env=None, render=False, n_episodes=10, verbose=False, safety_filter=None, **kwargs):
        """ppo.py:210-257: evaluation with the current (deterministic) policy — here `n_episodes` episodes side by side, one
        per env of the evaluation env.  Returns the reference's dict: ep_returns, ep_lengths (+ constraint_violation, mse).
        safety_filter: a cbf.CBF — every action passes through the filter (base_experiment.py:177-184) in ONE fused launch; the result
        gains `safety_filter_data` (per-env steps / corrected_steps / infeasible_steps / mean_correction)."""
        from safe_control_gym_amd.ppo import evaluate
        if render:
            raise NotImplementedError('no renderer: the simulator has no GUI')
        ev = env if isinstance(env, HipVecEnv) else None
        if safety_filter is not None:
            if ev is None:
                nn = hasattr(safety_filter, 'residual')                              # a cbf_nn.CBF_NN: its own library
                cached = getattr(self, '_run_env_cbf', None)
                if cached is None or cached.num_envs != n_episodes or (cached.cbf_nn_shape is not None) != nn:
                    if cached is not None:
                        cached.close()
                    self._run_env_cbf = HipVecEnv(self.env_id, n_episodes, seed=self.seed * 111, return_numpy=False, policy=self._policy_shape(),
                                                  cbf=not nn, cbf_nn=nn, **self.task_config)
                ev = self._run_env_cbf
            if getattr(self, 'norm_obs', False) or not getattr(self.impl, '_fused_rollout', False):
                raise L.ScgError('run(safety_filter=) needs the fused rollout path without observation normalisation')
            res = evaluate(self._act_module(), ev, policy=self.impl._policy_struct(True), safety_filter=safety_filter)
            a = ev._eval_cbf['acc']
            out = {'ep_returns': a[:, 1].double().cpu().numpy(), 'ep_lengths': a[:, 2].double().cpu().numpy(),
                   'constraint_violation': a[:, 3].double().cpu().numpy(), 'mse': a[:, 4].double().cpu().numpy(),
                   'safety_filter_data': {k: v.double().cpu().numpy() for k, v in res['safety_filter_data'].items()}}
            self.results_dict = out
            return out
        if ev is None:
            if getattr(self, '_run_env', None) is None or self._run_env.num_envs != n_episodes:
                self._run_env = self._vec(n_episodes, self.seed * 111, self._policy_shape())
            ev = self._run_env
        nz = self.impl.obs_normalizer if getattr(self, 'norm_obs', False) and hasattr(self.impl, 'obs_normalizer') else None
        pol = None
        if nz is None and getattr(self.impl, '_fused_rollout', False) and ev.policy_shape is not None:
            pol = self.impl._policy_struct(True)
        evaluate(self._act_module(), ev, obs_normalizer=nz, policy=pol)
        if pol is not None:
            a = ev._eval_fused['acc']
            tot = {'ret': a[:, 1], 'length': a[:, 2], 'viol': a[:, 3], 'mse': a[:, 4]}
        else:
            tot = ev._eval_cache['acc']
        out = {'ep_returns': tot['ret'].double().cpu().numpy(), 'ep_lengths': tot['length'].double().cpu().numpy(),
               'constraint_violation': tot['viol'].double().cpu().numpy(), 'mse': tot['mse'].double().cpu().numpy()}
        self.results_dict = out
        return out

    def learn(self, env=None, **kwargs):
        """ppo.py:150-193: train_step until max_env_steps with the reference's checkpoint / evaluation / logging cadence."""
        hist = []
        while self.total_steps < self.max_env_steps:
            before = self.total_steps
            results = self.train_step()
            crossed = lambda k: bool(k) and (self.total_steps // k) > (before // k)          # noqa: E731
            # (upstream tests `total_steps % interval == 0`, which only fires when the interval is a multiple of the per-iteration
            #  step count; crossing the multiple is the same cadence without that restriction)
            if self.total_steps >= self.max_env_steps or crossed(self.save_interval):
                self.save(self.checkpoint_path)
                self.save(os.path.join(self.output_dir, 'checkpoints', f'model_{self.total_steps}.pt'))
            if crossed(self.eval_interval):
                ev = self.run(n_episodes=self.eval_batch_size)
                results['eval'] = ev
                score = float(ev['ep_returns'].mean())
                if self.eval_save_best and getattr(self, 'eval_best_score', -np.inf) < score:
                    self.eval_best_score = score
                    self.save(os.path.join(self.output_dir, 'model_best.pt'))
            if crossed(self.log_interval):
                hist.append({k: v for k, v in results.items() if not isinstance(v, dict)})
        return hist


class PPO(HipController):
    """controllers/ppo/ppo.py:34-303."""
    DEFAULTS = PPO_DEFAULTS

    def _policy_shape(self):
        return (self.hidden_dim, self.activation) if not (self.norm_obs or self.norm_reward) else None

    def _build(self):
        from safe_control_gym_amd import ppo
        pcfg = ppo.PPOConfig.from_dict(self.algo_config)
        n = self.rollout_batch_size if self.training else self.eval_batch_size
        self.env = self._vec(n, self.seed, self._policy_shape())
        self.eval_env = None
        self.impl = self._make_impl(pcfg)

    def _make_impl(self, pcfg):
        from safe_control_gym_amd import ppo
        return ppo.PPO(self.env, pcfg, seed=self.seed)


class RARL(PPO):
    """controllers/rarl/rarl.py.  Extension key `fused_rollout=True` (not in RARL_DEFAULTS / RAP_DEFAULTS, which equal the YAML files):
    the training env is built with the protagonist's shape and the adversaries (HipVecEnv(..., policy=, adversaries=)), so that the
    collection runs as one scg_rollout_adversarial launch (rarl._TwoSided._collect_fused_both).  Evaluation keeps its own env."""
    DEFAULTS = RARL_DEFAULTS

    def _policy_shape(self):
        return None

    def _n_adversaries(self):
        return 1

    def _build(self):
        if not self.algo_config.get('fused_rollout'):
            return super()._build()
        from safe_control_gym_amd import ppo
        pcfg = ppo.PPOConfig.from_dict(self.algo_config)
        n = self.rollout_batch_size if self.training else self.eval_batch_size
        self.env = self._vec(n, self.seed, (pcfg.hidden_dim, pcfg.activation), adversaries=self._n_adversaries())
        self.eval_env = None
        self.impl = self._make_impl(pcfg)

    def _make_impl(self, pcfg):
        from safe_control_gym_amd import rarl
        return rarl.RARL(self.env, pcfg, seed=self.seed, agent_iterations=self.agent_iterations,
                         adversary_iterations=self.adversary_iterations)


class RAP(RARL):
    """controllers/rarl/rap.py."""
    DEFAULTS = RAP_DEFAULTS

    def _n_adversaries(self):
        return int(self.num_adversaries)

    def _make_impl(self, pcfg):
        from safe_control_gym_amd import rarl
        return rarl.RAP(self.env, pcfg, seed=self.seed, num_adversaries=self.num_adversaries)


def offpolicy_fused_shape(spec, algo_config, kind):
    """Whether a SAC / DDPG controller's evaluation is served by the fused actor rollout: (policy= tuple or None, warning text or None),
    a function of the task's EnvSpec (obs_dim, nx, nu) and the algo config alone, so it can be asked without a GPU.
      no `fused_rollout`                       (None, None); `wide_actor=True` without it raises ValueError
      widths 32 / 64 / 96 / 128                served on the agent's fused path (its flat parameter vector), as ever; `wide_actor` changes nothing
      width 256                                served with `wide_actor=True` (csrc/scg_actor_rollout_wide.h), from FlatAgent.packed_actor():
                                               the agent's fused update is not required; without the key it warns, as ever
      running normalisers, multi-row obs       warn and keep the eager loop, with or without `wide_actor`"""
    from safe_control_gym_amd import _ddpg, _sac
    if algo_config.get('wide_actor') and not algo_config.get('fused_rollout'):
        raise ValueError(f'{kind}: wide_actor=True extends fused_rollout=True (the fused evaluation at hidden_dim 256) and needs that key')
    if not algo_config.get('fused_rollout'):
        return None, None
    hidden, act = algo_config['hidden_dim'], algo_config.get('activation', 'relu')
    normalised = bool(algo_config.get('norm_obs') or algo_config.get('norm_reward'))
    single_row = spec.obs_dim in (spec.nx, 2 * spec.nx)
    if algo_config.get('wide_actor') and hidden == L.WIDE_HIDDEN:
        ok = L.actor_supported(spec.obs_dim, hidden, spec.nu, act) and single_row and not normalised
    else:
        agent_fused = (_sac if kind == 'sac' else _ddpg).supported(spec.obs_dim, hidden, spec.nu, act) \
            and bool(algo_config.get('cuda_graphs', True)) and bool(algo_config.get('fused_update', True))
        ok = L.policy_supported(spec.obs_dim, hidden, spec.nu, act) and single_row and agent_fused and not normalised
    if ok:
        return (int(hidden), act, kind), None
    served = 'widths 32, 64, 96, 128 on the fused agent, 256 from the packed actor' if algo_config.get('wide_actor') \
        else 'widths 32, 64, 96, 128 on the fused agent'                                        # (without the key: the text as ever)
    return None, (f'{kind}: fused_rollout=True is not served for hidden_dim {hidden} / {act} / obs {spec.obs_dim} '
                  f'({served}, no running normaliser): keeping the eager evaluation loop')


class _OffPolicy(HipController):
    """What SAC and DDPG share.  Extension key `fused_rollout=True` (not in SAC_DEFAULTS / DDPG_DEFAULTS, which equal the YAML files):
    the envs are built with the actor's shape and kind (HipVecEnv(..., policy=(hidden_dim, activation, 'sac' | 'ddpg'))), so that run()
    and the evaluations inside learn() are ONE scg_rollout_actor launch, and run(safety_filter=) one scg_rollout_cbf_actor launch.  A
    shape the kernel does not serve (hidden_dim 256, the YAML default), an agent off its fused path or a running normaliser warns once
    and keeps the eager evaluation loop.  Training collection is unchanged either way.
    Extension key `wide_actor=True` (not a default either; needs `fused_rollout=True`, ValueError otherwise): hidden_dim 256 joins the
    served widths.  The agent stays off its fused path at that width (training collection and gradient steps in PyTorch); the rollout
    reads FlatAgent.packed_actor(), refreshed from the module's parameters before every launch.  offpolicy_fused_shape decides.
    Extension key `collect_steps=K` (not a default either; `sac` only, needs `fused_rollout=True`, ValueError otherwise): training
    collection runs up to K vector steps per launch, sampled actor inside the env kernel, transitions written straight into the replay
    ring (scg_rollout_sac_collect, include/scg_actor_collect.h).  Updates happen exactly where the stepwise trainer's do
    (offpolicy.chunk_steps); K x envs must fit max_buffer_size (ValueError).  It needs the agent on its fused path, no running
    normaliser, one rank and hidden_dim <= 128: otherwise it warns once and the stepwise collector stays.  The chunked collector draws
    its action noise from the envs' own Philox streams (addressed by episode / step, so checkpoints carry it through
    env_random_state), the stepwise one from the agent's counter stream: at the same seed the two train on DIFFERENT samples, which is
    why the key is opt-in.  On `ddpg` the key raises ValueError: its exploration noise is one process shared by the envs and continued
    across them in env order."""
    KIND = None

    def _check_collect_steps(self):
        if not self.algo_config.get('collect_steps'):
            return
        if self.KIND != 'sac':
            raise ValueError(f'{self.KIND}: collect_steps is not served: the exploration noise is ONE shared noise process continued across '
                             f'the envs in env order, a dependency across the batch inside every step')
        if not self.algo_config.get('fused_rollout'):
            raise ValueError(f'{self.KIND}: collect_steps extends fused_rollout=True (the env library that carries the actor) and needs that key')

    def _policy_shape(self):
        if not hasattr(self, '_fused_shape'):
            from safe_control_gym_amd.env_config import EnvSpec
            cfg = dict(self.algo_config, hidden_dim=self.hidden_dim, norm_obs=self.norm_obs, norm_reward=self.norm_reward)
            self._fused_shape, warning = offpolicy_fused_shape(EnvSpec(self.env_id, dict(self.task_config)), cfg, self.KIND)
            if warning:
                import warnings
                warnings.warn(warning)
        return self._fused_shape

    def _mark_fused(self):
        wide = self._policy_shape() is not None and self._policy_shape()[0] == L.WIDE_HIDDEN       # (served from the packed copy)
        self.impl._fused_rollout = bool(self._policy_shape() is not None and (self.impl.agent.use_fused or wide))
        if self._policy_shape() is not None and not self.impl._fused_rollout:       # (e.g. several ranks: the agent left its fused path)
            import warnings
            warnings.warn(f'{self.KIND}: fused_rollout=True, but the agent is not on its fused path (no flat parameter vector): keeping the '
                          f'eager evaluation loop')


class SAC(_OffPolicy):
    """controllers/sac/sac.py:35-335."""
    DEFAULTS = SAC_DEFAULTS
    KIND = 'sac'

    def _build(self):
        from safe_control_gym_amd import sac
        self._check_collect_steps()
        scfg = sac.SACConfig.from_dict(self.algo_config)
        n = self.rollout_batch_size if self.training else self.eval_batch_size
        self.env = self._vec(n, self.seed, self._policy_shape())
        self.eval_env = None
        self.impl = sac.SAC(self.env, scfg, seed=self.seed)
        self._mark_fused()
        self._det = self.impl.agent.deterministic_policy()  # one object: evaluate() caches its captured graph per policy object

    def _act_module(self):
        return self._det

    def save(self, path, save_buffer=False):
        """sac.py:119-141: agent + (training) total_steps, obs, RNG state, env random state and, with save_buffer, the replay ring."""
        self.impl.save(path, training=self.training, save_buffer=save_buffer)

    def load(self, path):
        self.impl.load(path, training=self.training)


class DDPG(_OffPolicy):
    """controllers/ddpg/ddpg.py:28-341."""
    DEFAULTS = DDPG_DEFAULTS
    KIND = 'ddpg'

    def _build(self):
        from safe_control_gym_amd import ddpg
        self._check_collect_steps()
        self.activation = self.algo_config.setdefault('activation', 'relu')        # (ddpg.yaml has no such key: DDPGAgent's default)
        dcfg = ddpg.DDPGConfig.from_dict(self.algo_config)
        n = self.rollout_batch_size if self.training else self.eval_batch_size
        self.env = self._vec(n, self.seed, self._policy_shape())
        self.eval_env = None
        self.impl = ddpg.DDPG(self.env, dcfg, seed=self.seed)
        self._mark_fused()
        self._det = self.impl.agent.deterministic_policy()

    def reset(self):
        """ddpg.py:87-107: in training mode the noise process restarts from zero as well."""
        super().reset()
        if self.training:
            self.impl.reset_noise()

    def _act_module(self):
        return self._det

    def save(self, path, save_buffer=True):
        """ddpg.py:116-141: agent, normalisers + (training) total_steps, obs, RNG state, env random state, noise process and, with
        save_buffer (upstream's default: on), the replay ring."""
        self.impl.save(path, training=self.training, save_buffer=save_buffer)

    def load(self, path):
        self.impl.load(path, training=self.training)


class SafeExplorerPPO(PPO):
    """controllers/safe_explorer/safe_ppo.py:32-466 — two phases selected by the config, as upstream:
      pretraining: True    learn() = `constraint_epochs` x pretrain_step (random-action transitions -> constraint models); the
                           checkpoint's 'safety_layer' is what the second phase loads;
      pretraining: False   reset() loads the safety layer from `pretrained` (a checkpoint file, or a directory holding
                           model_latest.pt; safe_ppo.py:96-100) and learn() is PPO with the safety-filtered policy.
    Extension key `fused_rollout=True` (not in SAFE_EXPLORER_PPO_DEFAULTS, which equal the YAML): the training and evaluation envs are
    built with the actor's and the safety layer's shape (HipVecEnv(..., policy=(hidden_dim, activation), safety_layer=
    constraint_hidden_dim)), so that the PPO phase collects with one scg_rollout_safe launch and run() evaluates with one.  An
    unservable shape, a safety layer of more than one hidden layer or a running normaliser warns and keeps the eager path.
    Extension key `fused_pretrain=True` (not a default either, independent of `fused_rollout`): the envs are built on the same library and
    the pre-training phase runs fused — an epoch is one scg_collect_constraints launch (random actions drawn in the kernel, transitions
    written to the constraint buffer's ring) and one scg_safety_update launch for all its minibatches; eval_constraint_models takes the
    same two launches in loss-only mode.  Checkpoints keep upstream's keys: a fused run resumes eagerly and the other way round.  Without
    the key the pre-training phase runs eagerly, step by step."""
    DEFAULTS = SAFE_EXPLORER_PPO_DEFAULTS

    def _safety_shape(self):
        """(policy, safety_layer) arguments of the envs: the fused collector's shape when `fused_rollout` or `fused_pretrain` asks for the
        saferoll library and it serves the shape, else (None, None)."""
        from safe_control_gym_amd import _safe_explorer
        from safe_control_gym_amd.env_config import EnvSpec
        if not (self.algo_config.get('fused_rollout') or self.algo_config.get('fused_pretrain')) or self.norm_obs or self.norm_reward:
            return None, None
        hc = self.constraint_hidden_dim
        if isinstance(hc, (list, tuple)):
            if len(hc) != 1:
                return None, None
            hc = hc[0]
        spec = EnvSpec(self.env_id, dict(self.task_config))
        if spec.obs_dim not in (spec.nx, 2 * spec.nx) or not _safe_explorer.supported(spec.obs_dim, self.hidden_dim, spec.nu, self.activation,
                                                                                      spec.n_state_con_rows, hc):
            return None, None
        return (self.hidden_dim, self.activation), int(hc)

    def _vec(self, n, seed, policy=None, **over):
        pol, hc = self._safety_shape()
        if hc is None:
            return super()._vec(n, seed, policy, **over)
        return super()._vec(n, seed, pol, safety_layer=hc, **over)

    def _policy_shape(self):
        return None                                 # (the fused collector's shape comes with safety_layer=, _vec above)

    def _build(self):
        self.activation = self.algo_config.setdefault('activation', 'tanh')         # (safe_ppo_utils.py: the PPO networks' default)
        super()._build()
        self.safety_layer = self.impl.safety_layer
        self.num_constraints = self.impl.C
        self.impl.pretrain_steps = 0

    # pre-training epochs done: lives on the implementation object so that it is saved / restored with its checkpoint
    # (a resumed pre-training run continues at epoch k instead of repeating all `constraint_epochs`)
    _pretrain_steps = property(lambda self: self.impl.pretrain_steps,
                               lambda self, v: setattr(self.impl, 'pretrain_steps', int(v)))

    def _make_impl(self, pcfg):
        from safe_control_gym_amd import safe_explorer
        slack = self.constraint_slack
        if not isinstance(slack, (int, float, list, tuple)):        # safe_explorer_utils.py:47 asserts the same (the YAML default is null)
            raise AssertionError('constraint_slack must be a number or a list (one value per state constraint)')
        return safe_explorer.SafeExplorerPPO(self.env, pcfg, seed=self.seed, constraint_hidden_dim=self.constraint_hidden_dim,
                                             constraint_lr=self.constraint_lr, constraint_slack=slack,
                                             constraint_batch_size=self.constraint_batch_size,
                                             constraint_buffer_size=self.constraint_buffer_size)

    @property
    def total_steps(self):
        return self._pretrain_steps if (self.training and self.pretraining) else self.impl.total_steps

    def reset(self):
        super().reset()
        if self.training and not self.pretraining:
            if not self.pretrained:
                raise AssertionError('Must provide a pre-trained model for adaptation.')         # safe_ppo.py:97
            self.impl.load_safety_layer(self.pretrained)

    def pretrain_step(self):
        import time
        t0 = time.perf_counter()
        losses = self.impl.pretrain_step(self.constraint_steps_per_epoch, self.constraint_batch_size)
        self._pretrain_steps += 1
        res = {f'constraint_{i}_loss': v for i, v in enumerate(losses)}
        res.update({'step': self._pretrain_steps, 'elapsed_time': time.perf_counter() - t0})
        return res

    def eval_constraint_models(self):
        return {f'constraint_{i}_loss': v for i, v in
                enumerate(self.impl.eval_constraint_models(self.constraint_eval_steps, self.constraint_batch_size))}

    def select_action(self, obs, info=None):
        """safe_ppo.py:215-228: the current constraint values are the policy's second input."""
        with torch.inference_mode():
            o = torch.as_tensor(np.asarray(obs), dtype=torch.float32, device=self.device)
            c = torch.as_tensor(np.asarray(info['constraint_values'])[..., :self.num_constraints], dtype=torch.float32, device=self.device)
            nz = self.impl.obs_normalizer
            frozen = nz.read_only
            nz.set_read_only()
            o = nz(o)
            nz.read_only = frozen
            batched = o.dim() == 2
            a = self.impl.agent.ac.act(o if batched else o[None], c if batched else c[None])
            return (a if batched else a[0]).cpu().numpy()

    def run(self, env=None, render=False, n_episodes=10, verbose=False, **kwargs):
        if render:
            raise NotImplementedError('no renderer: the simulator has no GUI')
        ev = env if isinstance(env, HipVecEnv) else None
        if ev is None:
            if getattr(self, '_run_env', None) is None or self._run_env.num_envs != n_episodes:
                self._run_env = self._vec(n_episodes, self.seed * 111)
            ev = self._run_env
        tot = self.impl.evaluate(ev)
        out = {'ep_returns': tot['ret'].double().cpu().numpy(), 'ep_lengths': tot['length'].double().cpu().numpy(),
               'constraint_violation': tot['viol'].double().cpu().numpy(), 'mse': tot['mse'].double().cpu().numpy()}
        self.results_dict = out
        return out

    def learn(self, env=None, **kwargs):
        if not self.pretraining:
            return super().learn(env, **kwargs)
        hist = []                                   # safe_ppo.py:178-213 with final_step = constraint_epochs, train_func = pretrain_step
        while self._pretrain_steps < self.constraint_epochs:
            results = self.pretrain_step()
            k = self._pretrain_steps
            if k >= self.constraint_epochs or (self.save_interval and k % self.save_interval == 0):
                self.save(self.checkpoint_path)
            if self.eval_interval and k % self.eval_interval == 0:
                results['eval'] = self.eval_constraint_models()
            if self.log_interval and k % self.log_interval == 0:
                hist.append({q: v for q, v in results.items() if not isinstance(v, dict)})
        return hist


# (the ids 'ppo', 'sac', 'ddpg', 'rarl', 'rap', 'safe_explorer_ppo' are registered in registration.py with lazy entry points to these classes)

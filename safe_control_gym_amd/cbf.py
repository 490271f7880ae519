"""The reference's CBF-QP safety filter (safety_filters/cbf/cbf.py) on the HIP engine.

    sf = make('cbf', env_func, **sf_config)                        # registration.py; defaults = safety_filters/cbf/cbf.yaml
    certified, success = sf.certify_action(state, uncertified_action)
    valid, infeasible_states = sf.is_cbf()

The reference solves, per state and uncertified action, a QP with two unknowns (the cartpole's one input and one slack), one barrier
row that is affine in the input, and box bounds, through CasADi and qpOASES.  That QP has a closed-form minimiser (include/scg_cbf.h
states it; DESIGN.md derives it): `scg_cbf_certify` evaluates it for a batch of rows in one launch, and `scg_rollout_cbf` puts the same
device function between the actor and the env step of the fused policy rollout (HipVecEnv.rollout_cbf, ppo.evaluate(safety_filter=)).

Differences from upstream a caller can see: `certify_action` accepts a batch ([N, 4] states, [N] or [N, 1] physical actions, NumPy or
device tensors) and then returns arrays; the constructor does not instantiate an env (the task config is resolved on the host); there
is no CPU path — the certify runs on the device or raises.  CartPole only, as upstream.
"""
import numpy as np

from safe_control_gym_amd import _lib as L
from safe_control_gym_amd.env_config import EnvSpec
from safe_control_gym_amd.record_episode_statistics import resolve_env_func
from safe_control_gym_amd.symbolic import AnalyticModel

# safety_filters/cbf/cbf.yaml
CBF_DEFAULTS = dict(slope=0.1, soft_constrained=True, slack_weight=10000.0, slack_tolerance=1.0e-3,
                    prior_info=dict(prior_prop=None, randomize_prior_prop=False, prior_prop_rand_info=None))


def grid_points_per_dim(num_points, nx):
    """cbf.py:253-255: `num_points` rounded so that every vertex is checked, split over the state dimensions."""
    num_points = max(2 * nx, num_points + num_points % (2 * nx))
    return num_points // nx


def state_grid(state_limits, num_points=100, tolerance=0.01):
    """The states CBF.is_cbf checks (cbf.py:243-259): a regular grid over +-(limits + tolerance), first dimension slowest
    (cbf_utils.cartesian_product), float64 [P^nx, nx]."""
    hi = np.asarray(state_limits, dtype=np.float64) + tolerance
    n = grid_points_per_dim(num_points, len(hi))
    axes = [np.linspace(-hi[i], hi[i], n) for i in range(len(hi))]
    return np.stack(np.meshgrid(*axes, indexing='ij'), axis=-1).reshape(-1, len(hi))


class CBF:
    """Control Barrier Function safety filter (cbf.py:17-311)."""

    def __init__(self, env_func, slope=0.1, soft_constrained=True, slack_weight=10000.0, slack_tolerance=1.0e-3, prior_info=None,
                 training=True, checkpoint_path='temp/model_latest.pt', output_dir='temp', use_gpu=True, seed=0, policy=(64, 'tanh'),
                 **kwargs):
        # base_controller.py:30-41
        self.env_func, self.training, self.checkpoint_path, self.output_dir, self.use_gpu, self.seed = \
            env_func, training, checkpoint_path, output_dir, use_gpu, seed
        self.prior_info = prior_info
        for k, v in kwargs.items():
            setattr(self, k, v)
        self.slope, self.soft_constrained, self.slack_weight, self.slack_tolerance = slope, soft_constrained, slack_weight, slack_tolerance
        self.env_id, self.task_config = resolve_env_func(env_func)
        for k in ('output_dir', 'seed', 'num_envs', 'return_numpy', 'policy', 'device'):
            self.task_config.pop(k, None)
        self.spec = EnvSpec(self.env_id, dict(self.task_config))
        spec = self.spec
        input_constraints = [m for m in spec.con_meta if m['var'] == 'input']
        state_constraints = [m for m in spec.con_meta if m['var'] == 'state']
        if len(input_constraints) > 1:
            raise NotImplementedError('CBF currently can\'t handle more than 1 constraint')
        if len(input_constraints) == 0:
            raise Exception('CBF requires at least 1 input constraint')
        self.input_constraint = input_constraints[0]
        if len(state_constraints) > 1:
            raise NotImplementedError('CBF currently can\'t handle more than 1 constraint')
        if len(state_constraints) == 0:
            raise Exception('CBF requires at least 1 state constraint')
        self.state_constraint = state_constraints[0]
        self.policy_shape = (int(policy[0]), policy[1])
        self._venv = None
        self.reset()
        if self.env_id == 'cartpole':
            self.state_limits = [min(abs(self.state_constraint.upper_bounds[i]), abs(self.state_constraint.lower_bounds[i]))
                                 for i in range(self.model.nx)]
        else:
            raise NotImplementedError('[Error] Currently CBF is only implemented for the cartpole system.')
        self.physical_action_bounds = spec.physical_action_bounds

    # ---- the prior model (base_controller.py:134-193 on the analytic stand-in)
    def get_prior(self, prior_info=None):
        info = prior_info or self.prior_info or {}
        prior_prop = dict(info.get('prior_prop') or {})
        rand_info = info.get('prior_prop_rand_info') or {}
        if info.get('randomize_prior_prop', False) and rand_info:
            import copy
            rng = np.random.default_rng(self.seed)
            for k in rand_info:
                assert k in prior_prop, 'A prior param to randomize does not have a base value in prior_prop.'
            rand = copy.deepcopy(rand_info)
            for k in prior_prop:
                if k in rand:
                    distrib = getattr(rng, rand[k].pop('distrib'))
                    prior_prop[k] += distrib(*rand[k].pop('args', []), **rand[k])
        return AnalyticModel(self.env_id, self.spec, prior_prop)

    def params(self):
        """The scg_cbf_params (include/scg_cbf.h) of this filter."""
        from safe_control_gym_amd import _cbf
        p = self.model.params
        lo, hi = (float(np.asarray(b).reshape(-1)[0]) for b in self.physical_action_bounds)
        return _cbf.CbfParams(L=(_cbf.C.c_float * 4)(*[float(v) for v in self.state_limits]), m=p['m'], M=p['M'], l=p['length'], g=p['g'],
                              slope=float(self.slope), slack_weight=float(self.slack_weight), slack_tolerance=float(self.slack_tolerance),
                              lo=lo, hi=hi, soft=int(bool(self.soft_constrained)))

    # ---- the device side
    def attach(self, venv):
        """Certify through `venv`'s library (a HipVecEnv built with cbf=True) instead of an env of this filter's own."""
        if getattr(venv, 'cbf_shape', None) is None:
            raise L.ScgError('attach() needs a HipVecEnv built with policy=(hidden, activation), cbf=True')
        self._venv = venv
        return self

    def _env(self):
        if self._venv is None:
            from safe_control_gym_amd.vec_env import HipVecEnv
            self._venv, self._own_venv = HipVecEnv(self.env_id, 1, seed=self.seed, return_numpy=False, policy=self.policy_shape, cbf=True,
                                                   **self.task_config), True
        return self._venv

    def certify_tensors(self, states, actions):
        """(certified [n], slack [n], feasible uint8 [n]) device tensors of float32 states [n, 4] and physical actions [n]."""
        return self._env().certify_tensors(self.params(), states, actions)

    def certify_action(self, current_state, uncertified_action, info=None):
        """cbf.py:197-222.  One state (4 values; returns (certified ndarray of shape (), bool) and appends to results_dict) or a batch
        ([N, 4] states with [N] / [N, 1] actions, NumPy or device tensors; returns (certified [N], success bool [N]) of the same kind)."""
        import torch
        venv = self._env()
        is_t = torch.is_tensor(current_state)
        s = (current_state if is_t else torch.as_tensor(np.asarray(current_state, dtype=np.float64))).to(device=venv.device, dtype=torch.float32)
        single = s.dim() == 1
        s = s.reshape(-1, 4).contiguous()
        a_in = uncertified_action if torch.is_tensor(uncertified_action) else torch.as_tensor(np.asarray(uncertified_action, dtype=np.float64))
        a = a_in.to(device=venv.device, dtype=torch.float32).reshape(-1).contiguous()
        if a.numel() != s.shape[0]:
            raise ValueError(f'{s.shape[0]} states but {a.numel()} actions')
        cert, _, feas = self.certify_tensors(s, a)
        if single:
            lo, hi = self.physical_action_bounds
            unc = np.clip(np.asarray(uncertified_action.cpu() if torch.is_tensor(uncertified_action) else uncertified_action, dtype=np.float64),
                          lo, hi)
            certified, success = np.squeeze(np.array(float(cert[0]))), bool(feas[0])
            self.results_dict['uncertified_action'].append(unc)
            self.results_dict['feasible'].append(success)
            self.results_dict['certified_action'].append(certified)
            self.results_dict['correction'].append(np.linalg.norm(certified - unc))
            return certified, success
        if is_t:
            return cert, feas.bool()
        return cert.double().cpu().numpy(), feas.bool().cpu().numpy()

    def is_cbf(self, num_points=100, tolerance=0.01):
        """cbf.py:224-296 with the grid certified in ONE launch: (valid_cbf, list of infeasible states)."""
        import torch
        epsilon = 1e-6
        states = state_grid(self.state_limits, num_points, tolerance)
        venv = self._env()
        s = torch.as_tensor(states).to(device=venv.device, dtype=torch.float32)
        a = torch.ones(s.shape[0], device=venv.device, dtype=torch.float32)              # the reference's dummy control input
        _, _, feas = self.certify_tensors(s, a)
        bad = ~feas.bool().cpu().numpy()
        infeasible = states[bad]
        barrier = 1.0 - ((infeasible / np.asarray(self.state_limits, dtype=np.float64)) ** 2).sum(axis=1)
        num_infeasible, num_inside = int(bad.sum()), int((barrier > 0.0 + epsilon).sum())
        print('Number of infeasible states:', num_infeasible)
        print('Number of infeasible states inside superlevel set:', num_inside)
        if num_inside > 0:
            valid_cbf = False
            print('The provided CBF candidate is not a valid CBF.')
        elif num_infeasible > 0:
            valid_cbf = True
            print('The provided CBF candidate is a valid CBF inside its superlevel set for the checked states. '
                  'Consider increasing the sampling resolution to get a more precise evaluation. '
                  'The CBF is not valid on the entire provided domain. Consider softening the CBF constraint by '
                  'setting \'soft_constraint: True\' inside the config.')
        else:
            valid_cbf = True
            print('The provided CBF candidate is a valid CBF for the checked states. '
                  'Consider increasing the sampling resolution to get a more precise evaluation.')
        return valid_cbf, list(infeasible)

    # ---- the reference's bookkeeping surface
    def select_action(self, obs, info=None):
        raise NotImplementedError('[ERROR] select_action is not and will not be implemented for safety filters.')

    def setup_results_dict(self):
        self.results_dict = {'feasible': [], 'uncertified_action': [], 'certified_action': [], 'correction': []}

    def reset(self):
        self.model = self.get_prior()
        self.setup_results_dict()

    def reset_before_run(self, obs=None, info=None, env=None):
        self.setup_results_dict()

    def learn(self, env=None, **kwargs):
        return

    def save(self, path):
        return

    def load(self, path):
        return

    def close(self):
        if self._venv is not None and getattr(self, '_own_venv', False):
            self._venv.close()
        self._venv = None

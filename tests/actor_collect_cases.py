"""Task configs and actor shapes of the fused SAC training collector's tests (tests/test_gpu_sac_collect.py) and of its cost tool
(tools/actor_collect_cost.py); build() compiles the libraries for exactly these, so that the GPU run finds them in the tree.  Tasks
and their 25-step episodes are tests/actor_rollout_cases.task_config's."""
from tests.actor_rollout_cases import EPISODE_STEPS, task_config  # noqa: F401

# (task, hidden, activation), kind sac: the kernel paths that differ
CASES = (('cartpole_stab', 64, 'leaky_relu'),           # 16-byte rows: the transpose path
         ('quadrotor_2D_track', 128, 'relu'),
         ('quadrotor_3D_track', 128, 'relu'),           # act_dim 4: all four normal4 columns, eight head rows
         ('quadrotor_2D_stab', 96, 'relu'))             # 6-float rows: the row-by-row stores
# a state constraint that ends episodes early (done_on_violation): some ring rows are TERMINATED, not truncated
TERMINATING_TASK = 'cartpole_stab'
TERMINATING_OVERRIDE = dict(constraints=[{'constraint_form': 'default_constraint', 'constrained_variable': 'state',
                                          'upper_bounds': [2, 2, 0.03, 1], 'lower_bounds': [-2, -2, -0.03, -1]}], done_on_violation=True)
# libraries that export the entry point and must refuse: (task, hidden, activation, kind)
REFUSING = (('cartpole_stab', 32, 'tanh', 'ddpg'), ('cartpole_stab', 256, 'relu', 'sac'))
# the trainer test: the `sac` controller on CartPole stabilisation as shipped, (hidden, activation)
TRAINER_TASK, TRAINER_SHAPE = 'cartpole_stab', (64, 'leaky_relu')

# tools/actor_collect_cost.py: one chunk of COST_STEPS policy-mode vector steps of SAC 128 relu on Quadrotor 3D tracking as shipped
COST_TASK, COST_SHAPE, COST_STEPS, COST_ENVS = 'quadrotor_3D_track', (128, 'relu'), 25, (4, 256, 2048)


def terminating_task_config():
    env_id, cfg = task_config(TERMINATING_TASK)
    return env_id, dict(cfg, **TERMINATING_OVERRIDE)

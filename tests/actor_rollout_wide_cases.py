"""Task configs and actor shapes of the width-256 fused SAC / DDPG actor rollout's tests (tests/test_gpu_rollout_actor_wide.py) and of
its cost tool (tools/actor_rollout_wide_cost.py); build() compiles the libraries for exactly these, so that the GPU run finds them in
the tree.  Tasks are those of tests/actor_rollout_cases.py: 25-step episodes, so every env finishes, auto-resets and goes on inside a
40-step launch."""
from tests.actor_rollout_cases import EPISODE_STEPS, cbf_task_config, cost_task_config, task_config  # noqa: F401

HIDDEN = 256

# (task, kind, hidden, activation): the kernel paths that differ
CASES = (('cartpole_stab', 'sac', HIDDEN, 'relu'),              # 16-byte obs rows, the smallest L1Q
         ('quadrotor_3D_track', 'sac', HIDDEN, 'relu'),         # NU = 4, the stacked head, the largest L1Q and the most registers
         ('quadrotor_2D_stab', 'ddpg', HIDDEN, 'tanh'),         # 6-float rows, activation on both layers
         ('quadrotor_2D_track', 'ddpg', HIDDEN, 'leaky_relu'))
# the controllers' cases: (controller id, task, hidden, activation)
CONTROLLER_CASES = (('sac', 'cartpole_stab', HIDDEN, 'relu'), ('ddpg', 'cartpole_stab', HIDDEN, 'tanh'))
# the CBF cases (CartPole, the reference example's task with randomised initial states): (kind, hidden, activation)
CBF_CASES = (('sac', HIDDEN, 'relu'), ('ddpg', HIDDEN, 'tanh'))
# the narrow library whose scg_cbf_certify the wide filter rows are held to (built for tests/actor_rollout_cases.py)
CBF_NARROW = ('sac', 64, 'leaky_relu')

# tools/actor_rollout_wide_cost.py: (task, kind, hidden, activation), evaluations of COST_STEPS control steps
COST_STEPS = 250
COST_CASES = (('quadrotor_3D_track', 'sac', HIDDEN, 'relu'), ('cartpole_stab', 'ddpg', HIDDEN, 'relu'))

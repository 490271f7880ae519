"""Task configs and actor shapes of the cbf_nn safety filter's tests (tests/test_gpu_cbf_nn.py), example (examples/run_cbf_nn.py) and
cost tool (tools/cbf_nn_cost.py); build() compiles the libraries for exactly these, so that the GPU run finds them in the tree.  The
task is the reference example's CartPole (tests/golden/cbf_nn_settings.json) with randomised initial states."""
import copy
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def settings():
    with open(os.path.join(GOLDEN, 'cbf_nn_settings.json')) as f:
        return json.load(f)


def task_config(normalized=False, **over):
    """(env id, task config) of the example's CartPole."""
    s = settings()
    cfg = copy.deepcopy(s['task_config'])
    cfg.pop('seed', None)
    cfg.update(randomized_init=True, normalized_rl_action_space=bool(normalized))
    cfg.update(over)
    return s['task'], cfg


# (normalised action space, hidden, activation, auto_reset): the example's shipped PPO shape in both action-space settings, a second
# actor shape whose image does not fit beside the G = 8 row-split image (G = 1 at every N), and learn()'s env (auto_reset off)
CASES = ((False, 64, 'tanh', True), (True, 64, 'tanh', True), (False, 128, 'relu', True), (False, 64, 'tanh', False))
# a library of another task: it exports the entry points and refuses
REFUSING = ('quadrotor_2D_stab', 64, 'tanh')

"""Controller registry (registration.py / controllers.py): the reference's controller ids resolve, and get_config(idx) returns
the defaults of the reference's own controllers/<algo>/<algo>.yaml — as recorded in tests/golden/controller_defaults.json
(tests/golden/make_controller_defaults.py) — and the pinned literal."""
import json
import os

import pytest

from safe_control_gym_amd.registration import get_config, spec

GOLDEN = json.load(open(os.path.join(os.path.dirname(__file__), 'golden', 'controller_defaults.json')))
FILES = {'ppo': 'ppo/ppo.yaml', 'sac': 'sac/sac.yaml', 'rarl': 'rarl/rarl.yaml', 'rap': 'rarl/rap.yaml',
         'safe_explorer_ppo': 'safe_explorer/safe_ppo.yaml'}


@pytest.mark.parametrize('idx', sorted(FILES))
def test_controller_ids_and_default_configs(idx):
    assert spec(idx).entry_point.startswith('safe_control_gym_amd.controllers:')
    cfg = get_config(idx)
    assert cfg is not get_config(idx)                       # a fresh copy per call, like the YAML loader
    assert GOLDEN[idx]['file'] == FILES[idx]
    ref = GOLDEN[idx]['defaults']
    assert ref
    for k, v in ref.items():
        assert k in cfg, (idx, k)
        if isinstance(v, float) or isinstance(cfg[k], float):
            assert float(cfg[k]) == pytest.approx(float(v)), (idx, k)
        else:
            assert cfg[k] == v, (idx, k, cfg[k], v)


def test_pinned_defaults_without_the_reference():
    p, s = get_config('ppo'), get_config('sac')
    assert (p['hidden_dim'], p['activation'], p['opt_epochs'], p['mini_batch_size'], p['target_kl'], p['rollout_steps']) == (64, 'tanh', 10, 64, 0.01, 100)
    assert (s['hidden_dim'], s['activation'], s['tau'], s['train_interval'], s['warm_up_steps']) == (256, 'relu', 0.005, 100, 1000)
    assert get_config('rap')['num_adversaries'] == 2 and get_config('rarl')['agent_iterations'] == 10
    e = get_config('safe_explorer_ppo')
    assert (e['pretraining'], e['pretrained'], e['constraint_hidden_dim'], e['constraint_epochs'], e['constraint_slack']) == (True, None, 10, 25, None)

#!/usr/bin/env python3
"""Default configs of the REFERENCE's controllers (controllers/<algo>/<algo>.yaml) -> tests/golden/controller_defaults.json.

    python tests/golden/make_controller_defaults.py      (needs a reference checkout: ref_stubs.reference_root(), e.g. $SCG_REFERENCE_ROOT)

tests/test_controller_defaults.py holds get_config(idx) to these values.
"""
import json
import os
import sys

import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests.golden.ref_stubs import reference_root  # noqa: E402

FILES = {'ppo': 'ppo/ppo.yaml', 'sac': 'sac/sac.yaml', 'rarl': 'rarl/rarl.yaml', 'rap': 'rarl/rap.yaml',
         'safe_explorer_ppo': 'safe_explorer/safe_ppo.yaml'}

if __name__ == '__main__':
    root = reference_root()
    assert root, 'needs the reference checkout'
    out = {}
    for idx, rel in sorted(FILES.items()):
        with open(os.path.join(root, 'safe_control_gym', 'controllers', rel)) as f:
            out[idx] = {'file': rel, 'defaults': yaml.safe_load(f)}
    with open(os.path.join(HERE, 'controller_defaults.json'), 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(f'{len(out)} controllers -> tests/golden/controller_defaults.json')

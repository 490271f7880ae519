#!/usr/bin/env python3
"""ms per gradient step at the production shape (obs 24, hidden 128, 4 actions, relu, batch 4096), one process, one GPU:
the fused DDPG step (scg_ddpg_update_n, one HIP graph of n steps), the eager DDPGAgent.update (PyTorch kernels, the path of CPU
tensors and unsupported shapes) and the fused SAC step (scg_sac_update_n) at the same shape.  Each leg: warm-up calls, then `reps`
timed calls of `steps` gradient steps between two synchronisations, enqueued lazily (no statistics read back, so no host round trip
inside the timed interval; the eager leg still reads its losses back after every update, as the reference's update does with
.item()); the median of `trials` such timings is reported (with min / max).
A second record times the collector's action launch at `--envs` envs (scg_ddpg_noisy_act with the reference's OU noise, whose
single-launch scan re-walks up to ~23 000 envs in front of each 256-env workgroup, against the same launch without noise), as
replays of a HIP graph of 200 launches: device time, not the host's launch rate.

    python tools/ddpg_update_cost.py [--batch 4096] [--steps 8] [--reps 50] [--trials 5] [--out profiles/ddpg_update_cost.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=4096)
    ap.add_argument('--steps', type=int, default=8)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--trials', type=int, default=5)
    ap.add_argument('--envs', type=int, default=65536)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    from safe_control_gym_amd import ddpg, sac
    dev = torch.device('cuda', 0)
    low, high = -torch.ones(4, device=dev), torch.ones(4, device=dev)
    n = 500_000
    torch.manual_seed(0)
    ring = [torch.randn(n, 24, device=dev), torch.rand(n, 4, device=dev) * 2 - 1, torch.randn(n, device=dev), torch.randn(n, 24, device=dev),
            torch.ones(n, device=dev)]
    out = {'shape': [24, 128, 4, 'relu'], 'batch': a.batch, 'steps_per_call': a.steps, 'device': torch.cuda.get_device_name(dev)}

    def leg(tag, agent, reps):
        buf = sac.DeviceReplay(1_000_000, 24, 4, dev)
        buf.push(*ring)
        for _ in range(3):
            agent.update_from_buffer(buf, a.batch, a.steps, lazy=True)
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.trials):
            t0 = time.perf_counter()
            for _ in range(reps):
                agent.update_from_buffer(buf, a.batch, a.steps, lazy=True)
            torch.cuda.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0) / (reps * a.steps))
        ts.sort()
        out[tag] = {'ms_per_gradient_step_median': ts[len(ts) // 2], 'min': ts[0], 'max': ts[-1]}

    torch.manual_seed(1)
    leg('ddpg_fused', ddpg.DDPGAgent(24, 4, low, high, ddpg.DDPGConfig(hidden_dim=128, activation='relu'), dev), a.reps)
    torch.manual_seed(1)
    eager = ddpg.DDPGAgent(24, 4, low, high, ddpg.DDPGConfig(hidden_dim=128, activation='relu', extra={'fused_update': False}), dev)
    leg('ddpg_eager', eager, max(2, a.reps // 10))
    torch.manual_seed(1)
    leg('sac_fused', sac.SACAgent(24, 4, low, high, sac.SACConfig(hidden_dim=128, activation='relu'), dev), a.reps)
    out['noisy_act'] = noisy_act_cost(a.envs, a.trials)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(line + '\n')


def noisy_act_cost(n_envs, trials, reps=200):
    """us per scg_ddpg_noisy_act launch (+ its one-thread commit) at n_envs envs, 24-128-4 relu: OU noise vs none."""
    import ctypes as C
    import torch
    from safe_control_gym_amd import _ddpg, ddpg
    dev = torch.device('cuda', 0)
    torch.manual_seed(2)
    ag = ddpg.DDPGAgent(24, 4, -torch.ones(4), torch.ones(4), ddpg.DDPGConfig(hidden_dim=128, activation='relu'), dev)
    D = _ddpg.lib(24, 128, 4, 'relu')
    lo, hi = ag.act_bounds()
    obs = torch.randn(n_envs, 24, device=dev)
    out = torch.empty(n_envs, 4, device=dev)
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)
    noise = ddpg.DeviceNoise({'func': 'OrnsteinUhlenbeckProcess', 'std': {'func': 'LinearSchedule', 'args': 0.2}}, 4, dev)
    res = {'envs': n_envs}
    for tag, nz in (('ou_us', noise), ('no_noise_us', None)):
        def call():
            st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            _ddpg.check(D, D.scg_ddpg_noisy_act(ag._flat['p'].data_ptr(), C.byref(ag._flat['actor']), lo, hi, obs.data_ptr(), n_envs, 7,
                                                cnt.data_ptr(), 0, C.byref(nz.struct) if nz else None, None, out.data_ptr(), st))
            if nz:
                _ddpg.check(D, D.scg_ddpg_noise_commit(C.byref(nz.struct), st))
        for _ in range(10):
            call()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(reps):
                call()
        g.replay()
        torch.cuda.synchronize()
        ts = []
        for _ in range(trials):
            t0 = time.perf_counter()
            g.replay()
            torch.cuda.synchronize()
            ts.append(1e6 * (time.perf_counter() - t0) / reps)
        ts.sort()
        res[tag] = ts[len(ts) // 2]
    return res


if __name__ == '__main__':
    main()

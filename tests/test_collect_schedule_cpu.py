"""offpolicy.chunk_steps against a literal simulation of the stepwise OffPolicyTrainer.train_step loop: with the chunked collector the
updates happen at the same total_steps values, with the same n_updates, and every vector step runs in the same mode (uniform warm-up
or policy), whatever k_max is."""
import itertools

import pytest

pytest.importorskip('torch')

GRID = list(itertools.product((1, 4, 16, 2048), (0, 1, 100, 1000), (1, 64, 100, 5000), (1, 8, 25, 64)))


def stepwise(nw, warm_up, interval, max_steps):
    """train_step's loop, one vector step at a time: (mode of every step, {total_steps at an update: n_updates})."""
    total = since = 0
    modes, updates = [], {}
    while total < max_steps:
        modes.append(total < warm_up)
        total += nw
        since += nw
        if total > warm_up and since >= interval:
            updates[total] = since
            since = 0
    return modes, updates


def chunked(nw, warm_up, interval, k_max, max_steps):
    """The chunked train_step: (mode of every step, updates, chunk lengths)."""
    from safe_control_gym_amd.offpolicy import chunk_steps
    total = since = 0
    modes, updates, chunks = [], {}, []
    while total < max_steps:
        k = chunk_steps(total, since, nw, warm_up, interval, k_max)
        assert isinstance(k, int) and 1 <= k <= k_max
        warm = total < warm_up
        for j in range(k):              # one launch has one mode: every step of the chunk must be the stepwise loop's
            assert (total + j * nw < warm_up) == warm
        modes += [warm] * k
        chunks.append(k)
        total += k * nw
        since += k * nw
        if total > warm_up and since >= interval:
            updates[total] = since
            since = 0
    return modes, updates, chunks


@pytest.mark.parametrize('nw,warm_up,interval,k_max', GRID)
def test_chunked_schedule_is_the_stepwise_one(nw, warm_up, interval, k_max):
    max_steps = max(warm_up, interval) * 3 + 7 * nw
    m0, u0 = stepwise(nw, warm_up, interval, max_steps)
    m1, u1, chunks = chunked(nw, warm_up, interval, k_max, max_steps)
    # the chunked loop may overshoot max_steps by less than one chunk: compare on the stepwise run's range
    assert m1[:len(m0)] == m0 and len(m1) >= len(m0)
    last = len(m0) * nw
    assert {t: n for t, n in u1.items() if t <= last} == u0
    assert u0, 'the case never updates'


def test_chunks_are_as_long_as_the_schedule_allows():
    from safe_control_gym_amd.offpolicy import chunk_steps
    # sac.yaml: 4 envs, warm-up 1000 env steps, an update every 100: 250 uniform vector steps, then 25 per update
    assert chunk_steps(0, 0, 4, 1000, 100, 25) == 25
    assert chunk_steps(0, 0, 4, 1000, 100, 1000) == 250            # the switch to the policy ends the chunk
    assert chunk_steps(996, 996, 4, 1000, 100, 25) == 1
    assert chunk_steps(1000, 1000, 4, 1000, 100, 25) == 1          # the update the warm-up's steps owe comes after the first policy step
    assert chunk_steps(1004, 0, 4, 1000, 100, 64) == 25
    assert chunk_steps(1004, 40, 4, 1000, 100, 64) == 15
    assert chunk_steps(1004, 0, 4, 1000, 100, 8) == 8
    assert chunk_steps(5000, 0, 2048, 1000, 100, 25) == 1          # train_interval <= N: every chunk has length 1

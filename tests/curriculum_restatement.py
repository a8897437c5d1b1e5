"""The statistics per puzzle, the sampling weights and the weighted draw (``pw_episode_stats`` / ``pw_curriculum_update`` /
``pw_resample_weighted``) restated in numpy and plain Python integers -- a helper module for
tests/test_curriculum_host.py and tests/test_gpu_curriculum.py, not a test itself.  Written from the definitions in
include/pushworld_amd.h; Python integers never overflow, so nothing here depends on a word size."""
import bisect

import numpy as np

from pushworld_amd import _capi

EPISODES, SOLVED, STEPS, SOLVED_STEPS = 0, 1, 2, 3
UNIFORM, FAILURE, FRONTIER, GIVEN = 0, 1, 2, 3
MASK64 = (1 << 64) - 1


def mix64(seed, env, episode):
    """The host copy of the draw's hash (``pw_mix64``)."""
    return int(_capi.lib.pw_mix64(int(seed) & MASK64, int(env), int(episode)))


def episode_stats(stats, puzzle_id, steps, terminated, truncated):
    """Adds the episodes that the flags end to ``stats`` (a list of P rows of four Python integers, or an int64 array),
    in place, and returns it."""
    P = len(stats)
    for pid, n, t, u in zip(np.asarray(puzzle_id).tolist(), np.asarray(steps).tolist(), np.asarray(terminated).tolist(),
                            np.asarray(truncated).tolist()):
        if (t | u) == 0 or t == 0xFF or not 0 <= pid < P:
            continue
        stats[pid][EPISODES] += 1
        stats[pid][STEPS] += n
        if t != 0:
            stats[pid][SOLVED] += 1
            stats[pid][SOLVED_STEPS] += n
    return stats


def weight(mode, n, s, given=0, floor_q16=0):
    """The Q16 weight of one puzzle with ``n`` episodes of which ``s`` were solved."""
    n, s = max(int(n), 0), max(int(s), 0)
    k = max(0, n.bit_length() - 20)
    n1 = n >> k
    s1 = min(s >> k, n1)
    f1 = n1 - s1
    if mode == UNIFORM:
        w = 65536
    elif mode == FAILURE:
        w = (65536 * (f1 + 1)) // (n1 + 2)
    elif mode == FRONTIER:
        assert 262144 * (s1 + 1) * (f1 + 1) < 1 << 61
        w = (262144 * (s1 + 1) * (f1 + 1)) // ((n1 + 2) ** 2)
    elif mode == GIVEN:
        w = int(given)
    else:
        raise ValueError(mode)
    w = max(w, int(floor_q16))
    assert 0 <= w < 1 << 32
    return w


def curriculum_update(mode, stats, base=None, given=None, floor_q16=0, num_puzzles=None):
    """``(weights, cdf)`` as lists of Python integers."""
    P = num_puzzles if num_puzzles is not None else len(stats)
    weights = []
    for p in range(P):
        n = s = 0
        if mode in (FAILURE, FRONTIER):
            n, s = int(stats[p][EPISODES]), int(stats[p][SOLVED])
            if base is not None:
                n, s = n - int(base[p][EPISODES]), s - int(base[p][SOLVED])
        weights.append(weight(mode, n, s, given[p] if mode == GIVEN else 0, floor_q16))
    cdf, total = [], 0
    for w in weights:
        total += w
        cdf.append(total)
    assert total < 1 << 64
    return weights, cdf


def draw(cdf, r):
    """The puzzle drawn with the 64-bit random word ``r``."""
    P, total = len(cdf), int(cdf[-1])
    if total == 0:
        return (r * P) >> 64
    t = (r * total) >> 64
    return bisect.bisect_right(cdf, t)  # the smallest p with cdf[p] > t


def resample_weighted(puzzle_id, episode, seed, cdf, terminated=None, truncated=None):
    """New ``(puzzle_id, episode)`` arrays (int64 / uint32 values as Python-sized integers in int64 arrays)."""
    cdf = [int(c) for c in cdf]
    pid = np.array(puzzle_id, dtype=np.int64)
    ep = np.array(episode, dtype=np.int64) & 0xFFFFFFFF
    B = len(pid)
    redraw = np.ones(B, bool) if terminated is None and truncated is None else np.zeros(B, bool)
    for f in (terminated, truncated):
        if f is not None:
            redraw |= np.asarray(f) != 0
    for i in np.flatnonzero(redraw).tolist():
        ep[i] = (ep[i] + 1) & 0xFFFFFFFF
        pid[i] = draw(cdf, mix64(seed, i, int(ep[i])))
    return pid, ep


def resample_uniform(puzzle_id, episode, seed, num_puzzles, terminated=None, truncated=None):
    """``pw_resample`` without a table, the same way."""
    return resample_weighted(puzzle_id, episode, seed, [0] * num_puzzles, terminated, truncated)

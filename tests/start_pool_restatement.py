"""Start-state pools (``pw_start_pool_arm`` / ``pw_start_pool_draw`` / ``pw_start_pool_update_bands``) restated
in numpy and plain Python integers -- a helper module for tests/test_start_pool_host.py and tests/test_gpu_start_pool.py, not
a test itself.  Written from the definitions in include/pushworld_amd.h; Python integers never overflow, so nothing here
depends on a word size."""
import numpy as np

from pushworld_amd import _capi

MASK64 = (1 << 64) - 1
K_DRAW = 0x8EBC6AF09C88C6E3
K_KEEP = 0x589965CC75374CC3


def mix64(seed, env, ctr):
    """The host copy of the draw's hash (``pw_mix64``)."""
    return int(_capi.lib.pw_mix64(int(seed) & MASK64, int(env), int(ctr)))


def group(puzzle, level, num_puzzles):
    """``(order, max_level, lvl_off, start)`` as lists: the buckets one after the other, puzzle by puzzle and level by level,
    each in ascending entry index."""
    puzzle, level = [int(p) for p in puzzle], [int(v) for v in level]
    order, max_level, lvl_off, start = [], [], [], []
    for p in range(num_puzzles):
        mine = [e for e in range(len(puzzle)) if puzzle[e] == p]
        ml = max((level[e] for e in mine), default=-1)
        max_level.append(ml)
        lvl_off.append(len(start))
        for lv in range(ml + 1):
            start.append(len(order))
            order += [e for e in mine if level[e] == lv]
        start.append(len(order))  # the word behind the last level (the only word of a puzzle without entries)
    return order, max_level, lvl_off, start


def arm(terminated, truncated):
    return ((np.asarray(terminated) | np.asarray(truncated)) != 0).astype(np.uint8)


class Pool:
    """The arrays a draw reads."""

    def __init__(self, puzzle, level, pos, num_puzzles):
        self.puzzle, self.level, self.pos = np.asarray(puzzle), np.asarray(level), np.asarray(pos)
        self.num_puzzles = num_puzzles
        self.order, self.max_level, self.lvl_off, self.start = group(puzzle, level, num_puzzles)


def draw(pool, puzzle_id, pos, steps, terminated, truncated, counter, entry, level, seed=0, mask=None, band=None, lo_n=None,
         hi_n=None, lo=0, hi=-1, keep_q16=0):
    """One draw IN PLACE on numpy arrays (``terminated`` / ``truncated`` may be None; ``counter`` holds uint32 values in a wider
    integer type).  The band is ``lo_n`` / ``hi_n`` per environment, else ``band`` ``[P][2]`` per puzzle, else ``lo`` / ``hi``."""
    S = len(pool.order)
    for i in range(len(puzzle_id)):
        if mask is not None and mask[i] == 0:
            continue
        p = int(puzzle_id[i])
        if not 0 <= p < pool.num_puzzles or pool.max_level[p] < 0:
            entry[i] = level[i] = -1
            continue
        ml = pool.max_level[p]
        if lo_n is not None:
            a, b = int(lo_n[i]), int(hi_n[i])
        elif band is not None:
            a, b = int(band[p][0]), int(band[p][1])
        else:
            a, b = int(lo), int(hi)
        if b < 0:
            b = ml
        b = max(b, a)
        a, b = min(max(a, 0), ml), min(max(b, 0), ml)
        first, end = pool.start[pool.lvl_off[p] + a], pool.start[pool.lvl_off[p] + b + 1]
        if end <= first or end > S:
            entry[i] = level[i] = -1
            continue
        ctr = (int(counter[i]) + 1) & 0xFFFFFFFF
        counter[i] = ctr
        if keep_q16 > 0 and (mix64(seed ^ K_KEEP, i, ctr) >> 48) < keep_q16:
            entry[i] = level[i] = -1
            continue
        u = (mix64(seed ^ K_DRAW, i, ctr) * (end - first)) >> 64
        e = pool.order[first + u]
        pos[i] = pool.pos[e]
        steps[i] = 0
        if terminated is not None:
            terminated[i] = 0
        if truncated is not None:
            truncated[i] = 0
        entry[i] = e
        level[i] = pool.level[e]


def update_bands(max_level, stats, base, band, min_episodes=32, up_q16=52429, down_q16=13107, step=1, width=0, hi_min=1,
                 lo_min=1):
    """One band update IN PLACE on ``base`` and ``band`` (lists of lists or integer arrays); returns ``delta`` as a list."""
    delta = []
    for p in range(len(max_level)):
        ml = int(max_level[p])
        if ml < 0:
            delta.append(None)  # not written
            continue
        n = max(int(stats[p][0]) - int(base[p][0]), 0)
        s = min(max(int(stats[p][1]) - int(base[p][1]), 0), n)
        if n < min_episodes:
            delta.append(None)
            continue
        k = max(0, n.bit_length() - 20)
        n, s = n >> k, s >> k
        lo, hi = int(band[p][0]), int(band[p][1])
        if hi < 0:
            hi = ml
        was = hi
        if s * 65536 >= up_q16 * n:
            hi = min(hi + step, ml)
        elif s * 65536 < down_q16 * n:
            hi = max(hi - step, min(hi_min, ml))
        if width > 0:
            lo = max(lo_min, hi - width + 1)
        band[p][0], band[p][1] = lo, hi
        for c in range(4):
            base[p][c] = int(stats[p][c])
        delta.append((hi > was) - (hi < was))
    return delta

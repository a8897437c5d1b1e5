"""numpy / plain-Python restatement of the draws of ``pw_*_sample`` and the walks of ``pw_*_plans`` (include/pushworld_amd.h,
csrc/pw_table_sample.inc): what the kernels must compute, given a table's rows and its cost index as read back."""
import numpy as np

from test_gpu_vector import M64, mix64  # the numpy restatement of pw_mix64 that the resample tests check against the library

K_SAMPLE, K_PLAN = 0xA0761D6478BD642F, 0xE7037ED1A0B428DB
INF = 0xFFFF


def hash64(seed: int, a: int, b: int) -> int:
    return int(mix64(seed & M64, np.array([a], dtype=np.uint64), np.array([b], dtype=np.uint64))[0])


def clamp_band(lo: int, hi: int, max_cost: int):
    """The band as the kernel reads it: hi < lo is hi = lo, then both into 0 .. max_cost."""
    hi = max(hi, lo)
    return min(max(lo, 0), max_cost), min(max(hi, 0), max_cost)


def draw_row(seed: int, env: int, counter: int, lo: int, hi: int, rows_by_cost, cost_start):
    """The row environment ``env`` draws with its counter ALREADY advanced to ``counter``; None when the table has no
    finite-cost row (the kernel then writes -1 / -1 and does not advance the counter)."""
    max_cost = len(cost_start) - 3
    if int(cost_start[max_cost + 1]) == 0:
        return None
    lo, hi = clamp_band(lo, hi, max_cost)
    first, count = int(cost_start[lo]), int(cost_start[hi + 1]) - int(cost_start[lo])
    u = (hash64(seed ^ K_SAMPLE, env, counter) * count) >> 64
    return int(rows_by_cost[first + u])


def walk_plan(acts, succ, cost, row: int, tie: int, seed: int, item: int):
    """The plan from ``row``: None at a dead end; tie 0 the lowest optimal action, tie 1 the j-th set bit of acts & 15 with
    j = floor(mix64(seed ^ K_PLAN, item, t) * popcount / 2^64)."""
    if int(cost[row]) == INF:
        return None
    plan, i, t = [], int(row), 0
    while int(cost[i]) != 0:
        bits = int(acts[i]) & 15
        if tie:
            j = (hash64(seed ^ K_PLAN, item, t) * bin(bits).count("1")) >> 64
            for _ in range(j):
                bits &= bits - 1
        a = (bits & -bits).bit_length() - 1
        plan.append(a)
        i = int(succ[i][a])
        t += 1
    return plan

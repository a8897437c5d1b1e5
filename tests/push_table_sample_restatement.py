"""Plain-Python restatement of drawing from the cost-to-go tables over pushes (``pw_push_search_table_index`` / ``_sample`` /
``_plans`` / ``_emit``) over ``push_table_restatement.Table`` and ``table_sample_restatement``'s ``mix64``.  A helper
of tests/test_push_table_sample_host.py and tests/test_gpu_push_table_sample.py, not a test.

The index groups the STATES by cost, the dead ends last, in ascending store index inside a bucket.  A draw is K14's, over
states.  A plan takes, at every state, its ``best`` row (tie 0) or the j-th of its optimal rows (tie 1).  The emitted states are
computed FROM THE ORACLE: from the live state, walk along ``walk_restatement.path`` to the push's position with the C oracle's
step, then push with it -- never from the store's successor, so that the identity the kernel relies on is itself under test."""
from collections import namedtuple

import push_table_restatement as TR
import walk_restatement as WR
from table_sample_restatement import K_PLAN, K_SAMPLE, clamp_band, hash64

Step = namedtuple("Step", "frm action node")
Row = namedtuple("Row", "item t node frm action cost pos")


def cost_index(t):
    """(states_by_cost, cost_start) of a ``Table``: cost_start has max_cost + 3 words, [0, S] when no cost is finite."""
    mc = t.info[4]
    buckets = [[] for _ in range(mc + 2)]
    for i, c in enumerate(t.cost):  # ascending store index inside every bucket
        buckets[c if c >= 0 else mc + 1].append(i)
    start = [0]
    for b in buckets:
        start.append(start[-1] + len(b))
    return [i for b in buckets for i in b], start


def draw_state(seed, env, counter, lo, hi, states_by_cost, cost_start):
    """The state environment ``env`` draws with its counter ALREADY advanced to ``counter``; None when the table has no state of
    finite cost or the clamped band holds no state (the kernel then writes -1 / -1 and does not advance the counter)."""
    mc = len(cost_start) - 3
    if mc < 0 or int(cost_start[mc + 1]) == 0:
        return None
    lo, hi = clamp_band(lo, hi, mc)
    first, count = int(cost_start[lo]), int(cost_start[hi + 1]) - int(cost_start[lo])
    if count == 0:
        return None
    u = (hash64(seed ^ K_SAMPLE, env, counter) * count) >> 64
    return int(states_by_cost[first + u])


def plan(t, state, tie, seed, item):
    """The plan from store index ``state`` as a list of ``Step``s; None at a dead end or outside the store."""
    if not 0 <= state < t.info[0] or t.cost[state] < 0:
        return None
    steps, i, k = [], state, 0
    while t.cost[i] > 0:
        lo, hi = t.row_off[i], t.row_off[i + 1]
        if tie:
            optimal = [r for r in range(lo, hi) if t.flags[r] & TR.OPTIMAL]
            r = optimal[(hash64(seed ^ K_PLAN, item, k) * len(optimal)) >> 64]
        else:
            r = lo + t.best[i]
        steps.append(Step(tuple(t.frm[r]), t.action[r], i))
        k += 1
        if t.flags[r] & TR.GOAL:  # a goal row ends the plan, whatever its successor is
            break
        i = t.succ[r]
    assert len(steps) == t.cost[state]
    return steps


def states_along(cp, start, steps):
    """The states the pushes of ``steps`` are made from, from the oracle alone: ``start``, then after every push but the
    last -- walk to the push's position along the region's parent actions, then push; and the state after the last push."""
    out, state = [], tuple(tuple(xy) for xy in start)
    for s in steps:
        out.append(state)
        for a in WR.path(WR.region(cp, state), s.frm) + [s.action]:
            state = tuple(tuple(xy) for xy in cp.get_next_state(state, a))
    return out, state


def rows(cp, t, item, start, steps):
    """The emitted rows of one item whose live state is ``start`` (None: the stored state of its first node)."""
    if not steps:
        return []
    if start is None:
        start = t.store.states[steps[0].node]
    along, _ = states_along(cp, start, steps)
    return [Row(item, k, s.node, s.frm, s.action, len(steps) - k, along[k]) for k, s in enumerate(steps)]

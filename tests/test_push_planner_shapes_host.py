"""The inputs of tests/test_gpu_push_planner_shapes.py, pinned on the CPU before a device sees them: the runs of the best-first
search over pushes listed in tests/shape_states.py (``PLANNER_*``), restated by tests/push_planner_restatement.py.
  * the ten info words of every run, as literals;
  * the coverage conditions each group of runs was chosen for, asserted from the restatement alone: queues of NaN keys only, of
    finite and +inf keys, of all three classes with a pop from each, goal rows with a successor outside the grid, exhaustion and
    `limit` from overlapping starts, rounds that pop more than 256 states, 18 movables, 16-padded rows.
``restated(run)`` computes a run once per session, round by round, and keeps the key of every state and what every round
popped; the runs on one puzzle share the RGD movement graphs.  The 64 x 64 board is not among the runs: one round from its
initial state takes the restatement 79 s (101 regions of about 2 500 positions)."""
import math
import time
from collections import namedtuple

import pytest

import push_planner_restatement as PP
import shape_states as SS
import walk_restatement as WR
from oracle import pw_oracle
from test_push_planner_host import check_store_invariants, level1, oracles

# what one round popped: the store indices in pop order, their classes (0 finite, 1 +inf, 2 NaN), the buckets and the open
# entries before the round, the push rows of the popped states and the states the round appended
Round = namedtuple("Round", "pops classes buckets open rows appended")
Restated = namedtuple("Restated", "ref keys rounds seconds")

_ORACLES, _GRAPHS, _RUNS = {}, {}, {}

# status, rounds, expanded, states, open, goal index, RGD overruns, push rows, largest region, largest key
PINNED_NAN = [
    ("running", 6, 21, 59, 38, -1, 0, 143, 74, -1),
    ("running", 6, 71, 94, 23, -1, 0, 314, 81, -1),
    ("exhausted", 5, 25, 25, 0, -1, 0, 72, 89, -1),
    ("solved", 5, 5, 7, 1, 6, 0, 14, 63, -1),
    ("running", 6, 21, 124, 103, -1, 0, 547, 261, -1),
    ("running", 6, 252, 705, 453, -1, 0, 2762, 175, -1),
    ("solved", 2, 5, 28, 16, 27, 0, 73, 259, -1),
    ("running", 6, 21, 90, 69, -1, 0, 174, 47, -1),
    ("running", 6, 6, 29, 23, -1, 0, 43, 27, -1),
    ("running", 6, 241, 733, 492, -1, 0, 1832, 28, -1),
    ("solved", 2, 2, 15, 8, 14, 0, 34, 32, -1),
]
PINNED_MIXED = [
    ("running", 5, 17, 57, 40, -1, 0, 120, 13, 31),
    ("running", 5, 83, 123, 40, -1, 0, 527, 16, 32),
    ("running", 5, 17, 38, 21, -1, 0, 106, 21, 32),
    ("running", 5, 31, 40, 9, -1, 0, 165, 21, 32),
    ("running", 5, 16, 18, 2, -1, 0, 85, 18, 29),
    ("running", 5, 17, 18, 1, -1, 0, 90, 18, 29),
    ("running", 5, 17, 59, 42, -1, 0, 110, 10, 31),
    ("running", 5, 94, 139, 45, -1, 0, 528, 13, 31),
]
PINNED_BUDGET = [
    ("running", 64, 253, 261, 8, -1, 7, 1350, 29, 32),
    ("running", 87, 345, 352, 7, -1, 9, 1805, 29, 32),
]
PINNED_GOAL_OUTSIDE = [
    ("solved", 3, 27, 35, 0, 34, 0, 135, 44, -1),
    ("solved", 6, 6, 38, 28, 37, 0, 101, 68, -1),
    ("solved", 3, 70, 106, 0, 105, 0, 639, 68, -1),
    ("solved", 1, 1, 6, 0, 5, 0, 18, 25, -1),
    ("solved", 1, 1, 4, 0, 3, 0, 15, 35, -1),
]
PINNED_EXHAUSTED = [
    ("exhausted", 3, 3, 3, 0, -1, 0, 2, 14, -1),
    ("exhausted", 3, 3, 3, 0, -1, 0, 2, 14, -1),
]
PINNED_WIDE = [
    ("running", 7, 961, 1753, 792, -1, 0, 10709, 52, 17),
    ("running", 7, 1362, 2118, 756, -1, 0, 14784, 52, 17),
]
PINNED_18 = [
    ("running", 5, 17, 176, 159, -1, 0, 675, 249, 87),
    ("running", 5, 17, 131, 114, -1, 0, 621, 228, 87),
]
PINNED_16 = [
    ("running", 2, 5, 143, 138, -1, 0, 631, 737, 31),
    ("running", 2, 5, 137, 132, -1, 0, 559, 745, 31),
]
PINNED_LIMIT = ("limit", 4, 54, 54, 0, -1, 0, 291, 7, 29)
PINNED = dict(zip(SS.PLANNER_RUNS, PINNED_NAN + PINNED_MIXED + PINNED_BUDGET + PINNED_GOAL_OUTSIDE + PINNED_EXHAUSTED + PINNED_WIDE +
                  PINNED_18 + PINNED_16 + [PINNED_LIMIT]))


def run_id(run):
    start = "initial" if run.start is None else (str(run.start) if isinstance(run.start, int) else "state %d.." % run.start[0][0])
    return "%s-%s-K%d-b%s-m%s-r%s" % (run.case, start, run.k, run.budget, run.max_states, run.rounds)


def oracles_of(case):
    """(C oracle puzzle, Python oracle puzzle with its collision tables) of a case of shape_states or a Level-1 puzzle."""
    if isinstance(case, str):
        return oracles(case, level1(case))
    if case not in _ORACLES:
        _ORACLES[case] = (SS.puzzle(case), pw_oracle.OraclePuzzle(SS.text(case)))
    return _ORACLES[case]


def text_of(case):
    return level1(case) if isinstance(case, str) else SS.text(case)


def restated(run):
    """``Restated`` of a ``shape_states.PlannerRun``: computed once per session, round by round, and never changed."""
    if run not in _RUNS:
        t0 = time.perf_counter()
        cp, oz = oracles_of(run.case)
        ref = PP.PushPlannerRestatement(cp, oz, batch=run.k, max_states=1 << 20 if run.max_states is None else run.max_states,
                                        rgd_budget=run.budget, graphs=_GRAPHS.get(run.case))
        _GRAPHS[run.case] = ref.rgd.graphs
        keys, key_of = [], ref.key

        def key(state):  # the keys in the order of their evaluation, which is store order
            keys.append(key_of(state))
            return keys[-1]

        ref.key = key
        ref.begin(SS.planner_start(run))
        rounds = []
        while ref.status == "running" and (run.rounds is None or ref.rounds < run.rounds):
            before = {b: list(v) for b, v in ref.buckets.items()}
            open_, n, done = ref.open, len(ref.states), ref.rounds
            ref.run(1)
            if ref.rounds == done:  # the verdict `exhausted`: no round
                continue
            left = {i for v in ref.buckets.values() for i in v}
            gone = sorted(((b, -i) for b, v in before.items() for i in v if i not in left))  # lowest bucket, then newest, first
            pops = [-i for _, i in gone]
            rows = sum(len(WR.region(cp, ref.states[i]).pushes) for i in pops)
            rounds.append(Round(pops, [b[0] for b, _ in gone], len(before), open_, rows, len(ref.states) - n))
        _RUNS[run] = Restated(ref, keys, rounds, time.perf_counter() - t0)
    return _RUNS[run]


def classes(keys):
    """(finite keys, +inf keys, NaN keys) of a list of keys."""
    nan = [k for k in keys if k != k]
    inf = [k for k in keys if k == k and math.isinf(k)]
    return [k for k in keys if k == k and not math.isinf(k)], inf, nan


def test_runs_and_pins_line_up():
    assert len(PINNED) == len(SS.PLANNER_RUNS) == len(set(SS.PLANNER_RUNS)) == 35
    assert [PINNED[r] for r in SS.PLANNER_NAN] == PINNED_NAN and PINNED[SS.PLANNER_LIMIT] == PINNED_LIMIT


@pytest.mark.parametrize("run", SS.PLANNER_RUNS, ids=run_id)
def test_pinned(run):
    cp, _ = oracles_of(run.case)
    got = restated(run)
    ref = got.ref
    print(run_id(run), "%.1f s" % got.seconds)
    assert tuple(ref.info()) == PINNED[run]
    check_store_invariants(cp, ref)
    # the rounds as recorded: pops lowest class first, every state keyed once unless the search ended in its round
    assert len(got.rounds) == ref.rounds and sum(len(r.pops) for r in got.rounds) == ref.expanded
    assert all(r.classes == sorted(r.classes) and len(r.pops) == min(run.k, r.open) for r in got.rounds)
    assert sum(r.rows for r in got.rounds) == ref.push_rows
    keyed = len(ref.states) - (got.rounds[-1].appended if ref.status == "solved" else 0)
    assert len(got.keys) == keyed and ref.open + ref.expanded == keyed
    start = SS.planner_start(run)
    assert start is None or (WR.in_grid(cp, start) and ref.states[0] == tuple(start))


def test_nan_only_runs():
    most, overlapping = 0, set()
    for run in SS.PLANNER_NAN:
        cp, _ = oracles_of(run.case)
        got = restated(run)
        finite, inf, nan = classes(got.keys)
        assert not finite and not inf and len(nan) == len(got.keys) >= 1  # a movable off its graph: no overrun either
        assert got.ref.largest_key == -1 and got.ref.rgd_exceeded == 0
        assert all(r.buckets == 1 and set(r.classes) == {2} for r in got.rounds)
        assert all(r.pops == sorted(r.pops, reverse=True) for r in got.rounds)  # newest first
        most = max(most, len(got.ref.states))
        if SS.overlapping(cp, SS.planner_start(run)):
            overlapping.add(run.case)
    assert most > 500 and overlapping == set(SS.SMALL)
    assert {restated(r).ref.status for r in SS.PLANNER_NAN} == {"running", "exhausted", "solved"}
    ended = [r for r in SS.PLANNER_NAN if restated(r).ref.status == "exhausted"]
    assert ended and all(SS.overlapping(oracles_of(r.case)[0], SS.planner_start(r)) for r in ended)


def test_mixed_runs():
    cp, _ = oracles_of(SS.CASES[2])
    assert sum(SS.overlapping(cp, SS.states(SS.CASES[2])[s].state) for s in SS.PLANNER_MIXED_LISTED) >= 3
    for run in SS.PLANNER_MIXED:
        got = restated(run)
        finite, inf, nan = classes(got.keys)
        assert not nan and len(inf) >= 9 and len(set(finite)) >= 3
    assert any({0, 1} <= set(r.classes) for run in SS.PLANNER_MIXED for r in restated(run).rounds)  # one round pops from both


def test_budget_runs():
    assert SS.PLANNER_BUDGET == 32
    for run in SS.PLANNER_BUDGET_RUNS:
        got = restated(run)
        finite, inf, nan = classes(got.keys)
        assert min(len(finite), len(inf), len(nan)) >= 3 and got.ref.rgd_exceeded == len(nan)
        first = {c: min(k for k, r in enumerate(got.rounds) if c in r.classes) for c in (0, 1, 2)}  # a pop from each class
        assert first[0] == 0 < first[1] < first[2] == run.rounds - 1  # (the round count is the first that pops a NaN entry)
        assert {0} == set(got.rounds[7].classes)  # eight rounds pop finite keys only
        # the finite and the +inf buckets have drained at least once
        assert any(r.classes[0] == 1 for r in got.rounds) and got.rounds[-1].classes[-1] == 2
    # the same searches with the default budget overrun nowhere
    assert restated(SS.PLANNER_MIXED[0]).ref.rgd_exceeded == restated(SS.PLANNER_MIXED[6]).ref.rgd_exceeded == 0


def test_goal_outside_runs():
    latest = 0
    for run in SS.PLANNER_GOAL_OUTSIDE:
        cp, _ = oracles_of(run.case)
        ref = restated(run).ref
        assert ref.status == "solved" and ref.goal_index == len(ref.states) - 1
        assert not WR.in_grid(cp, ref.states[-1]) and ref.canons[-1] == (0, 0)
        assert all(WR.in_grid(cp, s) for s in ref.states[:-1])
        pushes = check_store_invariants(cp, ref)  # (replays the plan through the C oracle into a goal state)
        assert pushes >= 1 and SS.overlapping(cp, SS.planner_start(run))
        latest = max(latest, ref.rounds)
    assert latest >= 3 and sum(restated(r).ref.rounds >= 3 for r in SS.PLANNER_GOAL_OUTSIDE) >= 3


def test_exhausted_from_the_initial_state_of_the_30_x_30_board():
    for run in SS.PLANNER_EXHAUSTED:
        got = restated(run)
        finite, inf, nan = classes(got.keys)
        assert got.ref.status == "exhausted" and len(inf) == len(got.keys) == 3 and got.ref.largest_key == -1
        assert SS.PADDING[run.case] == 8 and SS.FRAME[run.case] == 32


def test_rounds_that_pop_more_than_256():
    k300, k1000 = (restated(run) for run in SS.PLANNER_WIDE)
    assert (SS.PLANNER_WIDE[0].k, SS.PLANNER_WIDE[1].k) == (300, 1000)
    full = [r for r in k300.rounds if len(r.pops) == 300 and r.open > 300 and r.buckets >= 10]
    assert len(full) >= 2 and [(r.open, r.buckets) for r in full] == [(401, 15), (623, 15)]
    part = [r for r in k1000.rounds if 256 < len(r.pops) < 1000]
    assert len(part) >= 2 and [len(r.pops) for r in part] == [401, 600]
    assert all(len(r.pops) == r.open for r in part)  # the whole open list
    assert max(k300.seconds, k1000.seconds) < 60  # (about 13 s each where the round counts were chosen)


def test_18_movables():
    cp, _ = oracles_of(SS.CASES[4])
    assert cp.num_movables == 18 and SS.PADDING[SS.CASES[4]] == 32
    for run in SS.PLANNER_18:
        got = restated(run)
        finite, inf, nan = classes(got.keys)
        assert len(got.ref.states) > 100 and len(set(finite)) > 10 and not nan
    assert [SS.overlapping(cp, SS.planner_start(r)) for r in SS.PLANNER_18] == [False, True]


def test_16_padded_rows():
    cp, _ = oracles_of(SS.CASES[3])
    assert cp.num_movables == 12 and SS.PADDING[SS.CASES[3]] == 16
    for run in SS.PLANNER_16:
        got = restated(run)
        assert run.rounds == SS.PLANNER_16_ROUNDS and len(got.ref.states) > 30 and got.ref.largest_region > 700
    assert [SS.overlapping(cp, SS.planner_start(r)) for r in SS.PLANNER_16] == [False, True]


def test_limit_from_an_overlapping_start():
    run = SS.PLANNER_LIMIT
    cp, _ = oracles_of(run.case)
    got = restated(run)
    ref, last = got.ref, got.rounds[-1]
    assert SS.overlapping(cp, SS.planner_start(run))
    assert ref.status == "limit" and ref.rounds >= 3 and last.appended == 0 and ref.plan() is None
    assert last.rows > 0 and len(ref.states) + last.rows > run.max_states  # the refused round's T is counted
    assert ref.push_rows == sum(r.rows for r in got.rounds) and all(r.appended > 0 for r in got.rounds[:-1])
    free = restated(SS.PLANNER_MIXED[7])  # the same search without the limit
    assert free.ref.states[:len(ref.states)] == ref.states and free.ref.links[:len(ref.states)] == ref.links
    assert [r.pops for r in free.rounds[:ref.rounds]] == [r.pops for r in got.rounds]

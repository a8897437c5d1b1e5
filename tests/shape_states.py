"""The random-shape puzzles of tests/test_gpu_shapes.py and seeded lists of their states -- overlapping ones above all -- for
the walk-region and push-search tests (tests/test_walk_shapes_host.py, test_gpu_walk_shapes.py, test_gpu_push_search_shapes.py).
The runs of the best-first search over pushes (``PLANNER_*``, tests/test_push_planner_shapes_host.py and
test_gpu_push_planner_shapes.py) and the push-step tests (test_gpu_push_step_shapes.py) use the same puzzles and lists.
A helper, not a test.  Everything is in Python object order (``oracle.c_oracle.COraclePuzzle(text)``).

Per case (n_movables, size, seed) the puzzle is the first draw of ``random_puzzle(np.random.default_rng(1000 + seed), n, size)``
and the list holds, in this order,
  initial    the initial state
  near       the initial state with about 30 % of the movables shifted by up to 2 cells either way, clipped to the frame
  far        ``random_states``: every movable anywhere inside the frame, border cells included, overlaps allowed
  goal_near  a far state with every goal movable one cell from its goal position, in a seeded direction
The seeds of the classes were chosen so that the lists meet the coverage conditions that tests/test_walk_shapes_host.py
asserts from the restatement; nothing is dropped from a list."""
from collections import namedtuple

import numpy as np

import push_search_restatement as PR
import walk_restatement as WR
from oracle import c_oracle
from test_gpu_shapes import random_puzzle, random_states

CASES = [(3, 12, 9), (5, 30, 1), (8, 16, 2), (12, 30, 4), (18, 30, 6), (32, 62, 5)]
SMALL = CASES[:3]  # the cases whose searches over pushes a CPU restates in seconds
PADDING = {CASES[0]: 4, CASES[1]: 8, CASES[2]: 8, CASES[3]: 16, CASES[4]: 32, CASES[5]: 32}
FRAME = {CASES[0]: 14, CASES[1]: 32, CASES[2]: 18, CASES[3]: 32, CASES[4]: 32, CASES[5]: 64}
AGENT = {CASES[0]: (8, 1), CASES[1]: (9, 8), CASES[2]: (8, 7), CASES[3]: (1, 1), CASES[4]: (1, 7), CASES[5]: (4, 1)}
# (near, far, goal_near) states per case; the restatement takes about 0.75 s per state of the 64 x 64 board
COUNTS = {c: (12, 12, 6) for c in CASES[:5]}
COUNTS[CASES[5]] = (3, 4, 0)
# (near, far, goal_near) seeds per case
SEEDS = {
    CASES[0]: (1, 4, 4),
    CASES[1]: (2, 4, 0),
    CASES[2]: (0, 3, 4),
    CASES[3]: (2, 0, 5),
    CASES[4]: (3, 1, 5),
    CASES[5]: (0, 4, 0),
}
DISPLACEMENTS = WR.DISPLACEMENTS

# Starts of the searches over pushes, chosen on the CPU (tests/test_walk_shapes_host.py asserts what they were chosen for).
# SEARCH_STARTS: four overlapping starts per small case from which three layers of pushes close 20 .. 400 canonical states and
# list rows whose successor lies outside the grid -- indices into states(case), or states out of far_states(seed 100).
SEARCH_STARTS = {
    CASES[0]: [((5, 12), (5, 2), (9, 12)), ((0, 12), (5, 5), (3, 9)), ((6, 9), (3, 9), (9, 3)), ((6, 3), (5, 6), (3, 4))],
    CASES[1]: [13, 20, 18, 19],
    CASES[2]: [14, 18, 20, 21],
}
# further starts of the searches that stop at a goal (beside the goal_near states of the lists, one push from a goal): their
# first goal row comes in the second or third layer
DEEP_GOAL_STARTS = {
    CASES[0]: [((6, 5), (4, 7), (4, 8))],
    CASES[1]: [((23, 9), (19, 16), (9, 17), (2, 18), (24, 21))],
    CASES[2]: [((2, 8), (11, 13), (8, 5), (1, 4), (6, 11), (15, 10), (16, 9), (15, 3)),
               ((1, 8), (11, 13), (5, 5), (3, 4), (9, 13), (9, 9), (1, 11), (6, 0))],
}
# Starts of (8, 16, 2) whose search ends at a goal row with a successor OUTSIDE the grid -- the row that
# pw_push_search_publish_kernel publishes although it owns no canonical state.  Found by a seeded search: state 7 of
# goal_near_states(seed 104) (the goal row in layer 3, as state 31) and state 82 of far_states(seed 102) (layer 3, state 107);
# states 29 and 30 of the list meet such a row in their first layer.
GOAL_OUTSIDE_STARTS = [
    ((1, 11), (12, 12), (12, 7), (16, 1), (14, 13), (7, 4), (5, 0), (0, 2)),
    ((10, 6), (10, 12), (14, 5), (1, 2), (15, 1), (16, 0), (3, 1), (6, 2)),
]
GOAL_OUTSIDE_LISTED = [29, 30]
# One overlapping start each of the two 32-padded cases for a single layer of pushes (every successor's region is restated,
# so the start of the 64 x 64 board is one with the agent shut into a region of 89 positions: state 9 of far_states(seed 103)).
MANY_START_18 = 15  # index into states(CASES[4]): 112 push rows, 6 of them out of the grid
MANY_START_32 = ((52, 13), (9, 51), (14, 27), (49, 37), (32, 1), (54, 10), (18, 49), (49, 4), (6, 7), (59, 25), (39, 6),
                 (3, 37), (19, 8), (49, 50), (45, 10), (54, 45), (43, 18), (50, 48), (1, 18), (5, 55), (53, 0), (43, 0),
                 (15, 30), (33, 21), (55, 19), (9, 42), (44, 13), (53, 49), (3, 60), (47, 31), (7, 33), (44, 30))

# Runs of the best-first search over pushes (pw_push_planner_*, K17), chosen on the CPU: tests/test_push_planner_shapes_host.py
# asserts what each group was chosen for and pins the ten info words of every run, tests/test_gpu_push_planner_shapes.py sends
# every run through the device.  ``case``: one of CASES, or the name of a Level-1 puzzle; ``start``: None (the initial state),
# an index into states(case), or a state; ``budget`` / ``max_states``: None for the defaults; ``rounds``: None runs to the end.
PlannerRun = namedtuple("PlannerRun", "case start k budget max_states rounds")
# NaN-only queues: a movable of the start is off its movement graph, so every key is NaN and every pop is newest-first out of
# one bucket (733 states from listed 28 of (8, 16, 2)).  All starts overlap.  Six rounds unless the search ends sooner: from
# SEARCH_STARTS[(3, 12, 9)][2] it is exhausted in round 5, from the DEEP_GOAL_STARTS it is solved.
PLANNER_NAN_ROUNDS = 6
PLANNER_NAN = [PlannerRun(case, start, k, None, None, PLANNER_NAN_ROUNDS) for case, start, k in (
    (CASES[0], SEARCH_STARTS[CASES[0]][3], 4), (CASES[0], SEARCH_STARTS[CASES[0]][1], 64), (CASES[0], SEARCH_STARTS[CASES[0]][2], 64),
    (CASES[0], DEEP_GOAL_STARTS[CASES[0]][0], 1),
    (CASES[1], 18, 4), (CASES[1], 19, 64), (CASES[1], DEEP_GOAL_STARTS[CASES[1]][0], 4),
    (CASES[2], 14, 4), (CASES[2], 18, 1), (CASES[2], 28, 64), (CASES[2], DEEP_GOAL_STARTS[CASES[2]][1], 1))]
# finite and +inf keys in one queue: the initial state and three near states of (8, 16, 2); listed 3, 4 and 9 overlap
PLANNER_MIXED_LISTED = [0, 3, 4, 9]
PLANNER_MIXED = [PlannerRun(CASES[2], s, k, None, None, 5) for s in PLANNER_MIXED_LISTED for k in (4, 64)]
# finite, +inf and NaN keys in one queue: 32 RGD frames per state overrun on a few states of (8, 16, 2).  The round counts are
# the first at which a NaN entry is popped at K = 4, i.e. after the finite and the +inf buckets have drained (8 rounds pop
# finite keys only; the first +inf entry pops in round 25 from the initial state, in round 34 from listed 9).
PLANNER_BUDGET = 32
PLANNER_BUDGET_RUNS = [PlannerRun(CASES[2], 0, 4, PLANNER_BUDGET, None, 64), PlannerRun(CASES[2], 9, 4, PLANNER_BUDGET, None, 87)]
# searches of (8, 16, 2) that end at a goal row whose successor lies outside the grid: in round 3 (K = 64) or 6 (K = 1) from
# GOAL_OUTSIDE_STARTS, in round 1 from the listed states
PLANNER_GOAL_OUTSIDE = [PlannerRun(CASES[2], GOAL_OUTSIDE_STARTS[0], 64, None, None, None),
                        PlannerRun(CASES[2], GOAL_OUTSIDE_STARTS[1], 1, None, None, None),
                        PlannerRun(CASES[2], GOAL_OUTSIDE_STARTS[1], 64, None, None, None),
                        PlannerRun(CASES[2], GOAL_OUTSIDE_LISTED[0], 1, None, None, None),
                        PlannerRun(CASES[2], GOAL_OUTSIDE_LISTED[1], 4, None, None, None)]
# the 30 x 30 board with 8-padded rows from its initial state: three states, all keys +inf, exhausted after three rounds
PLANNER_EXHAUSTED = [PlannerRun(CASES[1], None, k, None, None, None) for k in (4, 64)]
# rounds that pop more than 256 states (pw_push_planner_pop_kernel strides K over 256 threads): `Simple Tool` pops 300 of 401
# and of 623 open entries over 15 buckets in rounds 6 and 7 at K = 300, and the whole open list (401, 600) at K = 1000.  Seven
# rounds keep a restatement under 15 s of CPU (`Walk Past` needs over 20 s for five rounds and is left out).
PLANNER_WIDE = [PlannerRun("Simple Tool", None, 300, None, None, 7), PlannerRun("Simple Tool", None, 1000, None, None, 7)]
# 18 movables (32-padded rows, RGD with N > 16): the initial state and listed 3 (which overlaps) of (18, 30, 6)
PLANNER_18 = [PlannerRun(CASES[4], s, 4, None, None, 5) for s in (0, 3)]
# 16-padded rows: the initial state and listed 10 (which overlaps) of (12, 30, 4), regions of about 740 positions
PLANNER_16_ROUNDS = 2  # 143 and 137 states in 18 s and 15 s of CPU; a third round restates about 110 more such regions per start
PLANNER_16 = [PlannerRun(CASES[3], s, 4, None, None, PLANNER_16_ROUNDS) for s in (0, 10)]
# `limit` from an overlapping start: listed 9 of (8, 16, 2) at K = 64 holds 54 states after three rounds and the fourth pops
# 165 push rows, so a store of 150 (rounds 1 .. 3 need at most 106) refuses round 4
PLANNER_LIMIT = PlannerRun(CASES[2], 9, 64, None, 150, None)
PLANNER_RUNS = (PLANNER_NAN + PLANNER_MIXED + PLANNER_BUDGET_RUNS + PLANNER_GOAL_OUTSIDE + PLANNER_EXHAUSTED + PLANNER_WIDE +
                PLANNER_18 + PLANNER_16 + [PLANNER_LIMIT])

Listed = namedtuple("Listed", "kind state")
_TEXT, _PUZZLE, _STATES, _STORES, _REGIONS = {}, {}, {}, {}, {}


def text(case):
    if case not in _TEXT:
        n, size, seed = case
        _TEXT[case] = random_puzzle(np.random.default_rng(1000 + seed), n, size=size)
    return _TEXT[case]


def puzzle(case):
    """The case's oracle puzzle: one object per session, so the restatement's step cache on it is shared."""
    if case not in _PUZZLE:
        _PUZZLE[case] = c_oracle.COraclePuzzle(text(case))
    return _PUZZLE[case]


class _Frame:
    """What ``random_states`` reads of a puzzle, from the oracle's: the frame and the cells of the movables."""

    def __init__(self, cp):
        self.dimensions = (cp.width, cp.height)
        self.movable_objects = [namedtuple("Obj", "cells")(sorted(s)) for s in cp.py.shapes]


def _tuples(rows):
    return [tuple((int(v) // 10000, int(v) % 10000) for v in row) for row in rows]


def near_states(cp, rng, count):
    init = np.array([x * 10000 + y for (x, y) in cp.initial_state], np.int32)
    near = np.repeat(init[None], count, 0)
    jitter = rng.integers(-2, 3, near.shape) * 10000 + rng.integers(-2, 3, near.shape)
    near = near + jitter * (rng.random(near.shape) < 0.3)
    x, y = near // 10000, near % 10000
    for j, (w, h) in enumerate(cp.py.sizes):
        x[:, j] = np.clip(x[:, j], 0, cp.width - w)
        y[:, j] = np.clip(y[:, j], 0, cp.height - h)
    return [tuple((int(a), int(b)) for a, b in zip(xs, ys)) for xs, ys in zip(x, y)]


def far_states(cp, rng, count):
    return _tuples(random_states(rng, _Frame(cp), count))


def goal_near_states(cp, rng, count):
    """Far states with every goal movable one cell from its goal position: the seeded direction, or the next one (L, R, U, D
    in turn) that keeps the movable inside the frame."""
    out = []
    for s in far_states(cp, rng, count):
        s = list(s)
        for g, (gx, gy) in enumerate(cp.py.goal_state):
            w, h = cp.py.sizes[1 + g]
            first = int(rng.integers(0, 4))
            for k in range(4):
                dx, dy = DISPLACEMENTS[(first + k) % 4]
                x, y = gx + dx, gy + dy
                if 0 <= x <= cp.width - w and 0 <= y <= cp.height - h:
                    s[1 + g] = (x, y)
                    break
        out.append(tuple(s))
    return out


def states(case):
    """[Listed(kind, state)] of the case: 1 + near + far + goal_near states, computed once."""
    if case not in _STATES:
        cp = puzzle(case)
        counts, seeds = COUNTS[case], SEEDS[case]
        out = [Listed("initial", cp.initial_state)]
        for kind, make, count, seed in zip(("near", "far", "goal_near"), (near_states, far_states, goal_near_states), counts, seeds):
            if count:
                out += [Listed(kind, s) for s in make(cp, np.random.default_rng(seed), count)]
        _STATES[case] = out
    return _STATES[case]


def region(case, state):
    """``walk_restatement.region`` of a state of the case: computed once per session and never changed."""
    key = (case, tuple(map(tuple, state)))
    if key not in _REGIONS:
        _REGIONS[key] = WR.region(puzzle(case), key[1])
    return _REGIONS[key]


def search_starts(case):
    return [states(case)[s].state if isinstance(s, int) else s for s in SEARCH_STARTS[case]]


def goal_starts(case):
    """The starts of the searches that stop at a goal: the goal_near states of the list, then DEEP_GOAL_STARTS."""
    return [s.state for s in states(case) if s.kind == "goal_near"] + DEEP_GOAL_STARTS[case]


def planner_start(run):
    """The start state of a ``PlannerRun``; None for the initial state of a Level-1 puzzle."""
    if isinstance(run.case, str):
        return None
    if run.start is None:
        return puzzle(run.case).initial_state
    return states(run.case)[run.start].state if isinstance(run.start, int) else run.start


def _cells(cp, state, k):
    x, y = state[k]
    return {(x + cx, y + cy) for cx, cy in cp.py.shapes[k]}


def overlapping(cp, state):
    """True when two movables, or a movable and a wall, share a cell."""
    seen = set(cp.py.wall_cells)
    for k in range(cp.num_movables):
        cells = _cells(cp, state, k)
        if cells & seen:
            return True
        seen |= cells
    return False


def agent_overlaps(cp, state):
    """True when the agent shares a cell with a wall, an agent wall or another movable."""
    mine = _cells(cp, state, 0)
    return bool(mine & cp.py.agent_wall_cells) or any(mine & _cells(cp, state, k) for k in range(1, cp.num_movables))


def store(case, start, **kw):
    """``push_search_restatement.search_store`` of the case from ``start``: computed once per session and never changed."""
    key = (case, tuple(start), tuple(sorted(kw.items())))
    if key not in _STORES:
        _STORES[key] = PR.search_store(puzzle(case), start=start, **kw)
    return _STORES[key]

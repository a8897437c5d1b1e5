"""The random-shape puzzles of tests/test_gpu_shapes.py and seeded lists of their states -- overlapping ones above all -- for
the walk-region and push-search tests (tests/test_walk_shapes_host.py, test_gpu_walk_shapes.py, test_gpu_push_search_shapes.py).
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

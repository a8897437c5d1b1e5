"""The cases of the batched best-first search over pushes at its limits (``pw_push_plan_batch_*``): 6 .. 8
movables, boards 16 cells wide or high, coordinates of 15, RGD budgets that overrun, items of different N in one launch.  A helper
of tests/test_push_plan_batch_limits_host.py (which pins the ten info words of every run below and asserts what each case was
chosen for, from the restatement alone) and tests/test_gpu_push_plan_batch_limits.py (which sends them through the device); not
a test.  Everything is in Python object order (``oracle.c_oracle.COraclePuzzle(text)``).

A ``Run`` names a puzzle (a Level-1 name, a ``(movables, seed)`` pair of ``SHAPES`` or ``"outside8"``), a start (None: the
initial state), K, the largest number of rounds and the RGD budget (None: the default).  ``restated(run)`` restates it once per
session, round by round, with tests/push_planner_restatement.py, and keeps the info words after ``begin`` and after every round:
the store only grows, so the search after r rounds is ``infos[r]`` and the first ``infos[r].states`` entries of the store."""
import time
from collections import namedtuple

import numpy as np

import push_planner_restatement as PP
import shape_states as SS
import walk_restatement as WR
from oracle import c_oracle, pw_oracle
from test_gpu_shapes import random_puzzle
from test_push_planner_host import level1, oracles

Run = namedtuple("Run", "puzzle start k rounds budget")
Restated = namedtuple("Restated", "ref infos seconds")

MAX_STATES = 1 << 14  # (no run comes near it: `Shape Of You` at K = 64 stores 3 020 states and lists 8 675 rows in all)
KS = (1, 8, 64)

# ---- 1. Level-1 puzzles with 6, 7 and 8 movables and the board 16 cells high, with two small ones ------------------------------------
# name: (movables, width, height), the border included
LEVEL1 = {"Victory Road": (6, 7, 14), "Pick A Tool": (6, 11, 8), "Seeing Red": (7, 10, 11), "Shape Of You": (8, 13, 10),
          "Swiss Army Knife": (4, 14, 16), "Single Obstacle": (3, 8, 8), "Two Goals": (3, 10, 11)}
LARGEST_FIRST = ("Shape Of You", "Seeing Red", "Victory Road", "Pick A Tool", "Swiss Army Knife", "Two Goals", "Single Obstacle")
ORDERS = (LARGEST_FIRST, LARGEST_FIRST[::-1])
ROUNDS = 8
LEVEL1_RUNS = [Run(name, None, k, ROUNDS, None) for name in LARGEST_FIRST for k in KS]
LIVE_K, LIVE_ROUNDS, LIVE_ITEMS, LIVE_MAX_STATES = 8, 4, 1500, 1 << 12  # the states form: infos[4] of the runs at K = 8

# ---- 2. random shapes on 16 x 16 frames: (movables, seed) ---------------------------------------------------------------------------
SHAPES = ((8, 2), (8, 3), (6, 1), (7, 5))
SHAPE_SIZE, SHAPE_LISTED = 14, 6  # 14 x 14 cells inside the border; 6 near and 6 far states per case
SHAPE_ROUNDS, SHAPE_COVER_K, SHAPE_COVER_ROUNDS = 8, 8, 4  # (the coverage conditions: K = 8 after four rounds)


def shape_starts(case):
    """The initial state, then ``SHAPE_LISTED`` near and as many far states of the case (seeded by the case's seed)."""
    cp, _ = oracles_of(case)
    return ([tuple(cp.initial_state)] + SS.near_states(cp, np.random.default_rng(case[1]), SHAPE_LISTED) +
            SS.far_states(cp, np.random.default_rng(case[1]), SHAPE_LISTED))


def shape_runs(k):
    return [Run(case, s, k, SHAPE_ROUNDS, None) for case in SHAPES for s in range(1 + 2 * SHAPE_LISTED)]


def outside_start(case):
    """The case's initial state with its last movable shifted so that one of its cells leaves the frame, a different way per
    case: one column past the right edge, one row past the lower edge, x = -1, y = -1.  Every value fits int8."""
    cp, _ = oracles_of(case)
    state = [tuple(xy) for xy in cp.initial_state]
    j = cp.num_movables - 1
    (x, y), (w, h) = state[j], cp.py.sizes[j]
    state[j] = ((cp.width - w + 1, y), (x, cp.height - h + 1), (-1, y), (x, -1))[SHAPES.index(case)]
    return tuple(state)


# ---- 3. RGD budgets that overrun: (puzzle, budget) at K = 8 for at most ten rounds ---------------------------------------------------
BUDGET_K, BUDGET_ROUNDS = 8, 10
BUDGETS = (("Seeing Red", 1), ("Seeing Red", 2), ("Seeing Red", 3), ("Seeing Red", 4), ("Shape Of You", 1), ("Shape Of You", 2),
           ("Shape Of You", 3), ("Victory Road", 1), ("Victory Road", 2), ("Pick A Tool", 4))
BUDGET_RUNS = [Run(name, None, BUDGET_K, BUDGET_ROUNDS, b) for name, b in BUDGETS]

# ---- 4. eight movables; the push that takes m0 to its goal carries the far cell of m6, movable 7, out of the grid ----------------------
OUTSIDE8 = """
M1 M2 M3 M4 M5  .
 .  .  .  .  .  .
 A M0  .  . G0  .
M6  . M6  .  .  .
""".lstrip("\n")
OUTSIDE8_ORDER = ["a", "m0", "m1", "m2", "m3", "m4", "m5", "m6"]
OUTSIDE8_START = ((3, 3), (4, 3), (1, 1), (2, 1), (3, 1), (4, 1), (5, 1), (5, 3))
OUTSIDE8_RUN = Run("outside8", OUTSIDE8_START, 2, None, None)
OUTSIDE8_INSIDE_RUN = Run("outside8", None, 2, 6, None)  # its neighbour in the launch: the initial state, six rounds

# ---- 7. cost_range: `Seeing Red` at K = 8 to its end ---------------------------------------------------------------------------------
RANGE_RUN = Run("Seeing Red", None, 8, None, None)
RANGE_SAME = (26, 64, 65, 4096, 4097)  # the largest key is 25: these ranges hold it, on either side of the bitmap's word boundaries
RANGE_SHORT = 25

_ORACLES, _TEXT, _GRAPHS, _RUNS = {}, {}, {}, {}


def text_of(puzzle):
    if puzzle not in _TEXT:
        if puzzle == "outside8":
            _TEXT[puzzle] = OUTSIDE8
        elif isinstance(puzzle, str):
            _TEXT[puzzle] = level1(puzzle)
        else:
            _TEXT[puzzle] = random_puzzle(np.random.default_rng(2000 + puzzle[1]), puzzle[0], size=SHAPE_SIZE)
    return _TEXT[puzzle]


def oracles_of(puzzle):
    """(C oracle puzzle, Python oracle puzzle with its collision tables): one pair per session."""
    if isinstance(puzzle, str):
        return oracles(puzzle, text_of(puzzle))
    if puzzle not in _ORACLES:
        _ORACLES[puzzle] = (c_oracle.COraclePuzzle(text_of(puzzle)), pw_oracle.OraclePuzzle(text_of(puzzle)))
    return _ORACLES[puzzle]


def start_of(run):
    """The start state of a run, or None for the initial state."""
    if run.start is None or not isinstance(run.start, int):
        return run.start
    return shape_starts(run.puzzle)[run.start]


def restated(run, max_states=MAX_STATES):
    """``Restated`` of a run: computed once per session and never changed.  The runs on one puzzle share the movement graphs."""
    key = (run, max_states)
    if key not in _RUNS:
        t0 = time.perf_counter()
        cp, oz = oracles_of(run.puzzle)
        ref = PP.PushPlannerRestatement(cp, oz, batch=run.k, max_states=max_states, rgd_budget=run.budget,
                                        graphs=_GRAPHS.get(run.puzzle))
        _GRAPHS[run.puzzle] = ref.rgd.graphs
        ref.begin(start_of(run))
        infos = [ref.info()]
        while ref.status == "running" and (run.rounds is None or len(infos) <= run.rounds):
            infos.append(ref.run(1))
        _RUNS[key] = Restated(ref, infos, time.perf_counter() - t0)
    return _RUNS[key]


def after(run, rounds):
    """The info words of a run after at most ``rounds`` rounds."""
    infos = restated(run).infos
    return infos[min(rounds, len(infos) - 1)]


def pushes_of(ref, goal_index=None):
    """The restatement's chain of links from the start to the goal state: [(from, action)]."""
    out, index = [], ref.goal_index if goal_index is None else goal_index
    while ref.links[index].parent >= 0:
        ln = ref.links[index]
        out.append((tuple(ln.frm), ln.action))
        index = ln.parent
    return out[::-1]


def run_id(run):
    start = "initial" if run.start is None else (str(run.start) if isinstance(run.start, int) else "state")
    return "%s-%s-K%d-r%s-b%s" % (run.puzzle, start, run.k, run.rounds, run.budget)


def in_grid(puzzle, state):
    return WR.in_grid(oracles_of(puzzle)[0], state)

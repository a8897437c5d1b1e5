"""Hand-built puzzles that take the recursive graph distance (RGD) heuristic to its limits: `ladder`, whose first finite pushing
depth is as deep as the number of movables allows (up to 32 movables, 30 stack frames), and `room`, the open 64 x 64 board.
tests/test_rgd_puzzles_host.py pins their figures with the plain-Python restatement (tests/rgd_restatement.py); the GPU tests
are in tests/test_gpu_rgd_deep.py.

ladder(k, gap), drawn for k = 4, gap = 1 (`#` is an agent-wall cell, which only the agent cannot enter):

    #  #  #  #  #  #  M2 #  M1 #  #  G1
    #  #  #  #  M3 #  M2 #  #  #  #  #
    #  #  M4 #  M3 #  #  #  #  #  #  #
    A  .  M4 .  .  .  .  .  .  .  .  .

The agent walks the last row only.  M1 is one cell of the top row; M_i (i >= 2) is a vertical piece on rows i - 2 and i - 1, so
it shares a row with M_(i-1) and M_(i+1) alone.  M_i stands `gap` free cells left of M_(i-1) and M_k next to the agent.  Pushed
to the right, M_(i+1) is the only movable that can push M_i, and the agent reaches M_k alone: the cost of G1 is infinite with
fewer than k - 1 tools and finite with k - 1, the recursion is ONE chain of k frames, and N = k + 1.

With gap = 0 every push happens in the same move (cost 3: one agent move, then two more cells to the goal).  With gap >= 1
every level adds its own `distance + 1` = gap, so the cost is 2 + (k - 1) * gap + 1 and every frame adds a non-zero c on the
way back up."""
import glob
import os
import random

import rgd_restatement as R
from oracle import pw_oracle

LADDER_LIMIT = 62  # interior cells per side of the largest board (64 with the border)


def _grid(rows):
    return "\n".join(" ".join(r) for r in rows) + "\n"


def ladder(k, gap=0):
    assert k >= 2 and gap >= 0
    assert k * (1 + gap) + 5 <= LADDER_LIMIT, "ladder(%d, %d) does not fit a 64-wide board" % (k, gap)
    width = (k - 1) * (1 + gap) + 5
    g = [["AW"] * width for _ in range(k - 1)] + [["."] * width]

    def put(x, y, name):
        assert g[y][x] in ("AW", "."), (x, y, g[y][x])  # nothing overlaps: asserted, never clipped
        g[y][x] = name if g[y][x] == "." else "AW+" + name

    put(0, k - 1, "A")
    for i in range(1, k + 1):
        x = 1 + (k - i) * (1 + gap)
        if i == 1:
            put(x, 0, "M1")
            put(x + 3, 0, "G1")
            assert x + 3 == width - 1
        else:
            put(x, i - 2, "M%d" % i)
            put(x, i - 1, "M%d" % i)
    return _grid(g)


def ladder_cost(k, gap):
    """The RGD cost of ladder(k, gap)'s initial state with k - 1 tools (by the construction above)."""
    return 3 + (k - 1) * gap


def room(W, H):
    """An open W x H interior: the agent in the top-left corner, a box beside it and the goal in the bottom-right corner."""
    assert 3 <= W <= LADDER_LIMIT and 3 <= H <= LADDER_LIMIT
    g = [["."] * W for _ in range(H)]
    g[0][0], g[1][1], g[H - 1][W - 1] = "A", "M1", "G1"
    return _grid(g)


def walk(oz, steps, seed, right=0.0):
    """The initial state of `oz` (an OraclePuzzle) and the states of a seeded random walk of `steps` actions; with probability
    `right` a step is a move to the right, else one of the four at random.  Every state is reachable, hence on every graph."""
    rng = random.Random(seed)
    s = oz.initial_state
    out = [s]
    for _ in range(steps):
        a = 1 if rng.random() < right else rng.randrange(4)
        s = oz.get_next_state(s, a)
        out.append(s)
    return out


# the ladders of tests/test_gpu_rgd_deep.py: k = 2, 3 (the two smallest), 16, 17 (both sides of the 4-bit boundary of the packed
# object, pusher and depth fields) and 31 (PW_MAX_OBJECTS = 32 movables, 30 frames), with gap 0 and 1; gap 3 at k = 12.
# ladder(31, 1) would be 65 cells wide and cannot exist: the larger gap-1 cases are k = 20 and k = 28 (29 movables, 27 frames).
LADDERS = [(2, 0), (3, 0), (16, 0), (17, 0), (31, 0), (2, 1), (3, 1), (12, 1), (16, 1), (17, 1), (20, 1), (28, 1), (12, 3)]
# With fewest_tools every depth below k - 1 is tried first, and there nothing is finite, so no bound prunes: with gap >= 1 a
# pusher has two next positions with a finite cost and the calls double per level (4 552 for the initial state of (16, 1),
# 8 810 for (17, 1), 33 909 for (20, 1), more than 300 000 for (28, 1)); on (31, 0) the states after one and after two pushes
# (every piece can then be pushed back to the left as well) take 132 230 calls.  The ladders below get a budget that
# covers them, in the kernel and in the restatement alike; (20, 1) and (28, 1) are evaluated at full depth only.
DEFAULT_CALLS = 4000  # rgd_helpers.MAX_CALLS
FEWEST_CALLS = {(16, 1): 9000, (17, 1): 9000, (31, 0): 140000}
FULL_CALLS = {(28, 1): 5000}  # its initial state takes 4 694 calls at full depth, no other state of its walk more
FULL_DEPTH_ONLY = [(20, 1), (28, 1)]
# never a skipped state (asserted): every gap-0 ladder, and gap 1 up to k = 20; the others stay within SKIP_CAP
NEVER_SKIPPED = [(k, g) for k, g in LADDERS if g == 0 or (g == 1 and k <= 20)]
SKIP_CAP = 0.05
WALK_STEPS, WALK_RIGHT = 60, 0.6
MODES = [(k, g, fewest) for k, g in LADDERS for fewest in (False, True) if not (fewest and (k, g) in FULL_DEPTH_ONLY)]


def max_calls(k, gap, fewest):
    return (FEWEST_CALLS if fewest else FULL_CALLS).get((k, gap), DEFAULT_CALLS)


def ladder_walk(k, gap, steps=WALK_STEPS):
    text = ladder(k, gap)
    oz = pw_oracle.OraclePuzzle(text)
    return text, oz, walk(oz, steps, seed=1000 * k + gap, right=WALK_RIGHT)


_REFERENCE = {}


def ladder_reference(k, gap, fewest):
    """(text, states, costs, calls) of ladder(k, gap): its initial state and a walk, the restatement's cost of every state
    (None where it gave up past max_calls(k, gap, fewest)) and the calls each took.  The walk is shortened until at most
    SKIP_CAP of the states are given up.  Computed once per session and never changed."""
    key = (k, gap, fewest)
    if key not in _REFERENCE:
        for steps in (WALK_STEPS, 45, 30, 15, 0):
            text, oz, states = ladder_walk(k, gap, steps)
            h = R.RecursiveGraphDistance(oz, fewest, max_calls(k, gap, fewest))
            costs, calls = [], []
            for s in states:
                try:
                    costs.append(h.estimate(s))
                except R.GiveUp:
                    costs.append(None)
                calls.append(h.calls)
            if costs.count(None) <= SKIP_CAP * len(costs):
                break
        _REFERENCE[key] = (text, states, costs, calls)
    return _REFERENCE[key]


# ---- the shipped Level-2..4 puzzles ------------------------------------------------------------------------------------
PLAN_STATES, WALK_STATES = 5, 2  # per puzzle, besides the initial state: 8 states in all


def level_paths(level):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return sorted(glob.glob(os.path.join(root, "pushworld_amd", "data", "puzzles", "level%d" % level, "*.pwp")))


def level_states(path, level, oz, seed):
    """The initial state, PLAN_STATES states spread evenly over the shipped plan (its last state but one among them) and
    the states after 3 and 6 steps of a seeded random walk."""
    from rgd_helpers import solution_plan  # (imports torch)

    plan = solution_plan("level%d" % level, os.path.splitext(os.path.basename(path))[0])
    along = [oz.initial_state]
    for a in plan:
        along.append(oz.get_next_state(along[-1], a))
    last = len(along) - 2  # the state before the goal state
    picks = sorted({max(1, round(last * (j + 1) / PLAN_STATES)) for j in range(PLAN_STATES)})
    w = walk(oz, 3 * WALK_STATES, seed)
    return [along[0]] + [along[i] for i in picks] + [w[3 * (j + 1)] for j in range(WALK_STATES)]

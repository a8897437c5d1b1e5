"""Puzzle sets, start states and plans for the plan-replay and cell-grid tests on random shapes (tests/test_replay_shapes_host.py,
test_cells_shapes_host.py, test_gpu_plan_replay_shapes.py, test_gpu_cells_shapes.py).  A helper, not a test.  Built on
tests/shape_states.py: its six CASES and their state lists as they are, plus a THREE-GOAL variant of (5, 30, 1), (8, 16, 2) and
(12, 30, 4) -- the text ``random_puzzle`` returns with two seeded free ``.`` cells turned into ``G1`` and ``G2`` (the Python
object order then is A, M2, M1, M0, the rest in file order).  A puzzle is named by its KEY: the case, or the case + ("g3",).

Sets by padding (SETS): the puzzles of one engine.  Items of a set (``items(npad)``), in this order per puzzle:
  * for every start -- the listed states of the puzzle, then for a three-goal puzzle its constructed starts -- PLANS_PER_START
    seeded plans: a length out of {0, 1, GS - 1, GS, GS + 1, 2 GS, 2 GS + 1, CAP - 1, CAP} (GS the kernel's lane-group width, CAP
    = 37 the plan_cap), every action repeating the one before with probability 0.7.  A plan is cut before the first action that
    takes its oracle trace out of the engine's domain (``in_domain``).  Where the trace first reaches a goal after f >= 1 actions
    the plan cut to f (VALID) and to f + 1 (EARLY) follow it (f = len: the plan with its last action repeated, if that fits);
  * the constructed starts of a three-goal puzzle (a CPU probe showed seeded walks from goal-near states never finishing one):
    FINISH starts -- every goal movable on its goal but one, that one a single cell away and the agent where the oracle's step
    pushes it home -- and OFF_AND_BACK starts with their plans, found by a search of the oracle on the CPU, whose trace pushes
    a goal movable off its goal (-1.01), back onto it (0.99), and ends with 10.0.
Nothing else is dropped.  The seeds were chosen on the CPU so that the conditions of tests/test_replay_shapes_host.py hold.
Plan rows are filled with 0xEE beyond their length: a fetch past ``len`` shows as a wrong verdict."""
from collections import namedtuple

import numpy as np

import shape_states as SS
import walk_restatement as WR
from oracle import c_oracle

CAP = 37
FILL = 0xEE
G3 = ("g3",)
THREE = [SS.CASES[1] + G3, SS.CASES[2] + G3, SS.CASES[3] + G3]
KEYS = list(SS.CASES) + THREE
SETS = {
    4: [SS.CASES[0]],
    8: [SS.CASES[0], SS.CASES[1], SS.CASES[2], THREE[0], THREE[1]],
    16: [SS.CASES[3], THREE[2], SS.CASES[1]],
    32: [SS.CASES[4], SS.CASES[5], SS.CASES[2]],
}
# seeds of the two goal cells of a three-goal variant
GOAL_SEEDS = {THREE[0]: 17, THREE[1]: 8, THREE[2]: 6}
# (near, far, goal_near) counts and seeds of the variants' state lists (the recipe of shape_states.states)
COUNTS3 = (6, 10, 6)
SEEDS3 = {THREE[0]: (1, 2, 3), THREE[1]: (1, 2, 3), THREE[2]: (1, 2, 3)}
FINISH_SEED = 11  # far states the FINISH starts are built from: FINISH_PER_GOAL per goal movable
FINISH_PER_GOAL = 2
PLANS_PER_START = {4: 16, 8: 4, 16: 16, 32: 16}  # (a trace that leaves the grid and returns is one in a hundred on the larger boards)
PLAN_SEED = {4: 1, 8: 1, 16: 2, 32: 1}
# (start, plan) per three-goal puzzle: the oracle trace pushes a goal movable off its goal (-1.01), back onto it (0.99) and ends
# with 10.0.  Found on the CPU: the other goal movables on their goals or one cell away, the agent at a position INTERLOCKED with
# the first movable (a step one way and a step back both displace it), then a breadth-first search of the oracle for the rest of
# the plan; tests/test_replay_shapes_host.py asserts what they do.
OFF_AND_BACK = {
    THREE[0]: [
        (((12, 9), (25, 23), (22, 26), (17, 16), (24, 14)),
         (0, 1, 2, 0, 0, 0, 0, 0, 3, 3, 3, 3, 3, 3, 1, 3, 3, 3, 1, 3, 1, 1, 1, 1, 3, 3, 1)),
        (((22, 19), (25, 23), (23, 26), (18, 16), (24, 14)), (0, 1, 2, 0, 2, 0)),
    ],
    THREE[1]: [
        (((10, 0), (9, 13), (13, 6), (11, 13), (11, 2), (0, 9), (15, 6), (15, 7)), (0, 1, 0, 3, 0, 2, 0, 0, 0, 0, 1)),
        (((9, 1), (9, 13), (13, 6), (11, 13), (11, 2), (0, 9), (15, 6), (15, 7)), (0, 1, 0, 2, 0, 0, 0, 0, 1)),
    ],
    THREE[2]: [
        (((25, 17), (24, 16), (27, 14), (7, 11), (25, 14), (13, 17), (14, 16), (14, 9), (20, 1), (20, 11), (13, 9), (20, 7)),
         (2, 3, 1, 2, 1, 2)),
        (((25, 19), (24, 16), (27, 14), (7, 11), (25, 14), (13, 17), (14, 16), (14, 9), (20, 1), (20, 11), (13, 9), (20, 7)),
         (2, 3, 0, 0, 0, 2, 2, 2, 2, 1, 1, 2, 2, 2, 1, 3, 0, 3, 1, 1, 3, 3, 1, 2)),
    ],
}

Listed = SS.Listed
Item = namedtuple("Item", "pid key start plan kind")  # kind: "drawn", "valid", "early", "finish", "off_and_back"
Trace = namedtuple("Trace", "states rewards terms goals")
_TEXT, _PUZZLE, _STATES, _FINISH, _ITEMS, _TRACES = {}, {}, {}, {}, {}, {}


def gs(npad):
    """The lane-group width of the replay kernel."""
    return 8 if npad <= 8 else npad


def lengths(npad):
    """The plan lengths of a set: those of the length set that the plan_cap admits (2 GS and 2 GS + 1 do not fit for GS = 32)."""
    g = gs(npad)
    return sorted(n for n in {0, 1, g - 1, g, g + 1, 2 * g, 2 * g + 1, CAP - 1, CAP} if n <= CAP)


def is_three(key):
    return key[3:] == G3


def text(key):
    if not is_three(key):
        return SS.text(key)
    if key not in _TEXT:
        rows = [r.split() for r in SS.text(key[:3]).split("\n")]
        free = [(y, x) for y, r in enumerate(rows) for x, c in enumerate(r) if c == "."]
        pick = np.random.default_rng(GOAL_SEEDS[key]).choice(len(free), size=2, replace=False)
        for name, k in zip(("G1", "G2"), pick):
            y, x = free[int(k)]
            rows[y][x] = name
        _TEXT[key] = "\n".join("  ".join(r) for r in rows)
    return _TEXT[key]


def puzzle(key):
    """The key's oracle puzzle, one object per session."""
    if not is_three(key):
        return SS.puzzle(key)
    if key not in _PUZZLE:
        _PUZZLE[key] = c_oracle.COraclePuzzle(text(key))
    return _PUZZLE[key]


def states(key):
    """[Listed(kind, state)]: shape_states.states of a case; the same recipe with COUNTS3 / SEEDS3 for a three-goal variant."""
    if not is_three(key):
        return SS.states(key)
    if key not in _STATES:
        cp = puzzle(key)
        out = [Listed("initial", cp.initial_state)]
        for kind, make, count, seed in zip(("near", "far", "goal_near"), (SS.near_states, SS.far_states, SS.goal_near_states),
                                           COUNTS3, SEEDS3[key]):
            out += [Listed(kind, s) for s in make(cp, np.random.default_rng(seed), count)]
        _STATES[key] = out
    return _STATES[key]


def in_domain(cp, state):
    """The engine's domain (the header of tests/test_gpu_quad16.py): every movable inside the grid, or at most one cell beyond
    it while some cell of it still lies on the grid."""
    for k, ((x, y), (w, h)) in enumerate(zip(state, cp.py.sizes)):
        if x < -1 or y < -1 or x + w > cp.width + 1 or y + h > cp.height + 1:
            return False
        if not any(0 <= x + cx < cp.width and 0 <= y + cy < cp.height for cx, cy in cp.py.shapes[k]):
            return False
    return True


def trace(cp, start, plan):
    """The oracle stepped along `plan`: Trace(states [len + 1], rewards, terminated flags, goal flag of every state)."""
    sts, rewards, terms = [tuple(map(tuple, start))], [], []
    for a in plan:
        nxt, r, term = cp.env_step(sts[-1], a)
        sts.append(nxt)
        rewards.append(r)
        terms.append(term)
    return Trace(sts, rewards, terms, [cp.py.is_goal_state(s) for s in sts])


def item_trace(item):
    """``trace`` of an item, computed once per session and never changed."""
    key = (item.key, item.start, item.plan)
    if key not in _TRACES:
        _TRACES[key] = trace(puzzle(item.key), item.start, item.plan)
    return _TRACES[key]


def leaves_and_returns(cp, states_):
    """True when some state of the trace is outside the grid and a later one inside."""
    inside = [WR.in_grid(cp, s) for s in states_]
    return any(not a and any(inside[i + 1:]) for i, a in enumerate(inside))


def finish_starts(key):
    """[(start, action)] of a puzzle (the items take those of the three-goal puzzles): per goal movable FINISH_PER_GOAL far states with the other goal movables on
    their goals, this one a cell before its goal and the agent at the first position (row-major) from which the oracle's step
    by `action` ends the episode.  A (state, goal movable, action) without such a position gives none."""
    if key not in _FINISH:
        cp = puzzle(key)
        rng = np.random.default_rng(FINISH_SEED)
        out = []
        aw, ah = cp.py.sizes[0]
        for last in range(1, cp.num_goals + 1):
            for far in SS.far_states(cp, rng, FINISH_PER_GOAL):
                first = int(rng.integers(0, 4))
                s = list(far)
                for g, goal in enumerate(cp.py.goal_state):
                    s[1 + g] = tuple(goal)
                found = None
                for k in range(4):
                    a = (first + k) % 4
                    dx, dy = SS.DISPLACEMENTS[a]
                    s[last] = (cp.py.goal_state[last - 1][0] - dx, cp.py.goal_state[last - 1][1] - dy)
                    for y in range(cp.height - ah + 1):
                        for x in range(cp.width - aw + 1):
                            s[0] = (x, y)
                            st = tuple(s)
                            if WR.in_grid(cp, st) and cp.env_step(st, a)[2]:
                                found = (st, a)
                                break
                        if found:
                            break
                    if found:
                        break
                if found:
                    out.append(found)
        _FINISH[key] = out
    return _FINISH[key]


def _draw(rng, length):
    plan = []
    for t in range(length):
        plan.append(plan[-1] if t and rng.random() < 0.7 else int(rng.integers(0, 4)))
    return plan


def _cut(cp, start, plan):
    """`plan` cut before the first action that takes the trace out of the domain."""
    s = tuple(map(tuple, start))
    for t, a in enumerate(plan):
        s = cp.env_step(s, a)[0]
        if not in_domain(cp, s):
            return plan[:t]
    return plan


def _with_goal_cuts(pid, key, start, plan, kind, out):
    cp = puzzle(key)
    plan = tuple(_cut(cp, start, plan))
    out.append(Item(pid, key, start, plan, kind))
    goals = item_trace(out[-1]).goals
    f = goals.index(True) if True in goals else -1
    if f >= 1:
        if f < len(plan):
            out.append(Item(pid, key, start, plan[:f], "valid"))
            out.append(Item(pid, key, start, plan[:f + 1], "early"))
        elif f < CAP:
            longer = plan + plan[-1:]
            if tuple(_cut(cp, start, longer)) == longer:
                out.append(Item(pid, key, start, longer, "early"))


def starts(key):
    """The starts plans are drawn from: the listed states, then the FINISH starts of a three-goal puzzle."""
    out = [s for _, s in states(key)]
    if is_three(key):
        out += [s for s, _ in finish_starts(key)]
    return out


def items(npad):
    """[Item] of the set, computed once."""
    if npad not in _ITEMS:
        out = []
        choices = lengths(npad)
        for pid, key in enumerate(SETS[npad]):
            rng = np.random.default_rng([PLAN_SEED[npad], npad, pid])
            for start in starts(key):
                for _ in range(PLANS_PER_START[npad]):
                    _with_goal_cuts(pid, key, start, _draw(rng, int(rng.choice(choices))), "drawn", out)
            if is_three(key):
                for start, a in finish_starts(key):
                    _with_goal_cuts(pid, key, start, [a, a], "finish", out)
                for start, plan in OFF_AND_BACK.get(key, ()):
                    _with_goal_cuts(pid, key, start, list(plan), "off_and_back", out)
        _ITEMS[npad] = out
    return _ITEMS[npad]


def padded(state, npad):
    row = np.zeros((npad, 2), np.int8)
    row[:len(state)] = np.asarray(state, np.int8)
    return row


def packed(npad, its=None):
    """(puzzle ids int32 [n], starts int8 [n, npad, 2], plans uint8 [n, CAP] filled with FILL beyond the length, lengths int32
    [n]) of the items."""
    its = items(npad) if its is None else its
    ids = np.array([it.pid for it in its], np.int32)
    pos = np.stack([padded(it.start, npad) for it in its])
    plans = np.full((len(its), CAP), FILL, np.uint8)
    for i, it in enumerate(its):
        plans[i, :len(it.plan)] = it.plan
    return ids, pos, plans, np.array([len(it.plan) for it in its], np.int32)

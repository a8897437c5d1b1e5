"""Plain-Python restatement of the cost-to-go table over pushes (``pw_push_search_solve`` / ``pw_push_search_table_*``, DESIGN.md
K18) over ``push_search_restatement.search_store(stop_at_goal=False)`` and ``walk_restatement`` (``region``, ``canon``,
``in_grid``, ``path``).  A helper of tests/test_push_table_host.py and tests/test_gpu_push_table.py, not a test.

State i of the store has the push rows of ``region(states[i])`` in (y, x, action) order.  ``succ`` of a row is the store index
of its successor's canonical state (a dictionary over canonical states), -1 for a successor outside its grid.  The value of a
row is 0 when it is a goal row, else the cost of its successor, else infinite; the cost of a state is 0 at a goal state, else
1 + the least value of its rows, -1 where that is infinite.  Costs are found by level-synchronous sweeps, ``best`` is the lowest
row of the least value, bit 0 / 1 / 2 of ``flags`` are goal / optimal / safe."""
from collections import namedtuple

import push_search_restatement as PR
import walk_restatement as WR

GOAL, OPTIMAL, SAFE = 1, 2, 4
NO_ACTION = 0xFF

Table = namedtuple("Table", "store index row_off succ frm action flags cost best info")
Query = namedtuple("Query", "index cost action push_from push_action walk")
NOT_IN_TABLE = Query(-1, -2, -1, (0, 0), NO_ACTION, -1)


def _key(canon, state):
    return (tuple(canon),) + tuple(tuple(xy) for xy in state[1:])


def build(p, start=None, store=None):
    """``Table`` of the exhausted search from ``start`` (or of ``store``, a ``search_store(stop_at_goal=False)``)."""
    st = PR.search_store(p, start=start, stop_at_goal=False) if store is None else store
    assert st.goal_index == -1 and st.layer_states[-1] == 0
    S = st.num_states
    index = {_key(c, s): i for i, (s, c) in enumerate(zip(st.states, st.canons))}
    assert len(index) == S
    row_off, succ, frm, action, flags = [0], [], [], [], []
    for s in st.states:
        for pm in WR.region(p, s).pushes:
            succ.append(index[WR.canon(p, pm.next_state)] if WR.in_grid(p, pm.next_state) else -1)  # (KeyError: an internal error)
            frm.append(tuple(pm.frm))
            action.append(pm.action)
            flags.append(GOAL if pm.goal else 0)
        row_off.append(len(succ))
    cost = [0 if ln.goal else -1 for ln in st.links]
    best = [-1] * S

    def value(r):  # None: infinite
        if flags[r] & GOAL:
            return 0
        return cost[succ[r]] if succ[r] >= 0 and cost[succ[r]] >= 0 else None

    d = 0
    while True:  # sweep d gives cost d to every unset state with a row of value d - 1
        d += 1
        found = {}
        for i in range(S):
            if cost[i] == -1:
                for k in range(row_off[i + 1] - row_off[i]):
                    if value(row_off[i] + k) == d - 1:
                        found[i] = k
                        break
        if not found:
            break
        for i, k in found.items():
            cost[i], best[i] = d, k
    for i in range(S):
        for r in range(row_off[i], row_off[i + 1]):
            c = value(r)
            if c is not None:
                flags[r] |= SAFE
                if cost[i] > 0 and c == cost[i] - 1:
                    flags[r] |= OPTIMAL
    info = (S, len(succ), sum(c == 0 for c in cost), sum(c == -1 for c in cost), max(cost))  # (largest: -1 when all are dead)
    return Table(st, index, row_off, succ, frm, action, flags, cost, best, info)


def query(p, t, live):
    """The six outputs of the query for the live state ``live``."""
    live = tuple(tuple(xy) for xy in live)
    if not WR.in_grid(p, live):
        return NOT_IN_TABLE
    reg = WR.region(p, live)
    i = t.index.get(_key(reg.canon, live))
    if i is None:
        return NOT_IN_TABLE
    if t.best[i] < 0:
        return Query(i, t.cost[i], -1, (0, 0), NO_ACTION, -1)
    r = t.row_off[i] + t.best[i]
    walk = reg.dist[t.frm[r]]  # (the rows of node i are the rows of every live state that maps to it)
    return Query(i, t.cost[i], WR.path(reg, t.frm[r])[0] if walk else t.action[r], t.frm[r], t.action[r], walk)


def summary(p, t):
    """(states, rows, rows out of grid, of them goal rows, goal states, dead ends, largest cost, cost of the start)"""
    out = [r for r in range(len(t.succ)) if t.succ[r] < 0]
    return (t.info[0], t.info[1], len(out), sum(1 for r in out if t.flags[r] & GOAL), t.info[2], t.info[3], t.info[4], t.cost[0])


# ---- the cases of the table tests: name -> (puzzle text, oracle puzzle, start or None); tables computed once and never changed --
_CASES, _TABLES = {}, {}
# (states, rows, rows out of grid, of them goal rows, goal states, dead ends, largest cost (-1: none), cost of the start (-1: dead))
EXPECT = {
    "big": (1260, 6464, 0, 0, 35, 425, 8, 6),
    "corridor 7": (3, 2, 0, 0, 1, 0, 2, 2),
    "pockets": (3, 2, 0, 0, 1, 0, 2, 2),
    "serpentine 14x14": (3, 2, 0, 0, 1, 0, 2, 2),
    "serpentine 14x13 overshoot": (3, 2, 0, 0, 1, 1, 1, 1),
    "shape (3, 12, 9) deep goal start": (8, 21, 0, 0, 2, 2, 3, 3),
    "shape (8, 16, 2) deep goal start": (6997, 19791, 220, 2, 234, 4569, 36, 3),
    "shape (8, 16, 2) listed 29": (99, 648, 325, 54, 0, 67, 1, 1),
    "shape (8, 16, 2) listed 30": (1601, 9429, 2106, 210, 0, 729, 6, 1),
    "shape (3, 12, 9) search start 3": (261, 878, 24, 0, 0, 261, -1, -1),
}


def _make_cases():
    import deep_puzzles
    import shape_states as SS
    from oracle import c_oracle

    def deep(text):
        return lambda: (text, c_oracle.COraclePuzzle(text), None)

    def shape(case, start):
        return lambda: (SS.text(case), SS.puzzle(case), start() if callable(start) else start)

    a, c = SS.CASES[0], SS.CASES[2]
    _CASES.update({
        "big": deep(deep_puzzles.big()),
        "corridor 7": deep(deep_puzzles.corridor(7)),
        "pockets": deep(deep_puzzles.pockets()),
        "serpentine 14x14": deep(deep_puzzles.serpentine(14, 14)),
        "serpentine 14x13 overshoot": deep(deep_puzzles.serpentine(14, 13, True)),
        "shape (3, 12, 9) deep goal start": shape(a, SS.DEEP_GOAL_STARTS[a][0]),
        "shape (8, 16, 2) deep goal start": shape(c, SS.DEEP_GOAL_STARTS[c][0]),
        "shape (8, 16, 2) listed 29": shape(c, lambda: SS.states(c)[29].state),
        "shape (8, 16, 2) listed 30": shape(c, lambda: SS.states(c)[30].state),
        "shape (3, 12, 9) search start 3": shape(a, SS.SEARCH_STARTS[a][3]),
    })


def case(name):
    """(puzzle text, oracle puzzle, start, ``Table``) of a case of ``EXPECT``."""
    if not _CASES:
        _make_cases()
    if name not in _TABLES:
        text, cp, start = _CASES[name]()
        _TABLES[name] = (text, cp, start, build(cp, start=start))
    return _TABLES[name]

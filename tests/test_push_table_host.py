"""Host side of the cost-to-go tables over pushes (``pw_push_search_solve`` / ``pw_push_search_table_*``): the
restatement of tests/push_table_restatement.py against pinned figures, its equations and its query on a few live states, the
argument checks that return before anything touches a device, the header against ``_capi.SIGNATURES``, and the wrappers' input
checks."""
import ctypes
import os

import pytest

import push_table_restatement as TR
import walk_restatement as WR
from pushworld_amd import _capi
from pushworld_amd.search import PushQuery, PushSolutionTable, _push_query_outputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p(4096)  # a stand-in for a handle or a device array: every check below returns before anything is read through it
NAMES = ("solve", "table_read", "table_rows", "table_query")


@pytest.mark.parametrize("name", list(TR.EXPECT))
def test_restatement_figures(name):
    """(states, rows, rows out of grid, of them goal rows, goal states, dead ends, largest cost, cost of the start)"""
    _, cp, _, t = TR.case(name)
    assert TR.summary(cp, t) == TR.EXPECT[name]


@pytest.mark.parametrize("name", list(TR.EXPECT))
def test_restatement_satisfies_its_equations(name):
    """The sweeps' result against the definitions, row by row: cost, best and the bits."""
    _, cp, _, t = TR.case(name)
    S = t.info[0]
    assert len(t.row_off) == S + 1 and t.row_off[-1] == len(t.succ) == t.info[1]
    for i in range(S):
        vals = []
        for r in range(t.row_off[i], t.row_off[i + 1]):
            c = 0 if t.flags[r] & TR.GOAL else (t.cost[t.succ[r]] if t.succ[r] >= 0 and t.cost[t.succ[r]] >= 0 else None)
            vals.append(c)
            assert bool(t.flags[r] & TR.SAFE) == (c is not None)
            assert bool(t.flags[r] & TR.OPTIMAL) == (t.cost[i] > 0 and c == t.cost[i] - 1)
        finite = [c for c in vals if c is not None]
        if t.store.links[i].goal:
            assert (t.cost[i], t.best[i]) == (0, -1)
        elif not finite:
            assert (t.cost[i], t.best[i]) == (-1, -1)
        else:
            assert t.cost[i] == 1 + min(finite) and t.best[i] == vals.index(min(finite))


def test_no_goal_state_in_the_store_and_cost_one():
    """Listed state 29: every goal row leaves the grid, so no state of the store is a goal state and yet costs of 1 exist."""
    _, cp, _, t = TR.case("shape (8, 16, 2) listed 29")
    assert t.info[2] == 0 and t.info[4] == 1 and t.cost[0] == 1
    goal_rows = [r for r in range(len(t.succ)) if t.flags[r] & TR.GOAL]
    assert goal_rows and all(t.succ[r] == -1 for r in goal_rows)


def test_restatement_query():
    _, cp, _, t = TR.case("big")
    st = t.store
    # the start: its own node, six pushes to go, the action is the first of the walk to the best push (or the push)
    q = TR.query(cp, t, st.states[0])
    assert (q.index, q.cost) == (0, 6) and q.action in (0, 1, 2, 3)
    r = t.row_off[0] + t.best[0]
    assert (q.push_from, q.push_action) == (t.frm[r], t.action[r]) and q.walk == WR.region(cp, st.states[0]).dist[t.frm[r]]
    # another agent position of the same walk region: the same node, cost and push, another walk
    reg = WR.region(cp, st.states[0])
    far = max(reg.dist, key=lambda xy: reg.dist[xy])
    q2 = TR.query(cp, t, (far,) + tuple(st.states[0][1:]))
    assert (q2.index, q2.cost, q2.push_from, q2.push_action) == (0, 6, q.push_from, q.push_action)
    # following the actions from the start reaches a goal state with exactly six pushing steps
    state, pushes = tuple(st.states[0]), 0
    for _ in range(6 * 36):
        q = TR.query(cp, t, state)
        if q.cost == 0:
            break
        nxt, moved = cp.get_next_state_moved(state, q.action)
        pushes += len(moved) > 1
        state = tuple(tuple(xy) for xy in nxt)
    assert q.cost == 0 and pushes == 6 and cp.py.is_goal_state(state)
    # a goal state, a dead end, a movable outside its grid
    g = next(i for i in range(t.info[0]) if t.cost[i] == 0)
    assert TR.query(cp, t, st.states[g]) == TR.Query(g, 0, -1, (0, 0), 0xFF, -1)
    d = next(i for i in range(t.info[0]) if t.cost[i] == -1)
    assert TR.query(cp, t, st.states[d]) == TR.Query(d, -1, -1, (0, 0), 0xFF, -1)
    assert TR.query(cp, t, ((0, 0), (9, 2), (3, 3))) == TR.NOT_IN_TABLE


# ---- the C ABI: checks that return before any launch -----------------------------------------------------------------------------
def test_null_handle_and_null_info():
    lib = _capi.lib
    info = (ctypes.c_int64 * 5)()
    for name, call in (("pw_push_search_solve", lambda: lib.pw_push_search_solve(None, info, None)),
                       ("pw_push_search_table_read", lambda: lib.pw_push_search_table_read(None, 0, 1, P, P, P, None)),
                       ("pw_push_search_table_rows", lambda: lib.pw_push_search_table_rows(None, 0, 1, P, P, P, P, None)),
                       ("pw_push_search_table_query", lambda: lib.pw_push_search_table_query(None, None, P, 4, None, 1, P, P, P, P, P, P, None))):
        assert call() == _capi.PW_EINVAL
        msg = _capi.last_error()
        assert name in msg and "null search" in msg
    assert lib.pw_push_search_solve(P, None, None) == _capi.PW_EINVAL
    assert "pw_push_search_solve" in _capi.last_error() and "null info" in _capi.last_error()


@pytest.mark.parametrize("args, words", [
    ((None, P, 4, None, 0), "n must be >= 1"),
    ((None, P, 4, None, -3), "n must be >= 1"),
    ((None, None, 4, None, 1), "null pos"),
    ((None, P, 0, None, 1), "npad must be 4, 8, 16 or 32"),
    ((None, P, 6, None, 1), "npad must be 4, 8, 16 or 32"),
    ((None, P, 64, None, 1), "npad must be 4, 8, 16 or 32"),
])
def test_query_argument_checks(args, words):
    assert _capi.lib.pw_push_search_table_query(P, *args, P, P, P, P, P, P, None) == _capi.PW_EINVAL
    msg = _capi.last_error()
    assert "pw_push_search_table_query" in msg and words in msg


def test_read_argument_checks():
    lib = _capi.lib
    for first, count in ((-1, 1), (0, -1)):
        assert lib.pw_push_search_table_read(P, first, count, P, P, P, None) == _capi.PW_EINVAL
        assert "pw_push_search_table_read" in _capi.last_error() and "out of bounds" in _capi.last_error()
        assert lib.pw_push_search_table_rows(P, first, count, P, P, P, P, None) == _capi.PW_EINVAL
        assert "pw_push_search_table_rows" in _capi.last_error() and "out of bounds" in _capi.last_error()


def test_header_and_signatures():
    with open(os.path.join(ROOT, "include", "pushworld_amd.h")) as f:
        header = f.read()
    counts = {"solve": 3, "table_read": 7, "table_rows": 8, "table_query": 13}
    for name in NAMES:
        full = f"pw_push_search_{name}"
        assert f"int  {full}(" in header and full in _capi.SIGNATURES
        restype, argtypes = _capi.SIGNATURES[full]
        decl = header[header.index(f"int  {full}("):]
        decl = decl[:decl.index(");")]
        assert restype is ctypes.c_int and len(argtypes) == counts[name] == decl.count(",") + 1
        assert getattr(_capi.lib, full) is not None
    for words in ("16 bytes per state", "8 bytes per row", "ONE query at a time per handle", "not a count of moves"):
        assert words in header
    with open(os.path.join(ROOT, "pushworld_amd", "csrc", "pw_kernels.hip")) as f:
        unit = f.read()
    assert unit.index('#include "pw_push_search.inc"') < unit.index('#include "pw_push_table.inc"')


# ---- the wrappers ------------------------------------------------------------------------------------------------------------------
def test_wrapper_arguments():
    class NoEngine:  # the checks of the search's constructor come before an engine is asked for
        num_movables = 2

        def _engine(self):
            raise AssertionError("an engine was asked for")

    for bad in (0, -1, 1 << 31):
        with pytest.raises(ValueError, match="max_states"):
            PushSolutionTable(NoEngine(), max_states=bad)
    with pytest.raises(ValueError, match="chunk"):
        PushSolutionTable(NoEngine(), chunk=0)
    with pytest.raises(AssertionError, match="an engine was asked for"):
        PushSolutionTable(NoEngine())
    tab = PushSolutionTable.__new__(PushSolutionTable)
    tab.search = None
    for call in (tab.states, tab.offsets, tab.costs, tab.best, tab.rows):
        with pytest.raises(ValueError, match="closed"):
            call(0, 1)
    tab.close()
    q = PushQuery(1, 2, 3, 4, 5, 6)
    assert (q.index, q.cost, q.action, q.push_from, q.push_action, q.walk) == (1, 2, 3, 4, 5, 6) and len(q) == 6
    for bad in ((1, 2, 3), [None] * 5, "x"):
        with pytest.raises(ValueError, match="PushQuery of an earlier query"):
            _push_query_outputs(bad, 4, None)

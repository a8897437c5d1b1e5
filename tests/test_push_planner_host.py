"""Host side of the best-first search over pushes (``pw_push_planner_*``): the argument checks that return
before anything touches a device, the wrapper's input checks, the header and ``SIGNATURES``, the ``run_planner`` flags, and the
restatement (tests/push_planner_restatement.py) against the counts pinned in the issue that asked for the search.

One pinned figure differs from that issue's table: the largest region of `Simple Tool` is 53, not 54.  The sketch behind the
table also counted the region of the goal row's successor (54 positions, the last state of the store); the semantics say that
nothing is pushed in the round that meets the goal and that the largest region takes the maximum over the states pushed, and
the text wins."""
import ctypes
import os

import pytest

import push_planner_restatement as PP
import walk_restatement as WR
from oracle import c_oracle, pw_oracle
from pushworld_amd import _capi, run_planner
from pushworld_amd.search import PushBestFirstSearch, PushPlannerInfo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "pushworld_amd", "data")
P = ctypes.c_void_p(4096)  # a stand-in for an engine: every check below returns before anything is read through it

# (puzzle, K): status, rounds, expanded, states, open, push rows, pushes on the plan, largest region, largest key
PINNED = {
    ("Single Obstacle", 1): ("solved", 4, 4, 8, 3, 8, 3, 30, 4),
    ("Single Obstacle", 8): ("solved", 3, 8, 9, 0, 12, 3, 30, 4),
    ("Two Goals", 1): ("solved", 4, 4, 17, 12, 36, 4, 68, 15),
    ("Two Goals", 8): ("solved", 4, 23, 45, 21, 208, 4, 68, 17),
    ("Two Goals", 64): ("solved", 4, 51, 52, 0, 434, 4, 68, 17),
    ("2 Obstacle", 1): ("solved", 42, 42, 97, 53, 613, 17, 82, 11),
    ("2 Obstacle", 8): ("solved", 11, 78, 139, 59, 1231, 11, 82, 14),
    ("2 Obstacle", 64): ("solved", 11, 395, 397, 0, 6394, 11, 86, 17),
    ("Simple Tool", 1): ("solved", 50, 50, 201, 150, 551, 12, 53, 17),
    ("Simple Tool", 8): ("solved", 9, 65, 245, 179, 668, 9, 53, 15),
    ("Walk Past", 1): ("solved", 7, 7, 67, 54, 76, 7, 46, 12),
    ("Walk Past", 8): ("solved", 7, 49, 446, 390, 640, 7, 46, 14),
}

_PUZZLES, _RUNS = {}, {}


def level1(name):
    with open(os.path.join(DATA, "puzzles", "level1", name + ".pwp")) as f:
        return f.read()


def oracles(key, text):
    """(C oracle puzzle, Python oracle puzzle with its collision tables) of ``text``: made once per session."""
    if key not in _PUZZLES:
        _PUZZLES[key] = (c_oracle.COraclePuzzle(text), pw_oracle.OraclePuzzle(text))
    return _PUZZLES[key]


def restated(name, k, max_states=1 << 20):
    """The restatement of a Level-1 puzzle run to its end: computed once per session and never changed."""
    key = (name, k, max_states)
    if key not in _RUNS:
        cp, oz = oracles(name, level1(name))
        ref = PP.PushPlannerRestatement(cp, oz, batch=k, max_states=max_states)
        ref.begin()
        ref.run()
        _RUNS[key] = ref
    return _RUNS[key]


def check_store_invariants(cp, ref):
    keys = [(tuple(c),) + tuple(s[1:]) for s, c in zip(ref.states, ref.canons)]
    assert len(set(keys)) == len(keys)  # no two states of a store share a canonical state
    assert ref.links[0].parent == -1 and all(0 <= ln.parent < k for k, ln in enumerate(ref.links) if k)
    assert len(ref.states) == len(ref.canons) == len(ref.links)
    if ref.status == "solved":
        plan, pushes = ref.plan()
        state = ref.states[0]
        for a in plan:
            state = cp.get_next_state(state, a)
        assert cp.py.is_goal_state(state) and tuple(state) == tuple(ref.states[ref.goal_index])
        assert ref.goal_index == len(ref.states) - 1
        assert ref.links[-1].goal and not any(ln.goal for ln in ref.links[:-1])
        return pushes
    return None


def test_abi_version_unchanged():
    assert _capi.lib.pw_abi_version() == _capi.ABI_VERSION == 4


def test_create_argument_checks():
    out = ctypes.c_void_p()
    lib = _capi.lib
    for args, words in (((None, 0, 16, 1, 0, ctypes.byref(out)), "null engine"),
                        ((P, 0, 16, 1, 0, None), "null out"),
                        ((P, 0, 0, 1, 0, ctypes.byref(out)), "max_states"),
                        ((P, 0, -5, 1, 0, ctypes.byref(out)), "max_states"),
                        ((P, 0, 1 << 31, 1, 0, ctypes.byref(out)), "max_states"),
                        ((P, 0, 1 << 40, 1, 0, ctypes.byref(out)), "max_states"),
                        ((P, 0, 16, 0, 0, ctypes.byref(out)), "batch"),
                        ((P, 0, 16, -1, 0, ctypes.byref(out)), "batch"),
                        ((P, 0, 16, 65537, 0, ctypes.byref(out)), "batch"),
                        ((P, 0, 16, 1, -1, ctypes.byref(out)), "rgd_budget")):
        assert lib.pw_push_planner_create(*args) == _capi.PW_EINVAL
        msg = _capi.last_error()
        assert "pw_push_planner_create" in msg and words in msg
        assert not out.value


def test_null_handle():
    lib = _capi.lib
    info = (ctypes.c_int64 * 10)()
    buf = (ctypes.c_uint8 * 8)()
    lib.pw_push_planner_destroy(None)  # as free(NULL)
    for name, call in (("pw_push_planner_begin", lambda: lib.pw_push_planner_begin(None, None, None)),
                       ("pw_push_planner_run", lambda: lib.pw_push_planner_run(None, 0, info, None)),
                       ("pw_push_planner_read_states", lambda: lib.pw_push_planner_read_states(None, 0, 1, P, P, None)),
                       ("pw_push_planner_read_links", lambda: lib.pw_push_planner_read_links(None, 0, 1, P, P, P, P, P, None)),
                       ("pw_push_planner_plan", lambda: lib.pw_push_planner_plan(None, buf, 8, None, None))):
        assert call() == _capi.PW_EINVAL
        msg = _capi.last_error()
        assert name in msg and "null planner" in msg


def test_header_and_signatures():
    with open(os.path.join(ROOT, "include", "pushworld_amd.h")) as f:
        header = f.read()
    assert "typedef struct PwPushPlanner PwPushPlanner;" in header
    for name in ("create", "destroy", "begin", "run", "read_states", "read_links", "plan"):
        assert f"pw_push_planner_{name}(" in header and f"pw_push_planner_{name}" in _capi.SIGNATURES
        assert hasattr(_capi.lib, f"pw_push_planner_{name}")


def test_wrapper_arguments():
    class NoEngine:  # the checks of the constructor come before an engine is asked for
        num_movables = 2

        def _engine(self):
            raise AssertionError("an engine was asked for")

    for bad in (0, -1, 1 << 31, 1 << 40):
        with pytest.raises(ValueError, match="max_states"):
            PushBestFirstSearch(NoEngine(), max_states=bad)
    for bad in (0, -7, 65537):
        with pytest.raises(ValueError, match="batch"):
            PushBestFirstSearch(NoEngine(), batch=bad)
    for bad in (0, -3):
        with pytest.raises(ValueError, match="rgd_budget"):
            PushBestFirstSearch(NoEngine(), rgd_budget=bad)
    with pytest.raises(AssertionError, match="an engine was asked for"):  # good arguments do reach the engine
        PushBestFirstSearch(NoEngine(), batch=65536, max_states=(1 << 31) - 1, rgd_budget=1)
    bfs = PushBestFirstSearch.__new__(PushBestFirstSearch)
    bfs._handle, bfs._begun, bfs.num_objects, bfs.info = None, False, 2, None
    bfs.puzzle = type("P", (), {"initial_state": ((1, 1), (2, 2))})()
    for bad in (((1, 1),), ((1, 1), (2, 2), (3, 3)), ((1, 1), (2,)), ((1, 1), (2, 2, 2)), ()):
        with pytest.raises(ValueError, match="one .x, y. pair per movable"):
            bfs.begin(bad)
    with pytest.raises(ValueError, match="closed"):  # a well-formed start gets as far as the handle
        bfs.begin(((1, 1), (2, 2)))
    with pytest.raises(ValueError, match="begin"):
        bfs.run()
    for bad in (0, -2):
        with pytest.raises(ValueError, match="max_rounds"):
            bfs.run(bad)
    assert bfs.plan() is None
    bfs.close()
    info = PushPlannerInfo((1, 2, 3, 4, 5, 6, 7, 8, 9, 10))
    assert info.status == "solved"
    assert (info.rounds, info.expanded, info.states, info.open, info.goal_index, info.rgd_exceeded, info.push_rows,
            info.largest_region, info.largest_key) == (2, 3, 4, 5, 6, 7, 8, 9, 10)


def test_run_planner_flags(capsys):
    assert run_planner.main(["--best-first", "RGD", "missing.pwp"]) == 1  # --best-first without --pushes
    assert "--best-first needs --pushes" in capsys.readouterr().err
    assert run_planner.main(["--best-first", "missing.pwp"]) == 1
    assert "--best-first needs --pushes" in capsys.readouterr().err
    assert run_planner.main(["--pushes", "--best-first", os.path.join(ROOT, "no such puzzle.pwp")]) == 1  # reaches the parser
    assert "ERROR" in capsys.readouterr().err
    assert "--pushes --best-first <puzzle> [--batch K] [--max-states M]" in run_planner.USAGE
    assert run_planner.main(["--pushes", "--best-first"]) == 0 and "--best-first" in capsys.readouterr().out


@pytest.mark.parametrize("name, k", list(PINNED))
def test_restatement_pinned(name, k):
    ref = restated(name, k)
    cp, _ = oracles(name, level1(name))
    pushes = check_store_invariants(cp, ref)
    i = ref.info()
    assert (i.status, i.rounds, i.expanded, i.states, i.open, i.push_rows, pushes, i.largest_region, i.largest_key) == PINNED[name, k]
    assert i.goal_index == i.states - 1 and i.rgd_exceeded == 0
    assert i.largest_region == max(len(WR.region(cp, s).dist) for s in ref.states[:-1])


def test_restatement_max_states():
    ref = restated("2 Obstacle", 1, 97)  # (the solved store has 97 states, but the 33rd round's rows could overflow it)
    cp, _ = oracles("2 Obstacle", level1("2 Obstacle"))
    i = ref.info()
    assert (i.status, i.rounds, i.expanded, i.states, i.open, i.push_rows, i.goal_index) == ("limit", 33, 33, 73, 40, 475, -1)
    assert ref.plan() is None and ref.run() == i  # at its end a run changes nothing
    check_store_invariants(cp, ref)
    full = restated("2 Obstacle", 1)
    assert ref.states == full.states[:73] and ref.links == full.links[:73]
    ref = restated("2 Obstacle", 1, 138)
    i, j = ref.info(), full.info()
    assert i == j and i.status == "solved" and ref.states == full.states and ref.plan() == full.plan()


def test_restatement_steps_and_edges():
    cp, oz = oracles("2 Obstacle", level1("2 Obstacle"))
    full = restated("2 Obstacle", 8)
    ref = PP.PushPlannerRestatement(cp, oz, batch=8, graphs=full.rgd.graphs)
    ref.begin()
    i = ref.run(5)
    assert (i.status, i.rounds, i.goal_index) == ("running", 5, -1) and i.states == i.open + i.expanded
    while ref.status == "running":
        ref.run(1)
    assert ref.info() == full.info() and ref.states == full.states and ref.links == full.links
    # a goal start: solved at once, nothing pushed
    ref.begin(full.states[full.goal_index])
    assert ref.run() == PP.Info("solved", 0, 0, 1, 0, 0, 0, 0, 0, -1) and ref.plan() == ([], 0)
    with pytest.raises(ValueError, match="outside the grid"):
        ref.begin(((-1, 0),) + tuple(cp.initial_state[1:]))
    # a budget of one call: all but a few keys are NaN (a state whose costs need one call each keeps a finite key), and those
    # pop newest-first
    cp, oz = oracles("Two Goals", level1("Two Goals"))
    ref = PP.PushPlannerRestatement(cp, oz, batch=8, rgd_budget=1, graphs=restated("Two Goals", 8).rgd.graphs)
    ref.begin()
    i = ref.run(3)
    assert (i.states, i.rgd_exceeded, i.largest_key) == (43, 38, 4) and (2, 0) in ref.buckets

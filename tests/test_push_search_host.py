"""Host side of the breadth-first search over pushes (``pw_push_search_*``): the argument checks that return
before anything touches a device, the new engine option's name, the wrapper's input checks, and the store restatement
(tests/push_search_restatement.py) against ``walk_restatement.push_search``."""
import ctypes
import os
import zipfile

import pytest

import push_search_restatement as PR
import walk_restatement as WR
from oracle import c_oracle
from pushworld_amd import _capi
from pushworld_amd.search import PushBreadthFirstSearch, PushLayerInfo
from test_walk_host import HAND

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "pushworld_amd", "data")
P = ctypes.c_void_p(4096)  # a stand-in for an engine: every check below returns before anything is read through it


def _level1(name):
    with open(os.path.join(DATA, "puzzles", "level1", name + ".pwp")) as f:
        return f.read()


def _level0(member):
    with zipfile.ZipFile(os.path.join(DATA, "puzzles", "level0.zip")) as z:
        return z.read(member).decode()


CASES = {
    "Single Obstacle": (lambda: _level1("Single Obstacle"), 11),
    "Two Goals": (lambda: _level1("Two Goals"), 60),
    "2 Obstacle": (lambda: _level1("2 Obstacle"), 416),
    "level_0_walls_train_1732": (lambda: _level0("level0/walls/train/level_0_walls_train_1732.pwp"), None),
}


def test_abi_version_unchanged():
    assert _capi.lib.pw_abi_version() == _capi.ABI_VERSION == 4


def test_create_argument_checks():
    out = ctypes.c_void_p()
    lib = _capi.lib
    for args, words in (((None, 0, 16, ctypes.byref(out)), "null engine"),
                        ((P, 0, 16, None), "null out"),
                        ((P, 0, 0, ctypes.byref(out)), "max_states"),
                        ((P, 0, -5, ctypes.byref(out)), "max_states"),
                        ((P, 0, 1 << 31, ctypes.byref(out)), "max_states"),
                        ((P, 0, 1 << 40, ctypes.byref(out)), "max_states")):
        assert lib.pw_push_search_create(*args) == _capi.PW_EINVAL
        msg = _capi.last_error()
        assert "pw_push_search_create" in msg and words in msg
        assert not out.value


def test_null_handle():
    lib = _capi.lib
    info = (ctypes.c_int64 * 6)()
    buf = (ctypes.c_uint8 * 8)()
    lib.pw_push_search_destroy(None)  # as free(NULL)
    for name, call in (("pw_push_search_begin", lambda: lib.pw_push_search_begin(None, None, 1, None)),
                       ("pw_push_search_expand", lambda: lib.pw_push_search_expand(None, info, None)),
                       ("pw_push_search_read_states", lambda: lib.pw_push_search_read_states(None, 0, 1, P, P, None)),
                       ("pw_push_search_read_links", lambda: lib.pw_push_search_read_links(None, 0, 1, P, P, P, P, P, None)),
                       ("pw_push_search_plan", lambda: lib.pw_push_search_plan(None, 0, buf, 8, None, None))):
        assert call() == _capi.PW_EINVAL
        msg = _capi.last_error()
        assert name in msg and "null search" in msg


def test_fingerprint_bits_outside_0_to_32():
    for bad in (-1, 33, 64, 1 << 40):  # (refused before the engine is touched)
        assert _capi.lib.pw_engine_set_option(P, 52, bad) == _capi.PW_EINVAL
        assert "PW_OPT_PUSH_SEARCH_FP_BITS" in _capi.last_error()
    assert _capi.lib.pw_engine_set_option(None, 52, 8) == _capi.PW_EINVAL


def test_option_is_listed():
    assert _capi.OPTIONS["push_search_fp_bits"] == 52
    assert list(_capi.OPTIONS.values()).count(52) == 1
    with open(os.path.join(ROOT, "include", "pushworld_amd.h")) as f:
        header = f.read()
    assert "#define PW_OPT_PUSH_SEARCH_FP_BITS 52" in header
    for name in ("create", "destroy", "begin", "expand", "read_states", "read_links", "plan"):
        assert f"pw_push_search_{name}(" in header and f"pw_push_search_{name}" in _capi.SIGNATURES


def test_wrapper_arguments():
    class NoEngine:  # the checks of the constructor come before an engine is asked for
        num_movables = 2

        def _engine(self):
            raise AssertionError("an engine was asked for")

    for bad in (0, -1, 1 << 31, 1 << 40):
        with pytest.raises(ValueError, match="max_states"):
            PushBreadthFirstSearch(NoEngine(), max_states=bad)
    for bad in (0, -7):
        with pytest.raises(ValueError, match="chunk"):
            PushBreadthFirstSearch(NoEngine(), chunk=bad)
    with pytest.raises(AssertionError, match="an engine was asked for"):  # good arguments do reach the engine
        PushBreadthFirstSearch(NoEngine(), max_states=(1 << 31) - 1, chunk=1)
    # the shape of `start` is checked before anything else of begin(): an object without a handle shows it
    bfs = PushBreadthFirstSearch.__new__(PushBreadthFirstSearch)
    bfs._handle, bfs._begun, bfs.num_objects = None, False, 2
    bfs.puzzle = type("P", (), {"initial_state": ((1, 1), (2, 2))})()
    for bad in (((1, 1),), ((1, 1), (2, 2), (3, 3)), ((1, 1), (2,)), ((1, 1), (2, 2, 2)), ()):
        with pytest.raises(ValueError, match="one .x, y. pair per movable"):
            bfs.begin(bad)
    with pytest.raises(ValueError, match="closed"):  # a well-formed start gets as far as the handle
        bfs.begin(((1, 1), (2, 2)))
    with pytest.raises(ValueError, match="closed"):
        bfs.begin()
    for call in (bfs.expand, lambda: bfs.plan(0)):
        with pytest.raises(ValueError, match="begin"):
            call()
    bfs.close()
    info = PushLayerInfo((3, 5, 40, -1, 17, 9))
    assert (info.depth, info.new_states, info.total_states, info.goal_index, info.push_rows, info.largest_region) == (3, 5, 40, -1, 17, 9)


@pytest.mark.parametrize("name", list(CASES))
def test_store_restatement_agrees_with_push_search(name):
    make, pinned = CASES[name]
    cp = c_oracle.COraclePuzzle(make())
    want = WR.push_search(cp)
    st = PR.search_store(cp)
    assert (st.layer_states, st.num_states, st.pushes) == (want.layer_states, want.num_states, want.pushes)
    assert (st.push_rows, st.largest_region) == (want.push_rows, want.largest_region)
    assert pinned is None or st.num_states == pinned
    assert st.goal_index == st.num_states - 1 and len(st.states) == len(st.canons) == len(st.links) == st.num_states
    assert PR.plan_of(cp, st, st.goal_index) == want.plan
    assert sum(n for _, n in st.layers) == st.num_states
    # the links: the parent of a state lies in the layer before it, no two states share a canonical state
    depth = {}
    for d, (first, n) in enumerate(st.layers):
        for k in range(first, first + n):
            depth[k] = d
    assert all(depth[ln.parent] == depth[k] - 1 for k, ln in enumerate(st.links) if k)
    keys = [(tuple(c),) + tuple(s[1:]) for s, c in zip(st.states, st.canons)]
    assert len(set(keys)) == len(keys)
    assert st.links[-1].goal and not any(ln.goal for ln in st.links[:-1])
    assert PR.search_store(cp, max_pushes=want.pushes - 1).goal_index == -1


def test_store_restatement_exhausts_and_edges():
    cp = c_oracle.COraclePuzzle(CASES["level_0_walls_train_1732"][0]())
    want = WR.push_search(cp, stop_at_goal=False)
    st = PR.search_store(cp, stop_at_goal=False)
    assert (st.layer_states, st.num_states, st.pushes, st.goal_index) == (want.layer_states, 380, None, -1)
    assert (st.push_rows, st.largest_region) == (want.push_rows, want.largest_region)
    assert sum(st.layer_states) + 1 == st.num_states and any(ln.goal for ln in st.links)
    # a goal start; the hand-made board's plan of one push
    cp = c_oracle.COraclePuzzle(HAND)
    m0 = cp.py.names.index("m0")
    solved = tuple((4, 2) if k == m0 else xy for k, xy in enumerate(cp.initial_state))
    st = PR.search_store(cp, start=solved)
    assert (st.num_states, st.goal_index, st.pushes, st.layer_states) == (1, 0, 0, [])
    st = PR.search_store(cp)
    assert (st.num_states, st.goal_index, st.pushes, st.layer_states) == (3, 2, 1, []) and PR.plan_of(cp, st, 2) == [1]
    # exhausted without a goal
    cp = c_oracle.COraclePuzzle("G0 . A . M0 . .\n")
    want = WR.push_search(cp)
    st = PR.search_store(cp)
    assert (st.layer_states, st.num_states, st.goal_index, st.push_rows) == (want.layer_states, want.num_states, -1, want.push_rows)

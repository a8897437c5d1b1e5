"""Best-first search over pushes on the device (pw_push_planner_*, search.PushBestFirstSearch) against the
plain-Python restatement of its semantics (tests/push_planner_restatement.py) over the C oracle's step function and the RGD
restatement: the ten info words, pos / canon / every link field of every state in store order, and the plan."""
import ctypes
import os

import numpy as np
import pytest

import deep_puzzles
import push_planner_restatement as PP
import rgd_puzzles
import shape_states as SS
from oracle import c_oracle, pw_oracle
from pushworld_amd import _capi, run_planner
from pushworld_amd.puzzle import PushWorldPuzzle
from pushworld_amd.search import PLAN_STATUS, PushBestFirstSearch, PushBreadthFirstSearch, SetPuzzle
from pushworld_amd.vec_env import VecPushWorld
from test_push_planner_host import DATA, PINNED, level1, oracles, restated
from test_walk_host import HAND

pytestmark = pytest.mark.gpu

SEALED = "A W M0 . G0\n"  # the agent sealed in one cell: a region of one position, no push (as tests/test_gpu_walk.py)
AWAY = "G0 . A . M0 . .\n"  # the box can only be pushed away from its goal
STATUS = {v: k for k, v in PLAN_STATUS.items()}


def _info_words(i):
    return (STATUS[i.status],) + tuple(i[1:])


def _store_arrays(bfs):
    pos, canon = bfs.states()
    parent, frm, action, walk, goal = bfs.links()
    return tuple(t.cpu().numpy() for t in (pos, canon, parent, frm, action, walk, goal))


def _check(bfs, cp, ref, npad=None):
    """The ten info words, every field of every state and the plan of ``bfs`` (after a run) against the restatement's."""
    want = ref.info()
    print(tuple(bfs.info), _info_words(want))
    assert tuple(bfs.info) == _info_words(want) and bfs.info.status == want.status
    pos, canon, parent, frm, action, walk, goal = _store_arrays(bfs)
    n, N = want.states, cp.num_movables
    assert pos.shape == (n, int(bfs._engine.np) if npad is None else npad, 2) and pos.dtype == np.int8
    assert (pos[:, :N] == np.asarray(ref.states, np.int8)).all() and (pos[:, N:] == 0).all()
    assert (canon == np.asarray(ref.canons, np.int8)).all()
    assert parent.tolist() == [ln.parent for ln in ref.links]
    assert [tuple(q) for q in frm.tolist()] == [tuple(ln.frm) for ln in ref.links]
    assert action.tolist() == [ln.action for ln in ref.links]
    assert walk.tolist() == [ln.walk for ln in ref.links]
    assert goal.tolist() == [int(ln.goal) for ln in ref.links]
    plan = bfs.plan()
    if want.status == "solved":
        assert (plan, bfs.pushes) == ref.plan()
    else:
        assert plan is None
    return plan


def _reaches_goal(bfs, plan, start=None):
    """The plan through pw_plan_states: its last state is a goal state."""
    first = None if start is None else np.ascontiguousarray(np.asarray(start, np.int8))
    states, goals = bfs._engine.plan_states(bfs.puzzle_index, bytes(plan), start=first)
    return bool(goals[-1]) and len(states) == len(plan) + 1


def _restate(cp, oz, k, start=None, max_rounds=None, graphs=None, **kw):
    ref = PP.PushPlannerRestatement(cp, oz, batch=k, graphs=graphs, **kw)
    ref.begin(start)
    ref.run(max_rounds)
    return ref


# ---- 1. the pinned rows -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, k", list(PINNED))
def test_pinned_rows(name, k):
    ref = restated(name, k)
    cp, _ = oracles(name, level1(name))
    with PushBestFirstSearch(PushWorldPuzzle(text=level1(name)), batch=k) as bfs:
        bfs.begin()
        info = bfs.run()
        plan = _check(bfs, cp, ref)
        assert (info.status, info.rounds, info.expanded, info.states, info.open, info.push_rows, bfs.pushes,
                info.largest_region, info.largest_key) == PINNED[name, k]
        assert info.goal_index == info.states - 1 and _reaches_goal(bfs, plan)
        assert bfs.solve() == plan  # at its end a run changes nothing


# ---- 2. rounds one by one, fingerprint bits, padded sets ------------------------------------------------------------------------
def test_rounds_one_by_one_and_capped():
    name, k = "2 Obstacle", 8
    full = restated(name, k)
    cp, oz = oracles(name, level1(name))
    with PushBestFirstSearch(PushWorldPuzzle(text=level1(name)), batch=k) as bfs:
        bfs.begin()
        info = bfs.run(max_rounds=5)
        assert info.status == "running" and info.rounds == 5 and bfs.plan() is None
        _check(bfs, cp, _restate(cp, oz, k, max_rounds=5, graphs=full.rgd.graphs))
        bfs.begin()
        rounds = 0
        while bfs.run(1).status == "running":
            rounds += 1
            assert bfs.info.rounds == rounds
        assert rounds + 1 == full.rounds
        _check(bfs, cp, full)


@pytest.mark.parametrize("bits", [1, 2, 32])
def test_fingerprint_bits(bits):
    name, k = "2 Obstacle", 8
    cp, _ = oracles(name, level1(name))
    pz = PushWorldPuzzle(text=level1(name))
    eng = pz._engine()
    eng.set_option("push_search_fp_bits", bits)
    try:
        with PushBestFirstSearch(pz, batch=k) as bfs:
            bfs.begin()
            bfs.run()
            _check(bfs, cp, restated(name, k))
    finally:
        eng.set_option("push_search_fp_bits", 0)


@pytest.mark.parametrize("npad, index, tables", [(4, 0, "all"), (4, 0, "big"), (4, 0, "none"), (8, 1, "all"), (16, 1, "big"),
                                                 (32, 2, "none"), (32, 0, "all")])
def test_padded_sets_and_step_tables(npad, index, tables):
    """`2 Obstacle` as puzzle `index` of a set padded to `npad` by puzzles with more movables, under the three step_tables forms."""
    name, k = "2 Obstacle", 8
    cp, _ = oracles(name, level1(name))
    extra = {4: None, 8: 4, 16: 10, 32: deep_puzzles.POCKETS_EXTRA}[npad]
    texts = [deep_puzzles.pockets(extra)] * max(index, 1) if extra else []
    texts.insert(index, level1(name))
    vec = VecPushWorld([PushWorldPuzzle(text=t) for t in texts], len(texts), observation=None, max_steps=None,
                       engine_options={"step_tables": tables})
    assert vec.num_objects_padded == npad and cp.num_movables <= 4
    with PushBestFirstSearch(SetPuzzle(vec.pset, index, vec.engine), batch=k) as bfs:
        bfs.begin()
        bfs.run()
        plan = _check(bfs, cp, restated(name, k), npad)
        assert _reaches_goal(bfs, plan)


def test_17_movables():
    text = rgd_puzzles.ladder(16, 0)
    cp, oz = oracles("ladder 16", text)
    assert cp.num_movables == 17
    ref = _restate(cp, oz, 3, max_rounds=6)
    with PushBestFirstSearch(PushWorldPuzzle(text=text), batch=3) as bfs:
        bfs.begin()
        bfs.run(6)
        plan = _check(bfs, cp, ref)
        assert plan is None or _reaches_goal(bfs, plan)
    assert ref.info().states > 1


# ---- 3. keys: a budget of one frame, +inf, exhaustion -----------------------------------------------------------------------------
def test_budget_of_one_frame():
    name, k = "Two Goals", 8
    cp, oz = oracles(name, level1(name))
    ref = _restate(cp, oz, k, rgd_budget=1, graphs=restated(name, k).rgd.graphs)
    assert ref.info().rgd_exceeded > ref.info().states // 2  # most keys are NaN: those states pop newest-first, after the rest
    with PushBestFirstSearch(PushWorldPuzzle(text=level1(name)), batch=k, rgd_budget=1) as bfs:
        bfs.begin()
        bfs.run()
        plan = _check(bfs, cp, ref)
        assert bfs.info.rgd_exceeded == ref.info().rgd_exceeded
        assert plan is None or _reaches_goal(bfs, plan)


@pytest.mark.parametrize("text, k", [(SEALED, 1), (AWAY, 1), (AWAY, 4)])
def test_no_solution_is_exhausted(text, k):
    cp, oz = oracles(text, text)
    ref = _restate(cp, oz, k)
    pz = PushWorldPuzzle(text=text)
    with PushBestFirstSearch(pz, batch=k) as bfs:
        assert bfs.solve() is None and bfs.info.status == "exhausted" and bfs.info.open == 0
        _check(bfs, cp, ref)
        assert text != SEALED or bfs.info.largest_key == -1  # (the sealed agent's one key is +inf)
        mine = {tuple(c.tolist()) + tuple(map(tuple, p[1:].tolist())) for p, c in zip(*_store_arrays(bfs)[:2])}
        with PushBreadthFirstSearch(pz, stop_at_goal=False) as layers:  # an independent implementation of the same closed set
            assert layers.solve() is None and layers.exhausted
            assert bfs.info.states == layers.num_states
            pos, canon = (t.cpu().numpy() for t in layers.states())
            assert mine == {tuple(c.tolist()) + tuple(map(tuple, p[1:].tolist())) for p, c in zip(pos, canon)}


# ---- 4. starts -----------------------------------------------------------------------------------------------------------------------
def test_goal_start_and_bad_start():
    cp, oz = oracles("hand", HAND)
    m0 = cp.py.names.index("m0")
    solved = tuple((4, 2) if j == m0 else xy for j, xy in enumerate(cp.initial_state))
    with PushBestFirstSearch(PushWorldPuzzle(text=HAND), batch=2) as bfs:
        bfs.begin(solved)
        assert tuple(bfs.run()) == (STATUS["solved"], 0, 0, 1, 0, 0, 0, 0, 0, -1)
        assert bfs.plan() == [] and bfs.pushes == 0 and bfs.links()[4].cpu().tolist() == [1]
        _check(bfs, cp, _restate(cp, oz, 2, start=solved))
        for outside in ((cp.width, 2), (-1, 2), (300, 2)):  # a goal start is checked like any other
            with pytest.raises(ValueError, match="outside the grid"):
                bfs.begin((outside,) + solved[1:])
            with pytest.raises(ValueError, match="begin"):
                bfs.run()
        bfs.begin()
        assert bfs.solve() == [1]
        _check(bfs, cp, _restate(cp, oz, 2))


def test_start_other_than_the_initial_state():
    name, k = "2 Obstacle", 8
    full = restated(name, k)
    cp, oz = oracles(name, level1(name))
    start = full.states[5]
    assert start != full.states[0]
    ref = _restate(cp, oz, k, start=start, graphs=full.rgd.graphs)
    with PushBestFirstSearch(PushWorldPuzzle(text=level1(name)), batch=k) as bfs:
        bfs.begin(start)
        bfs.run()
        plan = _check(bfs, cp, ref)
        assert _reaches_goal(bfs, plan, start)


def test_overlapping_start():
    case = SS.CASES[0]
    cp = SS.puzzle(case)
    oz = pw_oracle.OraclePuzzle(SS.text(case))
    start = SS.search_starts(case)[0]
    assert SS.overlapping(cp, start)
    ref = _restate(cp, oz, 4, start=start, max_rounds=4)
    assert ref.info().states > 4
    with PushBestFirstSearch(PushWorldPuzzle(text=SS.text(case)), batch=4) as bfs:
        bfs.begin(start)
        bfs.run(4)
        _check(bfs, cp, ref)


# ---- 5. limits, repetition -------------------------------------------------------------------------------------------------------------
def test_max_states():
    name = "2 Obstacle"
    cp, _ = oracles(name, level1(name))
    pz = PushWorldPuzzle(text=level1(name))
    with PushBestFirstSearch(pz, batch=1, max_states=97) as bfs:
        bfs.begin()
        info = bfs.run()
        assert (info.status, info.rounds, info.states, info.open, info.push_rows) == ("limit", 33, 73, 40, 475)
        _check(bfs, cp, restated(name, 1, 97))
        assert bfs.run() == info and bfs.run(3) == info  # the same info again
        with pytest.raises(RuntimeError, match="max_states = 97"):
            bfs.solve()
        with pytest.raises(ValueError, match="not solved"):
            bfs._handle.plan()
        bfs.begin()  # begin starts afresh
        assert bfs.run(2).status == "running" and bfs.run() == info
        _check(bfs, cp, restated(name, 1, 97))
    with PushBestFirstSearch(pz, batch=1, max_states=138) as bfs:
        bfs.begin()
        assert bfs.run().status == "solved"
        _check(bfs, cp, restated(name, 1, 138))
        assert tuple(bfs.info) == _info_words(restated(name, 1).info())


def test_identical_runs_and_begin_again():
    name, k = "Two Goals", 8
    cp, _ = oracles(name, level1(name))
    pz = PushWorldPuzzle(text=level1(name))
    stores = []
    for _ in range(2):  # two fresh handles
        with PushBestFirstSearch(pz, batch=k) as bfs:
            bfs.begin()
            stores.append((tuple(bfs.run()), _store_arrays(bfs), bfs.plan()))
    with PushBestFirstSearch(pz, batch=k) as bfs:  # begin, run, begin, run on one handle
        bfs.begin()
        bfs.run(2)
        bfs.begin()
        stores.append((tuple(bfs.run()), _store_arrays(bfs), bfs.plan()))
        _check(bfs, cp, restated(name, k))
    for info, arrays, plan in stores[1:]:
        assert info == stores[0][0] and plan == stores[0][2]
        assert all(g.shape == w.shape and (g == w).all() for g, w in zip(arrays, stores[0][1]))


def test_fewer_states_than_breadth_first():
    pz = PushWorldPuzzle(text=level1("2 Obstacle"))
    with PushBestFirstSearch(pz, batch=1, max_states=4096) as bfs:
        plan = bfs.solve()
        assert pz.is_valid_plan(plan) and bfs.info.status == "solved"
        with PushBreadthFirstSearch(pz, max_states=4096) as layers:
            layers.solve()
            assert bfs.num_states < layers.num_states == 416


# ---- 6. the C ABI's checks that need a handle, and the command line ------------------------------------------------------------------
def test_checks_on_a_handle():
    pz = PushWorldPuzzle(text=level1("Single Obstacle"))
    eng, lib = pz._engine(), _capi.lib
    out = ctypes.c_void_p()
    for index in (-1, 1, 7):
        assert lib.pw_push_planner_create(eng.handle, index, 64, 1, 0, ctypes.byref(out)) == _capi.PW_EINVAL
        assert "pw_push_planner_create" in _capi.last_error() and "puzzle index" in _capi.last_error() and not out.value
    info = (ctypes.c_int64 * 10)()
    buf = (ctypes.c_uint8 * 64)()
    with PushBestFirstSearch(pz, max_states=64) as bfs:
        h = bfs._handle.handle
        for name, call in (("pw_push_planner_run", lambda: lib.pw_push_planner_run(h, 0, info, None)),
                           ("pw_push_planner_plan", lambda: lib.pw_push_planner_plan(h, buf, 64, None, None)),
                           ("pw_push_planner_read_states", lambda: lib.pw_push_planner_read_states(h, 0, 1, None, None, None))):
            assert call() == _capi.PW_EINVAL
            assert name in _capi.last_error() and "pw_push_planner_begin has not been called" in _capi.last_error()
        assert lib.pw_push_planner_run(h, 0, None, None) == _capi.PW_EINVAL and "null info" in _capi.last_error()
        bfs.begin()
        assert lib.pw_push_planner_plan(h, buf, 64, None, None) == _capi.PW_EINVAL  # begun, not solved
        assert "pw_push_planner_plan" in _capi.last_error() and "not solved" in _capi.last_error()
        assert lib.pw_push_planner_read_states(h, 0, 2, None, None, None) == _capi.PW_EINVAL
        assert "out of bounds" in _capi.last_error()
        assert bfs.solve() is not None


def test_command_line(capsys):
    name = "Single Obstacle"
    path = os.path.join(DATA, "puzzles", "level1", name + ".pwp")
    assert run_planner.main(["--pushes", "--best-first", path, "--batch", "8"]) == 0
    line = capsys.readouterr().out.strip()
    pz = PushWorldPuzzle(path, order="cpp")
    assert line and set(line) <= set("LRUD") and pz.is_valid_plan(["LRUD".index(c) for c in line])
    assert run_planner.main(["--pushes", "--best-first", path, "--max-states", "1"]) == 1
    assert "max_states = 1" in capsys.readouterr().err

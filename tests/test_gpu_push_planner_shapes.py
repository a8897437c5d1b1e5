"""Best-first search over pushes on the device (pw_push_planner_*, search.PushBestFirstSearch) on the runs of
tests/shape_states.py (``PLANNER_*``): overlapping starts of the random-shape puzzles, queues that hold finite, +inf and NaN
keys at once, rounds that pop more than 256 states, goal rows whose successor lies outside the grid, 16- and 32-padded rows with
12 and 18 movables, the 30 x 30 board, `exhausted` and `limit` from overlapping starts, and a searched puzzle that is not the
largest of its set.  Every store is compared with the restatement's by ``test_gpu_push_planner._check`` -- the ten info words,
pos with its zero padding, canon, every link field of every state in store order, the plan and its pushes;
tests/test_push_planner_shapes_host.py computes the restatements (once per session) and pins what the runs were chosen for."""
import numpy as np
import pytest

import shape_states as SS
import test_push_planner_shapes_host as H
import walk_restatement as WR
from pushworld_amd.puzzle import PushWorldPuzzle
from pushworld_amd.search import PushBestFirstSearch, SetPuzzle
from pushworld_amd.vec_env import VecPushWorld
from test_gpu_push_planner import _check, _reaches_goal, _store_arrays
from test_gpu_walk import TABLES

pytestmark = pytest.mark.gpu

_PUZZLES, _SETS = {}, {}


def _puzzle(case):
    if case not in _PUZZLES:
        _PUZZLES[case] = PushWorldPuzzle(text=H.text_of(case))
    return _PUZZLES[case]


def _search(run, puzzle=None):
    return PushBestFirstSearch(_puzzle(run.case) if puzzle is None else puzzle, batch=run.k,
                               max_states=1 << 20 if run.max_states is None else run.max_states, rgd_budget=run.budget)


def _ends_in_goal(bfs, cp, ref, plan, start):
    """The plan of a solved run through pw_plan_states and through the C oracle: both end in the store's last state, a goal
    state -- inside its grid or not."""
    assert _reaches_goal(bfs, plan, start)
    first = None if start is None else np.ascontiguousarray(np.asarray(start, np.int8))
    states, goals = bfs._engine.plan_states(bfs.puzzle_index, bytes(plan), start=first)
    assert (states[-1] == np.asarray(ref.states[-1], np.int8)).all() and not goals[:-1].any()
    state = ref.states[0]
    for a in plan:
        state = cp.get_next_state(state, a)
    assert cp.py.is_goal_state(state) and tuple(state) == tuple(ref.states[-1])


def _run_and_check(run, bfs, npad=None):
    cp, _ = H.oracles_of(run.case)
    ref = H.restated(run).ref
    start = SS.planner_start(run)
    bfs.begin(start)
    info = bfs.run(run.rounds)
    plan = _check(bfs, cp, ref, npad)
    assert (info.status,) + tuple(info[1:]) == H.PINNED[run]
    if info.status == "solved":
        _ends_in_goal(bfs, cp, ref, plan, start)
    return info


# ---- 1. every run of the list ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", SS.PLANNER_RUNS, ids=H.run_id)
def test_runs(run):
    cp, _ = H.oracles_of(run.case)
    with _search(run) as bfs:
        info = _run_and_check(run, bfs)
        if run in SS.PLANNER_GOAL_OUTSIDE:  # the goal state is in no grid: canon (0, 0), the coordinates as pushed
            pos, canon = (t.cpu().numpy() for t in bfs.states(info.goal_index, 1))
            state = tuple(map(tuple, pos[0, :cp.num_movables].tolist()))
            assert not WR.in_grid(cp, state) and tuple(canon[0]) == (0, 0) and info.goal_index == info.states - 1
        if run == SS.PLANNER_LIMIT:
            assert bfs.run() == info and bfs.plan() is None  # at its end a run changes nothing
            with pytest.raises(RuntimeError, match="max_states = %d" % run.max_states):
                bfs.solve()


# ---- 2. rounds one by one ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", [SS.PLANNER_NAN[9], SS.PLANNER_BUDGET_RUNS[0]], ids=H.run_id)
def test_rounds_one_by_one(run):
    cp, _ = H.oracles_of(run.case)
    got = H.restated(run)
    with _search(run) as bfs:
        bfs.begin(SS.planner_start(run))
        states = 1
        for k, want in enumerate(got.rounds):
            info = bfs.run(1)
            states += want.appended
            assert (info.status, info.rounds, info.states) == ("running", k + 1, states)
        _check(bfs, cp, got.ref)
        one_by_one = _store_arrays(bfs)
        bfs.begin(SS.planner_start(run))
        bfs.run(run.rounds)
        assert all(g.shape == w.shape and (g == w).all() for g, w in zip(_store_arrays(bfs), one_by_one))


# ---- 3. one handle, several searches ---------------------------------------------------------------------------------------------
def test_handle_reuse_after_a_goal_outside_the_grid():
    """`solved` at a goal row outside the grid, then another start on the same handle: the goal word, the closed set and the
    queue start afresh."""
    first, second = SS.PLANNER_GOAL_OUTSIDE[0], SS.PLANNER_MIXED[7]
    assert first.k == second.k == 64 and second.start == 9
    with _search(first) as bfs:
        assert _run_and_check(first, bfs).status == "solved"
        assert _run_and_check(second, bfs).goal_index == -1
        assert _run_and_check(first, bfs).status == "solved"


def test_handle_reuse_resets_the_overruns():
    first, second = SS.PLANNER_BUDGET_RUNS
    assert (first.k, first.budget) == (second.k, second.budget)
    with _search(first) as bfs:
        assert _run_and_check(first, bfs).rgd_exceeded == 7
        assert _run_and_check(second, bfs).rgd_exceeded == 9


# ---- 4. the searched puzzle is not the largest of its set ----------------------------------------------------------------------
def _set(tables):
    """All six puzzles in one set: 32-padded rows and boards of 64 rows, whichever puzzle is searched."""
    if tables not in _SETS:
        _SETS[tables] = VecPushWorld([PushWorldPuzzle(text=SS.text(c)) for c in SS.CASES], len(SS.CASES), observation=None,
                                     max_steps=None, engine_options={"step_tables": tables})
    return _SETS[tables]


@pytest.mark.parametrize("tables", TABLES)
@pytest.mark.parametrize("run", [SS.PLANNER_MIXED[6], SS.PLANNER_EXHAUSTED[0]], ids=H.run_id)
def test_searched_puzzle_is_not_the_largest_of_its_set(run, tables):
    vec = _set(tables)
    index = SS.CASES.index(run.case)
    assert (run.k, index) in ((4, 2), (4, 1)) and vec.num_objects_padded == 32 > SS.PADDING[run.case]
    assert max(SS.FRAME.values()) == 64 > SS.FRAME[run.case]
    with _search(run, SetPuzzle(vec.pset, index, vec.engine)) as bfs:
        _run_and_check(run, bfs, 32)
        in_set = _store_arrays(bfs)
    with _search(run) as bfs:  # the same search in the set of that puzzle alone
        _run_and_check(run, bfs)
        alone = _store_arrays(bfs)
    n = SS.PADDING[run.case]
    assert in_set[0].shape[1:] == (32, 2) and alone[0].shape[1:] == (n, 2)
    assert (in_set[0][:, :n] == alone[0]).all() and (in_set[0][:, n:] == 0).all()
    assert all(g.shape == w.shape and (g == w).all() for g, w in zip(in_set[1:], alone[1:]))


# ---- 5. fingerprint bits -------------------------------------------------------------------------------------------------------
def test_one_fingerprint_bit():
    """One bit of fingerprint: nearly every probe of the closed set meets an equal one and the exact comparison decides."""
    run = SS.PLANNER_BUDGET_RUNS[1]
    eng = _puzzle(run.case)._engine()
    eng.set_option("push_search_fp_bits", 1)
    try:
        with _search(run) as bfs:
            _run_and_check(run, bfs)
    finally:
        eng.set_option("push_search_fp_bits", 0)

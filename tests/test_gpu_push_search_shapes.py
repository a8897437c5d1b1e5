"""Breadth-first search over pushes on the device (pw_push_search_*, search.PushBreadthFirstSearch, search.PushSearch; DESIGN.md
K16) from overlapping starts of the random-shape puzzles of tests/shape_states.py.  The layers of such starts hold rows whose
successor lies outside its grid -- no candidate of the closed set -- and goal rows among them, which end the store without owning
a canonical state.  Every store is compared field by field, in store order, with tests/push_search_restatement.py
(``test_gpu_push_search._check_store``); tests/test_walk_shapes_host.py pins what the starts were chosen for."""
import numpy as np
import pytest
import torch

import push_search_restatement as PR
import shape_states as SS
import walk_restatement as WR
from pushworld_amd.puzzle import PushWorldPuzzle
from pushworld_amd.search import PushBreadthFirstSearch, PushSearch, walk_regions
from test_gpu_push_search import _check_store, _counters, _with_bits

pytestmark = pytest.mark.gpu

VARIANTS = ["default", "chunk 5", "1 fingerprint bit"]  # the same stores from many passes per layer and from exact compares alone
_PUZZLES = {}


def _puzzle(case):
    if case not in _PUZZLES:
        _PUZZLES[case] = PushWorldPuzzle(text=SS.text(case))
    return _PUZZLES[case]


def _run(case, variant, start, stop_at_goal, max_pushes, check):
    """One search from `start` under `variant`; `check(bfs, plan)` runs inside it."""
    pz = _puzzle(case)

    def run():
        with PushBreadthFirstSearch(pz, stop_at_goal=stop_at_goal, chunk=5 if variant == "chunk 5" else None) as bfs:
            bfs.begin(start)
            check(bfs, bfs.solve(max_pushes=max_pushes))

    _with_bits(pz, 1 if variant == "1 fingerprint bit" else 0, run)


def _check_plans(case, bfs, st, pos, step=7):
    """plan(i) of every `step`-th state against the restatement's; a state inside its grid is what the plan replays to."""
    cp, pz = SS.puzzle(case), _puzzle(case)
    start = np.ascontiguousarray(np.asarray(st.states[0], np.int8))
    for i in range(0, st.num_states, step):
        plan = bfs.plan(i)
        assert plan == PR.plan_of(cp, st, i), i
        if WR.in_grid(cp, st.states[i]):
            got, _ = pz._engine().plan_states(0, bytes(plan), start=start)
            assert (got[-1] == pos[i, :cp.num_movables]).all(), i


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("case", SS.SMALL)
def test_three_layers_from_overlapping_starts(case, variant):
    cp = SS.puzzle(case)
    for start in SS.search_starts(case):
        st = SS.store(case, start, stop_at_goal=False, max_pushes=3)

        def check(bfs, plan):
            assert plan is None and _counters(bfs) == _counters(st)
            pos, *_ = _check_store(bfs, cp, st)
            if variant == "default":
                _check_plans(case, bfs, st, pos)

        _run(case, variant, start, False, 3, check)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("case", SS.SMALL)
def test_stop_at_goal_from_goal_near_starts(case, variant):
    cp = SS.puzzle(case)
    met = 0
    for start in SS.goal_starts(case):
        st = SS.store(case, start, max_pushes=3)
        met += st.goal_index >= 0

        def check(bfs, plan):
            assert _counters(bfs) == _counters(st)
            pos, *_ = _check_store(bfs, cp, st)
            if st.goal_index >= 0:
                assert plan == PR.plan_of(cp, st, st.goal_index) and bfs.num_states == bfs.goal_index + 1
            else:
                assert plan is None
            if variant == "default":
                _check_plans(case, bfs, st, pos)

        _run(case, variant, start, True, 3, check)
    assert met >= 3


@pytest.mark.parametrize("variant", VARIANTS)
def test_goal_row_with_a_successor_outside_the_grid(variant):
    """The search ends at a goal row that owns no canonical state: its successor is published as the last state, with canon
    (0, 0), in the first layer (states 29 and 30 of the list) and in the third (GOAL_OUTSIDE_STARTS)."""
    case = SS.CASES[2]
    cp = SS.puzzle(case)
    for start in [SS.states(case)[k].state for k in SS.GOAL_OUTSIDE_LISTED] + SS.GOAL_OUTSIDE_STARTS:
        st = SS.store(case, start)
        g = st.goal_index
        assert g == st.num_states - 1 and not WR.in_grid(cp, st.states[g])

        def check(bfs, plan):
            assert (bfs.goal_index, bfs.num_states, bfs.pushes) == (g, st.num_states, st.pushes)
            pos, canon = (t.cpu().numpy() for t in bfs.states(g, 1))
            assert (pos[0, :cp.num_movables] == np.asarray(st.states[g], np.int8)).all() and (pos[0, cp.num_movables:] == 0).all()
            assert tuple(canon[0]) == st.canons[g] == (0, 0)
            parent, frm, action, walk, goal = (t.cpu().numpy() for t in bfs.links(g, 1))
            assert PR.Link(int(parent[0]), tuple(frm[0]), int(action[0]), int(walk[0]), bool(goal[0])) == st.links[g]
            assert plan == bfs.plan(g) == PR.plan_of(cp, st, g)
            assert _counters(bfs) == _counters(st)
            _check_store(bfs, cp, st)

        _run(case, variant, start, True, None, check)


def test_many_movables_one_layer():
    """19 and 32 movables: canonical states of 9 and 16 words, no 63-bit key."""
    for case, start, words in ((SS.CASES[4], SS.states(SS.CASES[4])[SS.MANY_START_18].state, 9), (SS.CASES[5], SS.MANY_START_32, 16)):
        cp = SS.puzzle(case)
        assert (cp.num_movables + 1) // 2 == words and SS.overlapping(cp, start)
        st = SS.store(case, start, stop_at_goal=False, max_pushes=1)
        assert st.num_states >= 20 and any(not WR.in_grid(cp, pm.next_state) for pm in SS.region(case, start).pushes)
        for variant in VARIANTS:
            def check(bfs, plan):
                assert plan is None and _counters(bfs) == _counters(st)
                pos, *_ = _check_store(bfs, cp, st)
                if variant == "default":
                    _check_plans(case, bfs, st, pos, step=5)

            _run(case, variant, start, False, 1, check)


def test_many_movables_layer_of_hundreds_of_rows():
    """One layer from the initial state of the 64 x 64 board: 393 push rows of 16 words each.  No restatement of 393 regions of
    2 400 positions: the store against the restatement's rows of the start, and against the host-driven search's dedupe
    (torch.unique over whole rows) of the canon that pw_walk_regions gives -- which tests/test_gpu_walk_shapes.py compares."""
    case = SS.CASES[5]
    cp, pz = SS.puzzle(case), _puzzle(case)
    r = SS.region(case, cp.initial_state)
    ps = PushSearch(pz)
    assert ps.solve(max_pushes=1, stop_at_goal=False) is None
    assert (ps.push_rows, ps.largest_region) == (len(r.pushes), len(r.dist)) and len(r.pushes) > 300
    with PushBreadthFirstSearch(pz, stop_at_goal=False, chunk=5) as bfs:
        assert bfs.solve(max_pushes=1) is None
        assert _counters(bfs) == _counters(ps) and bfs.num_states > 100
        pos, canon = bfs.states()
        parent, frm, action, walk, goal = (t.cpu().numpy() for t in bfs.links())
        # every state of the layer is the successor of the row its link names, in row order
        rows = {(pm.frm, pm.action): (k, pm) for k, pm in enumerate(r.pushes)}
        at = [rows[(tuple(frm[i]), int(action[i]))] for i in range(1, bfs.num_states)]
        assert [k for k, _ in at] == sorted(k for k, _ in at) and (parent[1:] == 0).all()
        assert (pos.cpu().numpy()[1:, :32] == np.asarray([pm.next_state for _, pm in at], np.int8)).all()
        assert walk[1:].tolist() == [pm.walk for _, pm in at] and goal[1:].tolist() == [int(pm.goal) for _, pm in at]
        reg = walk_regions(pz._engine(), torch.zeros(bfs.num_states, dtype=torch.int32, device=pos.device), pos)
        assert torch.equal(reg.canon, canon)


@pytest.mark.parametrize("case", SS.SMALL)
def test_host_driven_search_from_the_same_starts(case):
    """PushSearch.solve(start=, max_pushes=, stop_at_goal=): plan and counters against walk_restatement.push_search and against
    PushBreadthFirstSearch.  The two count alike but for a goal row with a successor outside its grid, which the store holds
    as its last state and the closed set does not."""
    cp, pz = SS.puzzle(case), _puzzle(case)
    ps = PushSearch(pz)
    runs = [(s, False) for s in SS.search_starts(case)] + [(s, True) for s in SS.goal_starts(case)]
    if case == SS.CASES[2]:
        runs += [(s, True) for s in SS.GOAL_OUTSIDE_STARTS]
    unowned = 0
    for start, stop in runs:
        want = WR.push_search(cp, start=start, max_pushes=3, stop_at_goal=stop)
        plan = ps.solve(start=start, max_pushes=3, stop_at_goal=stop)
        assert plan == want.plan
        assert (ps.layer_states, ps.num_states, ps.pushes) == (want.layer_states, want.num_states, want.pushes)
        assert (ps.push_rows, ps.largest_region) == (want.push_rows, want.largest_region)
        st = SS.store(case, start, stop_at_goal=stop, max_pushes=3)
        extra = int(st.goal_index >= 0 and not WR.in_grid(cp, st.states[st.goal_index]))
        unowned += extra
        with PushBreadthFirstSearch(pz, stop_at_goal=stop) as bfs:
            bfs.begin(start)
            assert bfs.solve(max_pushes=3) == plan
            assert (bfs.layer_states, bfs.pushes, bfs.push_rows, bfs.largest_region) == (ps.layer_states, ps.pushes, ps.push_rows,
                                                                                         ps.largest_region)
            assert bfs.num_states == ps.num_states + extra
    assert unowned >= (4 if case == SS.CASES[2] else 0)

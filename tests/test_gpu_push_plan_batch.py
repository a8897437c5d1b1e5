"""Best-first search over pushes of many puzzles or live states in one launch (pw_push_plan_batch_*, search.PushPlanBatch /
PushStatePlanner).  The puzzles form is checked against the plain-Python restatement of K17's semantics
(tests/push_planner_restatement.py, the runs that tests/test_push_planner_host.py shares and pins); the states form against
``PushBestFirstSearch`` (K17 on the same device: existing code, not the code under test).  The restatements at K = 64 of `Simple
Tool` and `Walk Past` take about 5 s and 12 s of CPU once per session; everything on the device takes milliseconds."""
import ctypes

import numpy as np
import pytest
import torch

import push_planner_restatement as PP
import shape_states as SS
from pushworld_amd import _capi
from pushworld_amd.puzzle import PushWorldPuzzle
from pushworld_amd.search import (PLAN_STATUS, PUSH_NONE, REPLAY_VALID, PushBestFirstSearch, PushPlanBatch, PushStatePlanner,
                                  SetPuzzle, replay_plans, solve_many_pushes)
from pushworld_amd.vec_env import VecPushWorld
from test_push_planner_host import PINNED, level1, oracles, restated
from test_walk_host import HAND

pytestmark = pytest.mark.gpu

NAMES = ("Single Obstacle", "Two Goals", "2 Obstacle", "Simple Tool", "Walk Past")
KS = (1, 8, 64)
MAX_STATES = 1 << 14  # (no run below comes near it: `Walk Past` at K = 64 stores 2 347 states and lists 4 376 rows in all)
STATUS = {v: k for k, v in PLAN_STATUS.items()}
_PUZZLES = {}


def _puzzle(name):
    if name not in _PUZZLES:
        _PUZZLES[name] = PushWorldPuzzle(text=level1(name))
    return _PUZZLES[name]


def _info_words(i):
    return (STATUS[i.status],) + tuple(i[1:])


def _ref_pushes(ref):
    """The restatement's chain of links from the start to the goal state: [(from, action)]."""
    out, index = [], ref.goal_index
    while ref.links[index].parent >= 0:
        ln = ref.links[index]
        out.append((tuple(ln.frm), ln.action))
        index = ln.parent
    return out[::-1]


def _check_store(pb, item, cp, ref):
    pos, canon = (t.cpu().numpy() for t in pb.states(item))
    parent, frm, action, goal = (t.cpu().numpy() for t in pb.links(item))
    n, N = len(ref.states), cp.num_movables
    assert pos.shape == (n, pb.npad, 2) and pos.dtype == np.int8 and canon.shape == (n, 2)
    assert (pos[:, :N] == np.asarray(ref.states, np.int8)).all() and (pos[:, N:] == 0).all()
    assert (canon == np.asarray(ref.canons, np.int8)).all()
    assert parent.tolist() == [ln.parent for ln in ref.links]
    assert [tuple(q) for q in frm.tolist()] == [tuple(ln.frm) for ln in ref.links]
    assert action.tolist() == [ln.action for ln in ref.links]
    assert goal.tolist() == [int(ln.goal) for ln in ref.links]


# ---- 1. the pinned puzzles, one batch per K -------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_pinned_puzzles_in_one_launch(k):
    with PushPlanBatch([_puzzle(n) for n in NAMES], batch=k, max_states=MAX_STATES) as pb:
        pb.run()
        results = pb.results()
        plans, plan_len, pushes = (t.cpu().numpy() for t in pb.primitive_plans())
        verdict = pb.validate().cpu().tolist()
        ids = torch.arange(len(NAMES), dtype=torch.int32, device=pb.device)
        again = replay_plans(pb._engine, ids, *pb.primitive_plans()[:2], rows=False).verdict.cpu().tolist()
        assert verdict == again == [REPLAY_VALID] * len(NAMES)
        for i, name in enumerate(NAMES):
            ref = restated(name, k)
            cp, _ = oracles(name, level1(name))
            got, info, seconds = results[i]
            want = ref.info()
            print(name, k, tuple(info), _info_words(want), seconds)
            assert tuple(info) == _info_words(want) and info.status == want.status == "solved" and seconds > 0
            want_plan, want_pushes = ref.plan()
            if (name, k) in PINNED:
                assert (info.status, info.rounds, info.expanded, info.states, info.open, info.push_rows, len(got),
                        info.largest_region, info.largest_key) == PINNED[name, k]
            assert got == _ref_pushes(ref) and len(got) == want_pushes == int(pushes[i])
            assert plans[i, :plan_len[i]].tolist() == want_plan and _puzzle(name).is_valid_plan(want_plan)
            _check_store(pb, i, cp, ref)
    assert [r[0] for r in solve_many_pushes([_puzzle(n) for n in NAMES[:2]], batch=k, max_states=MAX_STATES)] == \
        [_ref_pushes(restated(n, k)) for n in NAMES[:2]]


def test_max_rounds():
    name = "2 Obstacle"
    cp, oz = oracles(name, level1(name))
    ref = PP.PushPlannerRestatement(cp, oz, batch=1, graphs=restated(name, 1).rgd.graphs)
    ref.begin()
    ref.run(3)
    with PushPlanBatch([_puzzle(name)], batch=1, max_states=MAX_STATES) as pb:
        pb.run(max_rounds=3)
        (got, info, _), = pb.results()
        assert got is None and info.status == "running" and info.rounds == 3
        assert tuple(info) == _info_words(ref.info())
        _check_store(pb, 0, cp, ref)
        assert pb.primitive_plans()[1].cpu().tolist() == [-1]


# ---- 2. slabs and tags are reused ---------------------------------------------------------------------------------------------------
def test_slab_reuse():
    """300 items that repeat the five puzzles, run twice on one handle: every repeat and both runs give the same info and plans.
    A device has up to two workgroups per CU, so 300 items may each get a slab of their own; the states form below runs 1 500
    items, more than any device has workgroups, so that slabs and tags are reused within a launch too."""
    repeat = 60
    with PushPlanBatch([_puzzle(n) for n in NAMES] * repeat, batch=8, max_states=1 << 12) as pb:
        runs = []
        for _ in range(2):
            pb.run()
            info, plan_len, plan_from, plan_action, plan_pos = (t.cpu().numpy() for t in pb._out)
            runs.append((info[:, :10], plan_len, plan_from, plan_action, plan_pos))
        for a, b in zip(*runs):
            assert (a == b).all()
        info, plan_len, plan_from, plan_action, plan_pos = runs[0]
        for i, name in enumerate(NAMES):
            assert tuple(info[i]) == _info_words(restated(name, 8).info())
            for arr in runs[0]:
                assert (arr[i::len(NAMES)] == arr[i]).all(), name
    vec = VecPushWorld([_puzzle(n) for n in NAMES], 5 * 300, observation=None, max_steps=None)
    vec.reset()
    with vec.push_planner(batch=8, max_states=1 << 12) as planner:
        for _ in range(2):
            q = vec.planned_pushes(planner, push_cap=32)
            info = planner.info().cpu().numpy()[:, :10]
            results = planner.results()
            for i, name in enumerate(NAMES):
                assert (info[i::len(NAMES)] == np.asarray(_info_words(restated(name, 8).info()))).all(), name
                assert all(r[0] == _ref_pushes(restated(name, 8)) for r in results[i::len(NAMES)])
            assert (q.pushes > 0).all() and (q.push_action != PUSH_NONE).all()


# ---- 3. items beyond the limits ---------------------------------------------------------------------------------------------------
def test_skipped_items():
    names = ("Two Goals", "Pull Up", "Simple Tool", "Irrelevant Obstacles", "Single Obstacle")
    puzzles = [PushWorldPuzzle(text=level1(n)) for n in names]
    assert (puzzles[1]._parsed.width, puzzles[1]._parsed.height) == (20, 20) and puzzles[3].num_movables == 11
    with PushPlanBatch(puzzles, batch=8, max_states=MAX_STATES) as pb:
        pb.run()
        results = pb.results()
        info = pb._out[0].cpu().numpy()
        plan_len = pb._out[1].cpu().tolist()
        for i, name in enumerate(names):
            if i in (1, 3):
                assert results[i][1].status == "skipped" and results[i][0] is None and plan_len[i] == -1
                assert info[i].tolist() == [6] + [0] * 10
                with pytest.raises(ValueError, match="store is gone"):
                    pb.states(i, 0, 1)
            else:
                assert tuple(results[i][1]) == _info_words(restated(name, 8).info())
                assert results[i][0] == _ref_pushes(restated(name, 8))
        assert pb.primitive_plans()[1].cpu().tolist()[1::2] == [-1, -1]
    vec = VecPushWorld(puzzles, 10, observation=None, max_steps=None)
    vec.reset()
    with vec.push_planner(batch=8, max_states=MAX_STATES) as planner:
        q = vec.planned_pushes(planner)
        status, pushes, act, frm = (t.cpu().tolist() for t in (q.status, q.pushes, q.push_action, q.push_from))
        for e in range(10):
            if e % 5 in (1, 3):
                assert (status[e], pushes[e], act[e], frm[e]) == (STATUS["skipped"], -1, PUSH_NONE, [0, 0])
            else:
                ref = restated(names[e % 5], 8)
                assert status[e] == STATUS["solved"] and pushes[e] == len(_ref_pushes(ref))
                assert (tuple(frm[e]), act[e]) == _ref_pushes(ref)[0]


# ---- 4. the states form against K17 on the same device --------------------------------------------------------------------------------
K_STATES, ROUNDS_STATES, MAX_STATES_LIVE = 8, 12, 1 << 13


def _live_batch():
    """48 environments over the five puzzles after 0 .. 12 seeded random steps, then the overlapping starts of the one shape
    case within the limits (14 x 14 cells with the border, 3 movables; the next one is 18 x 18)."""
    case = SS.CASES[0]
    puzzles = [_puzzle(n) for n in NAMES] + [PushWorldPuzzle(text=SS.text(case))]
    shaped = [(5, s) for s in SS.search_starts(case) + SS.DEEP_GOAL_STARTS[case]]
    assert all(SS.overlapping(SS.puzzle(case), s) for s in SS.search_starts(case))
    ids = [e % 5 for e in range(48)] + [pid for pid, _ in shaped]
    vec = VecPushWorld(puzzles, len(ids), puzzle_ids=ids, observation=None, max_steps=None)
    assert vec.num_objects_padded == 8
    vec.reset()
    gen = torch.Generator().manual_seed(24)
    snaps = [vec.pos.clone()]
    for _ in range(12):
        vec.step(torch.randint(0, 4, (len(ids),), generator=gen, dtype=torch.uint8).to(vec.device))
        snaps.append(vec.pos.clone())
    pos = torch.stack([snaps[e % 13][e] for e in range(len(ids))]).cpu().numpy()
    for e, (_, state) in enumerate(shaped, 48):
        pos[e] = 0
        pos[e, :len(state)] = np.asarray(state, np.int8)
    vec.reset()
    vec.set_states(pos)
    return vec, pos, ids


def test_live_states_against_the_single_puzzle_search():
    vec, pos, ids = _live_batch()
    n = len(ids)
    mask = torch.ones(n, dtype=torch.uint8, device=vec.device)
    mask[3] = mask[50] = 0
    with vec.push_planner(batch=K_STATES, max_states=MAX_STATES_LIVE) as planner:
        q = vec.planned_pushes(planner, mask=mask, max_rounds=ROUNDS_STATES, push_cap=64)
        info = planner.info().cpu().numpy()
        results = planner.results()
        first_from, first_action, pushes = (t.cpu().tolist() for t in (q.push_from, q.push_action, q.pushes))
        assert planner.validate().cpu().tolist() == [REPLAY_VALID if r[0] is not None else -1 if m else -3
                                                     for r, m in zip(results, mask.cpu().tolist())]
        searches = {}
        solved = 0
        for e in range(n):
            if e in (3, 50):
                assert info[e].tolist() == [6] + [0] * 10 and (pushes[e], first_action[e], first_from[e]) == (-1, PUSH_NONE, [0, 0])
                continue
            pid = ids[e]
            if pid not in searches:
                searches[pid] = PushBestFirstSearch(SetPuzzle(vec.pset, pid, vec.engine), batch=K_STATES, max_states=MAX_STATES_LIVE)
            bfs = searches[pid]
            start = [tuple(int(v) for v in xy) for xy in pos[e, :bfs.num_objects]]
            bfs.begin(start)
            want = bfs.run(ROUNDS_STATES)
            assert tuple(info[e, :10]) == tuple(want), (e, pid, tuple(info[e, :10]), tuple(want))
            chain = None
            if want.status == "solved":
                parent, frm, action, _, _ = (t.cpu().tolist() for t in bfs.links())
                chain, at = [], want.goal_index
                while parent[at] >= 0:
                    chain.append((tuple(frm[at]), action[at]))
                    at = parent[at]
                chain = chain[::-1]
                solved += 1
            assert results[e][0] == chain, e
            assert pushes[e] == (len(chain) if chain is not None else -1)
            assert (tuple(first_from[e]), first_action[e]) == (chain[0] if chain else ((0, 0), PUSH_NONE))
            if e >= 48:  # the stores of the shape starts
                want_pos, want_canon = (t.cpu().numpy() for t in bfs.states())
                got_pos = torch.empty((want.states, 8, 2), dtype=torch.int8, device=vec.device)
                got_canon = torch.empty((want.states, 2), dtype=torch.int8, device=vec.device)
                planner.handle.read_states(e, 0, want.states, got_pos, 8, got_canon)
                assert (got_pos.cpu().numpy() == want_pos).all() and (got_canon.cpu().numpy() == want_canon).all()
        for bfs in searches.values():
            bfs.close()
        assert solved >= 40
        # ids outside the set, a puzzle the planner did not prepare
        other = vec.puzzle_id.clone()
        other[0], other[1], other[2] = -1, 7, 1 << 20
        q2 = planner.plan(other, vec.pos, max_rounds=ROUNDS_STATES)
        assert q2.status[:3].cpu().tolist() == [6, 6, 6] and q2.pushes[:3].cpu().tolist() == [-1, -1, -1]
        assert q2.push_action[:3].cpu().tolist() == [PUSH_NONE] * 3
        assert (q2.status[4:48] == q.status[4:48]).all() and (q2.push_action[4:48] == q.push_action[4:48]).all()
    with vec.push_planner(puzzles=[0, 2], batch=K_STATES, max_states=MAX_STATES_LIVE) as partial:
        q3 = vec.planned_pushes(partial, max_rounds=ROUNDS_STATES)
        prepared = torch.tensor([i in (0, 2) for i in ids], device=vec.device)
        assert ((q3.status == 6) == ~prepared).all() and (q3.pushes[prepared] == q.pushes[prepared]).all()


def test_plan_and_step_by_pushes_until_done():
    vec, pos, ids = _live_batch()
    live = torch.tensor([e < 48 for e in range(len(ids))], device=vec.device)
    with vec.push_planner(batch=K_STATES, max_states=MAX_STATES_LIVE) as planner:
        first = vec.planned_pushes(planner, mask=live)
        solvable = (first.status == STATUS["solved"]) & (first.pushes > 0)
        assert int(solvable.sum()) >= 40 and (first.status[~live] == 6).all()
        done = torch.zeros_like(solvable)
        q = first
        for _ in range(3 * int(first.pushes.max())):
            _, _, terminated, _, _, status = vec.step_push(q.push_from, q.push_action)
            assert ((status == _capi.PUSH_REFUSED) == (q.pushes <= 0)).all()  # refused exactly where there is no push to make
            done |= terminated.bool()
            if bool((done | ~solvable).all()):
                break
            q = vec.planned_pushes(planner, mask=live)
        assert bool(done[solvable].all())


# ---- 5. limits ---------------------------------------------------------------------------------------------------------------------
def test_limits():
    name = "2 Obstacle"
    cp, _ = oracles(name, level1(name))
    with PushPlanBatch([_puzzle(name)], batch=1, max_states=97) as pb:  # K17's limit round (tests/test_gpu_push_planner.py)
        pb.run()
        (got, info, _), = pb.results()
        assert got is None
        assert (info.status, info.rounds, info.states, info.open, info.push_rows) == ("limit", 33, 73, 40, 475)
        assert tuple(info) == _info_words(restated(name, 1, 97).info())
        _check_store(pb, 0, cp, restated(name, 1, 97))
    with PushPlanBatch([_puzzle(name)], batch=1, max_states=MAX_STATES, cost_range=4) as pb:
        pb.run()
        (got, info, _), = pb.results()
        assert got is None and info.status == "range" and info.goal_index == -1


def test_goal_start():
    cp, _ = oracles("hand", HAND)
    m0 = cp.py.names.index("m0")
    solved = [(4, 2) if j == m0 else xy for j, xy in enumerate(cp.initial_state)]
    vec = VecPushWorld([PushWorldPuzzle(text=HAND)], 2, observation=None, max_steps=None)
    vec.reset()
    pos = vec.states()
    pos[1, :len(solved)] = np.asarray(solved, np.int8)
    vec.set_states(pos)
    with vec.push_planner(batch=2) as planner:
        q = vec.planned_pushes(planner, push_cap=8)
        info = planner.info().cpu().numpy()
        assert info[1, :10].tolist() == [STATUS["solved"], 0, 0, 1, 0, 0, 0, 0, 0, -1]
        assert q.pushes.cpu().tolist() == [1, 0] and q.push_action.cpu().tolist()[1] == PUSH_NONE
        assert planner.results()[1][0] == [] and planner.results()[0][1].status == "solved"
        assert planner.primitive_plans()[1].cpu().tolist() == [1, 0]


# ---- 6. the C ABI's checks that need an engine ---------------------------------------------------------------------------------------
def test_checks_on_an_engine():
    vec = VecPushWorld([_puzzle(n) for n in NAMES[:2]], 2, observation=None, max_steps=None)
    lib, out = _capi.lib, ctypes.c_void_p()
    for bad in ([-1], [2], [0, 7]):
        ids = (ctypes.c_int32 * len(bad))(*bad)
        assert lib.pw_push_plan_batch_create(vec.engine.handle, ids, len(bad), 64, 1, 0, 0, ctypes.byref(out)) == _capi.PW_EINVAL
        assert "pw_push_plan_batch_create" in _capi.last_error() and "puzzle index" in _capi.last_error() and not out.value
    with vec.push_planner(max_states=16) as planner:
        h = planner.handle.handle
        buf = torch.zeros(64, dtype=torch.int64, device=vec.device)
        p = ctypes.c_void_p(buf.data_ptr())
        assert lib.pw_push_plan_batch_run(h, 0, 0.0, p, None, None, None, None, 0, 2, None) == _capi.PW_EINVAL
        assert "npad" in _capi.last_error()
        assert lib.pw_push_plan_batch_read_states(h, 0, 0, 1, None, 4, None, None) == _capi.PW_EINVAL
        assert "no run yet" in _capi.last_error()
        vec.reset()
        q = vec.planned_pushes(planner)
        assert q.status.cpu().tolist() == [STATUS["solved"], STATUS["limit"]]  # (`Single Obstacle` stores 8 states, `Two Goals` 17)
        assert lib.pw_push_plan_batch_read_states(h, 0, 0, 1000, None, 4, None, None) == _capi.PW_EINVAL
        assert "out of bounds" in _capi.last_error()
        assert lib.pw_push_plan_batch_read_states(h, 5, 0, 1, None, 4, None, None) == _capi.PW_EINVAL
        assert "store is gone" in _capi.last_error()
        planner.cancel()  # (nothing in flight: the next call runs as usual)
        assert vec.planned_pushes(planner).status.cpu().tolist() == q.status.cpu().tolist()


# ---- 7. a goal state outside its grid ---------------------------------------------------------------------------------------------
# m1 is two cells with a gap.  From OUTSIDE_START its far cell stands in the border column (an overlap), and the push that takes
# m0 to its goal carries that cell out of the grid: the goal row is appended although its successor is outside, canon (0, 0).
OUTSIDE = """
 A M0  .  . G0  .
M1  . M1  .  .  .
""".lstrip("\n")
OUTSIDE_START = ((3, 1), (4, 1), (5, 1))
INSIDE_START = ((1, 2), (3, 1), (5, 1))  # the same puzzle, solved after six rounds at K = 2 by a goal row inside the grid


def test_goal_state_outside_its_grid():
    cp, oz = oracles("outside", OUTSIDE)
    starts = (OUTSIDE_START, INSIDE_START)
    refs = []
    for start in starts:
        ref = PP.PushPlannerRestatement(cp, oz, batch=2)
        ref.begin(start)
        ref.run()
        refs.append(ref)
    assert refs[0].info()[:6] == ("solved", 1, 1, 2, 0, 1) and refs[0].states[-1] == ((4, 1), (5, 1), (6, 1))
    assert refs[0].canons[-1] == (0, 0) and refs[1].status == "solved" and refs[1].canons[-1] != (0, 0)
    pz = PushWorldPuzzle(text=OUTSIDE)
    vec = VecPushWorld([pz], 2, observation=None, max_steps=None)
    assert vec.num_objects_padded == 4
    vec.reset()
    pos = vec.states()
    for e, start in enumerate(starts):
        pos[e, :3] = np.asarray(start, np.int8)
    vec.set_states(pos)
    with vec.push_planner(batch=2) as planner:
        q = vec.planned_pushes(planner, push_cap=16)
        info = planner.info().cpu().numpy()
        results = planner.results()
        for e, ref in enumerate(refs):
            assert tuple(info[e, :10]) == _info_words(ref.info())
            assert results[e][0] == _ref_pushes(ref)
            n = len(ref.states)
            got_pos = torch.empty((n, 4, 2), dtype=torch.int8, device=vec.device)
            got_canon = torch.empty((n, 2), dtype=torch.int8, device=vec.device)
            parent = torch.empty((n,), dtype=torch.int32, device=vec.device)
            frm = torch.empty((n, 2), dtype=torch.int8, device=vec.device)
            action = torch.empty((n,), dtype=torch.uint8, device=vec.device)
            goal = torch.empty((n,), dtype=torch.uint8, device=vec.device)
            planner.handle.read_states(e, 0, n, got_pos, 4, got_canon)
            planner.handle.read_links(e, 0, n, parent, frm, action, goal)
            assert (got_pos.cpu().numpy()[:, :3] == np.asarray(ref.states, np.int8)).all() and (got_pos[:, 3] == 0).all()
            assert (got_canon.cpu().numpy() == np.asarray(ref.canons, np.int8)).all()
            assert parent.cpu().tolist() == [ln.parent for ln in ref.links]
            assert [tuple(f) for f in frm.cpu().tolist()] == [tuple(ln.frm) for ln in ref.links]
            assert action.cpu().tolist() == [ln.action for ln in ref.links]
            assert goal.cpu().tolist() == [int(ln.goal) for ln in ref.links]
        assert (tuple(q.push_from[0].cpu().tolist()), int(q.push_action[0])) == ((3, 1), 1) and int(q.pushes[0]) == 1
    with PushBestFirstSearch(pz, batch=2) as bfs:  # and K17 on the device says the same
        bfs.begin(OUTSIDE_START)
        assert tuple(bfs.run()) == tuple(info[0, :10])
        assert bfs.states()[0].cpu().numpy()[:, :3].tolist() == [list(map(list, s)) for s in refs[0].states]


# ---- 8. captured launches ----------------------------------------------------------------------------------------------------------
def test_captured_run_replays():
    """`run` captured once and replayed: every replay takes fresh closed-set tags on the device, so it equals the eager run."""
    with PushPlanBatch([_puzzle(n) for n in NAMES], batch=8, max_states=1 << 12) as pb:
        pb.run(push_cap=32)
        want = [t.clone() for t in pb._out]
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            pb.run(push_cap=32)
        out = pb._out
        for replay in range(3):
            out[0].fill_(-7)
            out[1].fill_(-7)
            if replay == 2:
                pb.cancel()  # nothing is running: what is replayed afterwards is not cancelled
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out[0][:, :10], want[0][:, :10]), replay
            for got, w in zip(out[1:], want[1:]):
                assert torch.equal(got, w), replay
        for i, name in enumerate(NAMES):
            assert tuple(out[0][i, :10].cpu().tolist()) == _info_words(restated(name, 8).info())
        pb.run(push_cap=32)  # and an eager run after the replays
        assert torch.equal(pb._out[0][:, :10], want[0][:, :10]) and torch.equal(pb._out[2], want[2])


def test_captured_planned_pushes_replays_on_new_states():
    vec = VecPushWorld([_puzzle(n) for n in NAMES], 50, observation=None, max_steps=None)
    vec.reset()
    with vec.push_planner(batch=8, max_states=1 << 12) as planner:
        q0 = [t.clone() for t in vec.planned_pushes(planner, push_cap=16)]  # (eager first: the workgroups exist afterwards)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            q = vec.planned_pushes(planner, push_cap=16)
        captured = planner._out
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(q, q0))
        for step in range(3):  # the states move on; the replay plans from where they are now
            vec.step_push(q0[0], q0[1])
            q0 = [t.clone() for t in vec.planned_pushes(planner, push_cap=16)]
            want_plans = [t.clone() for t in planner._out[1:4]]
            if step == 1:
                torch.cuda.synchronize()  # (the eager call above has ended: a cancel stops what is queued or running)
                planner.cancel()
            g.replay()
            torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(q, q0)), step
            assert all(torch.equal(a, b) for a, b in zip(captured[1:4], want_plans)), step
        assert int((q.pushes > 0).sum()) >= 40

"""The batched best-first search over pushes at its limits (pw_push_plan_batch_*, search.PushPlanBatch / PushStatePlanner;
DESIGN.md K24): 6, 7 and 8 movables, boards 16 cells wide or high, items of different N in one launch, RGD budgets that overrun,
``push_cap``, the time limit, ``cost_range`` and starts and goal states outside their grid.  Every run is a case of
tests/push_plan_limit_cases.py, restated once per session by tests/push_planner_restatement.py (K17's semantics in plain Python
on the oracle; tests/test_push_plan_batch_limits_host.py pins its figures and asserts what each case covers) and compared bit
for bit: the ten info words, the store (the states as reached, zero beyond N, the canon), the links and the push plan.  The
restatements take about 25 s of CPU in all, the longest (`Shape Of You` at K = 64) about 6 s; the device takes milliseconds."""
import numpy as np
import pytest
import torch

import push_plan_limit_cases as C
from pushworld_amd.puzzle import PushWorldPuzzle
from pushworld_amd.search import (PLAN_STATUS, PUSH_NONE, PUSH_PLAN_CUT, REPLAY_NONE, REPLAY_SKIPPED, REPLAY_VALID,
                                  PushBestFirstSearch, PushPlanBatch)
from pushworld_amd.vec_env import VecPushWorld

pytestmark = pytest.mark.gpu

STATUS = {v: k for k, v in PLAN_STATUS.items()}
SKIPPED = [STATUS["skipped"]] + [0] * 10
_PUZZLES = {}


def _puzzle(key):
    if key not in _PUZZLES:
        _PUZZLES[key] = PushWorldPuzzle(text=C.text_of(key))
    return _PUZZLES[key]


def _words(i):
    return (STATUS[i.status],) + tuple(i[1:])


def _check_store(handle, item, npad, device, ref, n=None):
    """The first ``n`` entries (default: all) of the store and the links of ``item`` against the restatement's."""
    n = len(ref.states) if n is None else n
    N = len(ref.states[0])
    pos = torch.full((n, npad, 2), 0x55, dtype=torch.int8, device=device)
    canon = torch.full((n, 2), 0x55, dtype=torch.int8, device=device)
    parent = torch.full((n,), -7, dtype=torch.int32, device=device)
    frm = torch.full((n, 2), 0x55, dtype=torch.int8, device=device)
    action = torch.full((n,), 0x55, dtype=torch.uint8, device=device)
    goal = torch.full((n,), 0x55, dtype=torch.uint8, device=device)
    handle.read_states(item, 0, n, pos, npad, canon)
    handle.read_links(item, 0, n, parent, frm, action, goal)
    pos = pos.cpu().numpy()
    assert (pos[:, :N] == np.asarray(ref.states[:n], np.int8)).all() and (pos[:, N:] == 0).all()
    assert (canon.cpu().numpy() == np.asarray(ref.canons[:n], np.int8)).all()
    links = ref.links[:n]
    assert parent.cpu().tolist() == [ln.parent for ln in links]
    assert [tuple(f) for f in frm.cpu().tolist()] == [tuple(ln.frm) for ln in links]
    assert action.cpu().tolist() == [ln.action for ln in links]
    assert goal.cpu().tolist() == [int(ln.goal) for ln in links]


def _check_batch_item(pb, i, ref, result, plan, pushes, verdict):
    """Item ``i`` of a ``PushPlanBatch`` run that was not cut short: info, store, links, push plan, primitive plan."""
    got, info, _ = result
    assert tuple(info) == _words(ref.info()), (i, tuple(info), _words(ref.info()))
    _check_store(pb.handle, i, pb.npad, pb.device, ref)
    if ref.status == "solved":
        want_plan, want_pushes = ref.plan()
        assert got == C.pushes_of(ref) and len(got) == want_pushes == pushes
        assert plan == want_plan and verdict == REPLAY_VALID
    else:
        assert got is None and plan is None and pushes == 0 and verdict == REPLAY_NONE


def _batch_results(pb):
    results = pb.results()
    plans, plan_len, pushes = (t.cpu().numpy() for t in pb.primitive_plans())
    verdict = pb.validate().cpu().tolist()
    plans = [plans[i, :plan_len[i]].tolist() if plan_len[i] >= 0 else None for i in range(len(results))]
    assert [p is None for p in plans] == [int(v) == REPLAY_NONE for v in plan_len]
    return results, plans, pushes.tolist(), verdict


# ---- 1. 6, 7 and 8 movables and the board 16 cells high among small puzzles: items of different N in one launch ----------------------
@pytest.mark.parametrize("order", (0, 1), ids=("largest-first", "largest-last"))
@pytest.mark.parametrize("k", C.KS)
def test_level1_items_of_different_n(k, order):
    names = C.ORDERS[order]
    with PushPlanBatch([_puzzle(n) for n in names], batch=k, max_states=C.MAX_STATES) as pb:
        assert pb.npad == 8
        pb.run(max_rounds=C.ROUNDS)
        results, plans, pushes, verdict = _batch_results(pb)
        for i, name in enumerate(names):
            ref = C.restated(C.Run(name, None, k, C.ROUNDS, None)).ref
            print(name, k, tuple(results[i][1]), _words(ref.info()))
            _check_batch_item(pb, i, ref, results[i], plans[i], pushes[i], verdict[i])


def test_live_items_of_different_n_reuse_slabs():
    """1 500 environments over the seven puzzles, more items than any device has workgroups, twice on one planner: a slab
    runs items of N = 3 .. 8 in turn, and every repeat of a puzzle gives its restatement's info and first push."""
    names = C.ORDERS[0]
    vec = VecPushWorld([_puzzle(n) for n in names], C.LIVE_ITEMS, observation=None, max_steps=None)
    assert vec.num_objects_padded == 8
    vec.reset()
    runs = []
    with vec.push_planner(batch=C.LIVE_K, max_states=C.LIVE_MAX_STATES) as planner:
        for _ in range(2):
            q = vec.planned_pushes(planner, max_rounds=C.LIVE_ROUNDS, push_cap=8)
            info = planner.info().cpu().numpy()[:, :10]
            out = [t.cpu().numpy() for t in (q.push_from, q.push_action, q.pushes) + tuple(planner._out[1:5])]
            results = planner.results()
            for i, name in enumerate(names):
                run = C.Run(name, None, C.LIVE_K, C.ROUNDS, None)
                want = C.after(run, C.LIVE_ROUNDS)
                assert want.states + 64 * C.LIVE_K < C.LIVE_MAX_STATES  # (no round came near the smaller store's limit)
                assert (info[i::len(names)] == np.asarray(_words(want))).all(), name
                for arr in out:
                    assert (arr[i::len(names)] == arr[i]).all(), name
                chain = C.pushes_of(C.restated(run).ref) if want.status == "solved" else None
                assert all(r[0] == chain for r in results[i::len(names)]), name
                first = (chain[0][0], chain[0][1], len(chain)) if chain else ((0, 0), PUSH_NONE, -1)
                assert (tuple(out[0][i].tolist()), int(out[1][i]), int(out[2][i])) == first, name
            runs.append([info] + out)
        assert all((a == b).all() for a, b in zip(*runs))  # the second call repeats the first


# ---- 2. random shapes on 16 x 16 frames: overlapping starts, coordinates of 15, queues of +inf and NaN keys --------------------------
def _shape_items():
    """(set index, case, start index or None, start state) per item: the 13 starts of every case, then its start outside the
    grid."""
    items = []
    for pid, case in enumerate(C.SHAPES):
        items += [(pid, case, s, state) for s, state in enumerate(C.shape_starts(case))]
        items.append((pid, case, None, C.outside_start(case)))
    return items


@pytest.mark.parametrize("k, rounds", [(k, C.SHAPE_ROUNDS) for k in C.KS] + [(C.SHAPE_COVER_K, C.SHAPE_COVER_ROUNDS)])
def test_shapes_at_the_size_limit(k, rounds):
    items = _shape_items()
    vec = VecPushWorld([_puzzle(c) for c in C.SHAPES], len(C.SHAPES), observation=None, max_steps=None)
    assert vec.num_objects_padded == 8 and len(items) == 56
    ids = torch.tensor([it[0] for it in items], dtype=torch.int32, device=vec.device)
    zero = np.zeros((len(items), 8, 2), np.int8)
    noisy = np.random.default_rng(24).integers(-128, 128, zero.shape).astype(np.int8)  # bytes beyond a puzzle's movables
    for e, (_, case, _, state) in enumerate(items):
        assert all(-128 <= v <= 127 for xy in state for v in xy)
        zero[e, :case[0]] = noisy[e, :case[0]] = np.asarray(state, np.int8)
    assert sum((noisy[e] != zero[e]).any() for e in range(len(items))) == 28  # every item of the puzzles with 6 and 7 movables
    outs = []
    with vec.push_planner(batch=k, max_states=C.MAX_STATES) as planner:
        for pos in (noisy, zero):
            q = planner.plan(ids, torch.as_tensor(pos).to(vec.device), max_rounds=rounds, push_cap=16)
            info = planner.info().cpu().numpy()[:, :10]
            outs.append([info] + [t.cpu().numpy() for t in (q.push_from, q.push_action, q.pushes) + tuple(planner._out[1:5])])
            if pos is zero:
                continue
            results = planner.results()
            verdict = planner.validate().cpu().tolist()
            plans, plan_len, _ = (t.cpu().numpy() for t in planner.primitive_plans())
            first_from, first_action, pushes = outs[0][1:4]
            for e, (pid, case, s, state) in enumerate(items):
                if s is None:  # a start outside its grid
                    assert not C.in_grid(case, state)
                    assert planner.info()[e].cpu().tolist() == SKIPPED and results[e][0] is None
                    assert (pushes[e], first_action[e], first_from[e].tolist()) == (-1, PUSH_NONE, [0, 0])
                    assert verdict[e] == REPLAY_SKIPPED  # (the replay's own range test of the start)
                    continue
                got = C.restated(C.Run(case, s, k, C.SHAPE_ROUNDS, None))
                want = C.after(C.Run(case, s, k, C.SHAPE_ROUNDS, None), rounds)
                assert tuple(info[e]) == _words(want), (case, s, tuple(info[e]), _words(want))
                _check_store(planner.handle, e, 8, vec.device, got.ref, want.states)
                if want.status == "solved":
                    chain = C.pushes_of(got.ref)
                    assert results[e][0] == chain and pushes[e] == len(chain) > 0
                    assert (tuple(first_from[e].tolist()), int(first_action[e])) == chain[0]
                    assert plans[e, :plan_len[e]].tolist() == got.ref.plan()[0] and verdict[e] == REPLAY_VALID
                else:
                    assert results[e][0] is None and verdict[e] == REPLAY_NONE
                    assert (pushes[e], first_action[e], first_from[e].tolist()) == (-1, PUSH_NONE, [0, 0])
    assert all((a == b).all() for a, b in zip(*outs))  # random bytes beyond the movables change nothing


# ---- 3. RGD budgets that overrun: NaN keys of overruns beside finite keys ---------------------------------------------------------
@pytest.mark.parametrize("budget", sorted({b for _, b in C.BUDGETS}))
def test_rgd_budget_overruns(budget):
    runs = [r for r in C.BUDGET_RUNS if r.budget == budget]
    with PushPlanBatch([_puzzle(r.puzzle) for r in runs], batch=C.BUDGET_K, max_states=C.MAX_STATES, rgd_budget=budget) as pb:
        pb.run(max_rounds=C.BUDGET_ROUNDS)
        results, plans, pushes, verdict = _batch_results(pb)
        for i, run in enumerate(runs):
            ref = C.restated(run).ref
            print(run.puzzle, budget, tuple(results[i][1]), _words(ref.info()))
            assert results[i][1].rgd_exceeded == ref.rgd_exceeded > 0
            _check_batch_item(pb, i, ref, results[i], plans[i], pushes[i], verdict[i])


# ---- 4. a goal state outside its grid whose offending movable is number 7 ---------------------------------------------------------------
def test_goal_state_outside_its_grid_with_8_movables():
    runs = (C.OUTSIDE8_RUN, C.OUTSIDE8_INSIDE_RUN)
    refs = [C.restated(r).ref for r in runs]
    cp, _ = C.oracles_of("outside8")
    assert not C.in_grid("outside8", refs[0].states[-1]) and refs[0].canons[-1] == (0, 0) and refs[0].status == "solved"
    pz = _puzzle("outside8")
    vec = VecPushWorld([pz], 2, observation=None, max_steps=None)
    assert vec.num_objects_padded == 8
    vec.reset()
    pos = vec.states()
    assert [tuple(xy) for xy in pos[1].tolist()] == [tuple(xy) for xy in cp.initial_state]
    pos[0] = np.asarray(C.OUTSIDE8_START, np.int8)
    vec.set_states(pos)
    with vec.push_planner(batch=2) as planner:
        q = vec.planned_pushes(planner, max_rounds=C.OUTSIDE8_INSIDE_RUN.rounds, push_cap=16)
        info = planner.info().cpu().numpy()
        results = planner.results()
        for e, ref in enumerate(refs):
            assert tuple(info[e, :10]) == _words(ref.info())
            assert results[e][0] == (C.pushes_of(ref) if ref.status == "solved" else None)
            _check_store(planner.handle, e, 8, vec.device, ref)
        assert (tuple(q.push_from[0].cpu().tolist()), int(q.push_action[0]), int(q.pushes[0])) == ((3, 3), 1, 1)
        assert planner.validate().cpu().tolist()[0] == REPLAY_VALID
    with PushBestFirstSearch(pz, batch=2) as bfs:  # and K17 on the device says the same
        bfs.begin(C.OUTSIDE8_START)
        assert tuple(bfs.run()) == tuple(info[0, :10])
        got_pos, got_canon = (t.cpu().numpy() for t in bfs.states())
        assert got_pos[:, :8].tolist() == [list(map(list, s)) for s in refs[0].states]
        assert got_canon.tolist() == [list(c) for c in refs[0].canons]


# ---- 5. push_cap ---------------------------------------------------------------------------------------------------------------------
PUSH_CAP_NAMES = ("Shape Of You", "Two Goals", "Shape Of You", "Two Goals")  # N = 8 and N = 3: plans of 8 and of 4 pushes
PUSH_CAP_K = 64
FILL = 0x55


def _plan_arrays(refs, cap, npad, fill):
    """(plan_len, plan_from, plan_action, plan_pos) as a run with ``push_cap`` = cap leaves buffers that held ``fill``."""
    n = len(refs)
    plan_len = np.zeros((n,), np.int32)
    plan_from = np.full((n, cap, 2), fill, np.int8)
    plan_action = np.full((n, cap), fill, np.uint8)
    plan_pos = np.full((n, cap, npad, 2), fill, np.int8)
    for i, ref in enumerate(refs):
        rows, index = [], ref.goal_index
        while ref.links[index].parent >= 0:
            ln = ref.links[index]
            rows.append((ln.frm, ln.action, ref.states[ln.parent]))
            index = ln.parent
        rows = rows[::-1]
        plan_len[i] = len(rows) if len(rows) <= cap else PUSH_PLAN_CUT
        if len(rows) <= cap:
            for t, (frm, action, state) in enumerate(rows):
                plan_from[i, t], plan_action[i, t], plan_pos[i, t] = frm, action, 0
                plan_pos[i, t, :len(state)] = np.asarray(state, np.int8)
    return plan_len, plan_from, plan_action, plan_pos


def test_push_cap_in_both_forms():
    refs = [C.restated(C.Run(n, None, PUSH_CAP_K, C.ROUNDS, None)).ref for n in PUSH_CAP_NAMES]
    chains = [C.pushes_of(ref) for ref in refs]
    lengths = [len(c) for c in chains]
    assert lengths == [8, 4, 8, 4] and all(ref.status == "solved" for ref in refs)
    words = [_words(ref.info()) for ref in refs]
    puzzles = [_puzzle(n) for n in PUSH_CAP_NAMES]
    caps = (8, 7, 4, 3)  # L and L - 1 of either plan
    with PushPlanBatch(puzzles, batch=PUSH_CAP_K, max_states=C.MAX_STATES) as pb:
        dev = pb.device
        for cap in caps:
            pb.run(max_rounds=C.ROUNDS, push_cap=cap)
            results = pb.results()
            plans, plan_len, pushes = (t.cpu().numpy() for t in pb.primitive_plans())
            verdict = pb.validate().cpu().tolist()
            for got, want in zip((t.cpu().numpy() for t in pb._out[1:]), _plan_arrays(refs, cap, pb.npad, 0)):
                assert np.array_equal(got, want), cap
            for i, ref in enumerate(refs):
                assert tuple(results[i][1]) == words[i]  # a cut plan's search is solved all the same
                if lengths[i] <= cap:
                    assert results[i][0] == chains[i] and pushes[i] == lengths[i] and verdict[i] == REPLAY_VALID
                    assert plans[i, :plan_len[i]].tolist() == ref.plan()[0]
                else:  # results: None; primitive_plans: no written plan
                    assert results[i][0] is None and plan_len[i] == REPLAY_NONE and pushes[i] == 0 and verdict[i] == REPLAY_NONE
            # the same run into buffers that hold a pattern: nothing is written past an item's plan or its push_cap
            info = torch.zeros((4, 11), dtype=torch.int64, device=dev)
            bufs = [torch.full((4,), FILL, dtype=torch.int32, device=dev), torch.full((4, cap, 2), FILL, dtype=torch.int8, device=dev),
                    torch.full((4, cap), FILL, dtype=torch.uint8, device=dev),
                    torch.full((4, cap, pb.npad, 2), FILL, dtype=torch.int8, device=dev)]
            pb.handle.run(C.ROUNDS, 0.0, info, *bufs, cap, pb.npad)
            assert [tuple(r) for r in info[:, :10].cpu().tolist()] == words
            for got, want in zip(bufs, _plan_arrays(refs, cap, pb.npad, FILL)):
                assert np.array_equal(got.cpu().numpy(), want), cap
    vec = VecPushWorld(puzzles[:2], 4, observation=None, max_steps=None)
    vec.reset()
    with vec.push_planner(batch=PUSH_CAP_K, max_states=C.MAX_STATES) as planner:
        for cap in caps + (0,):
            q = vec.planned_pushes(planner, max_rounds=C.ROUNDS, push_cap=cap)
            assert [tuple(r) for r in planner.info()[:, :10].cpu().tolist()] == words
            whole = [cap == 0 or n <= cap for n in lengths]  # (without plan arrays nothing is cut)
            assert q.pushes.cpu().tolist() == [n if w else PUSH_PLAN_CUT for n, w in zip(lengths, whole)]
            assert [tuple(f) for f in q.push_from.cpu().tolist()] == [c[0][0] if w else (0, 0) for c, w in zip(chains, whole)]
            assert q.push_action.cpu().tolist() == [c[0][1] if w else PUSH_NONE for c, w in zip(chains, whole)]
            if cap == 0:
                with pytest.raises(ValueError, match="kept no plans"):
                    planner.results()
                continue
            for got, want in zip((t.cpu().numpy() for t in planner._out[1:5]), _plan_arrays(refs, cap, 8, 0)):
                assert np.array_equal(got, want), cap
            results = planner.results()
            plans, plan_len, pushes = (t.cpu().numpy() for t in planner.primitive_plans())
            verdict = planner.validate().cpu().tolist()
            for i, ref in enumerate(refs):
                if whole[i]:
                    assert results[i][0] == chains[i] and pushes[i] == lengths[i] and verdict[i] == REPLAY_VALID
                    assert plans[i, :plan_len[i]].tolist() == ref.plan()[0]
                else:
                    assert results[i][0] is None and plan_len[i] == REPLAY_NONE and pushes[i] == 0 and verdict[i] == REPLAY_NONE


# ---- 6. the time limit -----------------------------------------------------------------------------------------------------------------
def test_time_limit():
    """A microsecond per item: every search ends `timeout` between two rounds, after r rounds (r is whatever the device's clock
    gives, possibly 0) that equal the restatement's first r.  One launch; nothing is timed or repeated here."""
    names = C.ORDERS[0]
    with PushPlanBatch([_puzzle(n) for n in names], batch=8, max_states=C.MAX_STATES) as pb:
        pb.run(max_rounds=C.ROUNDS, time_limit=1e-6)
        results = pb.results()
        plan_len = pb._out[1].cpu().tolist()
        for i, name in enumerate(names):
            run = C.Run(name, None, 8, C.ROUNDS, None)
            got, info, seconds = results[i]
            print(name, tuple(info), seconds)
            assert info.status == "timeout" and got is None and plan_len[i] == -1
            r = info.rounds
            assert 0 <= r < C.restated(run).infos[-1].rounds  # the limit did bite
            want = C.after(run, r)
            assert want.status == "running" and tuple(info)[1:] == _words(want)[1:]
            _check_store(pb.handle, i, pb.npad, pb.device, C.restated(run).ref, want.states)


# ---- 7. cost_range: the bucket bitmap's word boundaries ------------------------------------------------------------------------------
@pytest.mark.parametrize("cost_range", (None,) + C.RANGE_SAME)
def test_cost_ranges_that_hold_every_key(cost_range):
    ref = C.restated(C.RANGE_RUN).ref
    assert ref.largest_key == 25 and ref.status == "solved"
    with PushPlanBatch([_puzzle(C.RANGE_RUN.puzzle)], batch=C.RANGE_RUN.k, max_states=C.MAX_STATES, cost_range=cost_range) as pb:
        pb.run()
        results, plans, pushes, verdict = _batch_results(pb)
        _check_batch_item(pb, 0, ref, results[0], plans[0], pushes[0], verdict[0])


def test_cost_range_one_short():
    got = C.restated(C.RANGE_RUN)
    first = min(r for r, i in enumerate(got.infos) if i.largest_key >= C.RANGE_SHORT)  # the round that first pushes such a key
    with PushPlanBatch([_puzzle(C.RANGE_RUN.puzzle)], batch=C.RANGE_RUN.k, max_states=C.MAX_STATES, cost_range=C.RANGE_SHORT) as pb:
        pb.run()
        (plan, info, _), = pb.results()
        print(tuple(info), first)
        assert plan is None and info.status == "range" and info.goal_index == -1 and pb._out[1].cpu().tolist() == [-1]
        assert info.rounds <= first and info.largest_key < C.RANGE_SHORT
        _check_store(pb.handle, 0, pb.npad, pb.device, got.ref, info.states)  # what it stored is the restatement's store so far

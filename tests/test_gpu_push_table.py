"""Exact cost-to-go tables over pushes (pw_push_search_solve / pw_push_search_table_*, search.PushSolutionTable,
VecPushWorld.push_table / push_cost_to_go / push_expert_actions) against the plain-Python restatement of
tests/push_table_restatement.py, field by field; the query against the restatement and against the move-by-move table
(search.SolutionTable); the expert end to end in a VecPushWorld; `room3` (no CPU reference in a test's time) against pinned
figures, sampled rows and the Bellman equations recomputed with torch."""
import numpy as np
import pytest
import torch

import deep_puzzles
import push_table_restatement as TR
import walk_restatement as WR
from oracle import c_oracle
from pushworld_amd.puzzle import PushWorldPuzzle
from pushworld_amd.search import COST_UNKNOWN, PUSH_NONE, PushBreadthFirstSearch, PushQuery, PushSolutionTable, SolutionTable
from pushworld_amd.vec_env import VecPushWorld
from test_gpu_push_search import SEARCH_CASES, _pushing_steps, _with_bits

pytestmark = pytest.mark.gpu

_PZ = {}


def _puzzle(name):
    if name not in _PZ:
        _PZ[name] = PushWorldPuzzle(text=TR.case(name)[0])
    return _PZ[name]


def _arrays(tab):
    """(row_off, cost, best, succ, from, action, flags) of a table as numpy arrays."""
    succ, frm, action, flags = tab.rows()
    return tuple(t.cpu().numpy() for t in (tab.offsets(), tab.costs(), tab.best(), succ, frm, action, flags))


def _check_table(tab, cp, t):
    """Every field of every state and row against the restatement's; the store it sits on is the restatement's too."""
    S, R = t.info[0], t.info[1]
    assert tab.info == t.info and (tab.num_states, tab.num_rows) == (S, R)
    pos, canon = (x.cpu().numpy() for x in tab.states())
    N = cp.num_movables
    assert (pos[:, :N] == np.asarray(t.store.states, np.int8)).all() and (canon == np.asarray(t.store.canons, np.int8)).all()
    row_off, cost, best, succ, frm, action, flags = _arrays(tab)
    assert row_off.dtype == np.int64 and row_off.tolist() == t.row_off
    assert succ.dtype == np.int32 and succ.tolist() == t.succ
    assert frm.dtype == np.int8 and frm.shape == (R, 2) and [tuple(q) for q in frm.tolist()] == t.frm
    assert action.dtype == np.uint8 and action.tolist() == t.action
    assert flags.dtype == np.uint8 and flags.tolist() == t.flags
    assert cost.dtype == np.int32 and cost.tolist() == t.cost
    assert best.dtype == np.int32 and best.tolist() == t.best
    # a window in the middle reads the same values
    if S > 4:
        assert tab.offsets(2, 2).cpu().tolist() == t.row_off[2:5] and tab.costs(2, 2).cpu().tolist() == t.cost[2:4]
        assert tab.best(S - 1, 1).cpu().tolist() == t.best[S - 1:]
    if R > 4:
        w = tab.rows(1, 3)
        assert w[0].cpu().tolist() == t.succ[1:4] and w[3].cpu().tolist() == t.flags[1:4]


# ---- 1. field by field --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TR.EXPECT))
def test_field_by_field(name):
    _, cp, start, t = TR.case(name)
    assert TR.summary(cp, t) == TR.EXPECT[name]
    with PushSolutionTable(_puzzle(name), start=start) as tab:
        _check_table(tab, cp, t)


def test_big_many_passes():
    _, cp, _, t = TR.case("big")
    with PushSolutionTable(_puzzle("big"), chunk=7) as tab:
        _check_table(tab, cp, t)


def test_big_one_fingerprint_bit():
    """Almost every probe of the lookup meets an equal fingerprint: the exact comparison decides."""
    _, cp, _, t = TR.case("big")
    pz = _puzzle("big")

    def run():
        with PushSolutionTable(pz, chunk=7) as tab:
            _check_table(tab, cp, t)

    _with_bits(pz, 1, run)


@pytest.mark.parametrize("tables", ["all", "big", "none"])
@pytest.mark.parametrize("npad, index", [(4, 0), (8, 1), (16, 1), (32, 2)])
def test_big_padded(npad, index, tables):
    """`big` as puzzle `index` of a set padded to `npad` by puzzles with more movables, under the three forms of the step tables."""
    _, cp, _, t = TR.case("big")
    extra = {4: None, 8: 4, 16: 10, 32: deep_puzzles.POCKETS_EXTRA}[npad]
    texts = [deep_puzzles.pockets(extra)] * max(index, 1) if extra else []
    texts.insert(index, deep_puzzles.big())
    vec = VecPushWorld([PushWorldPuzzle(text=x) for x in texts], len(texts), observation=None, max_steps=None,
                       engine_options={"step_tables": tables})
    assert vec.num_objects_padded == npad
    with vec.push_table(index) as tab:
        _check_table(tab, cp, t)
        # the live states of the batch: the environment of `big` is at node 0, the others are left as they were
        vec.reset()
        q = vec.push_cost_to_go([tab])
        want = TR.query(cp, t, cp.initial_state)
        assert index in vec.puzzle_id.cpu().tolist()
        for e in range(vec.num_envs):
            got = _item(_host(q), e)
            assert got == (want if int(vec.puzzle_id[e]) == index else TR.NOT_IN_TABLE)


# ---- 2. solve's errors ----------------------------------------------------------------------------------------------------------
def test_solve_errors():
    pz = _puzzle("big")
    with PushBreadthFirstSearch(pz) as bfs:  # stop_at_goal
        assert bfs.solve() is not None
        with pytest.raises(ValueError, match="pw_push_search_solve.*stop"):
            bfs._handle.solve()
    with PushBreadthFirstSearch(pz, stop_at_goal=False) as bfs:
        with pytest.raises(ValueError, match="pw_push_search_solve.*begin"):
            bfs._handle.solve()
        bfs.begin()
        with pytest.raises(ValueError, match="pw_push_search_solve.*not exhausted"):
            bfs._handle.solve()
        bfs.expand()
        with pytest.raises(ValueError, match="pw_push_search_solve.*not exhausted"):
            bfs._handle.solve()
        assert bfs.solve() is None and bfs._handle.solve()[:2] == (1260, 6464)  # exhausted: the same handle solves
    with PushBreadthFirstSearch(pz, max_states=100, stop_at_goal=False) as bfs:
        with pytest.raises(ValueError, match="max_states"):
            bfs.solve()
        with pytest.raises(ValueError, match="pw_push_search_solve.*overflowed"):
            bfs._handle.solve()
    with pytest.raises(ValueError, match="max_states"):
        PushSolutionTable(pz, max_states=100)


def test_begin_discards_the_table():
    pz = _puzzle("big")
    with PushSolutionTable(pz) as tab:
        pos = torch.zeros((1, tab.npad, 2), dtype=torch.int8, device=tab.device)
        assert int(tab.costs(0, 1).cpu()[0]) == 6
        tab.search.begin()
        for call in (lambda: tab.costs(0, 1), lambda: tab.rows(0, 1), lambda: tab.query(None, pos)):
            with pytest.raises(ValueError, match="no table"):
                call()
        for bad in (lambda: tab.search._handle.table_read(-1, 1, None, None, None),):
            with pytest.raises(ValueError, match="out of bounds"):
                bad()
        while not tab.search.exhausted:  # and the handle solves again
            tab.search.expand()
        assert tab.search._handle.solve() == tab.info and int(tab.costs(0, 1).cpu()[0]) == 6
        with pytest.raises(ValueError, match="out of bounds"):
            tab.costs(1259, 2)
        with pytest.raises(ValueError, match="out of bounds"):
            tab.rows(6464, 1)
        assert tab.rows(6464, 0)[0].numel() == 0 and tab.offsets(1260, 0).cpu().tolist() == [6464]


# ---- 3. the query against the restatement ---------------------------------------------------------------------------------------
def _item(q, i):
    return TR.Query(int(q.index[i]), int(q.cost[i]), int(q.action[i]), tuple(int(v) for v in q.push_from[i]), int(q.push_action[i]),
                    int(q.walk[i]))


def _host(q):
    return PushQuery(*(x.cpu().numpy() for x in q))


def _pos(states, npad, device):
    pos = np.zeros((len(states), npad, 2), np.int8)
    for i, s in enumerate(states):
        pos[i, :len(s)] = np.asarray(s, np.int64).astype(np.int8)
    return torch.as_tensor(pos, device=device)


_MOVES = {}


def _big_moves():
    """Every state the move-by-move search reaches on `big` and its table of costs in moves: computed once, never changed."""
    if not _MOVES:
        with_table = SolutionTable(_puzzle("big"), max_states=1 << 16)
        _MOVES["states"] = np.ascontiguousarray(with_table.states().astype(np.int8))
        _MOVES["cost"] = with_table.costs().cpu().numpy().astype(np.int64)
        with_table.close()
    return _MOVES["states"], _MOVES["cost"]


def test_query_against_the_restatement():
    _, cp, _, t = TR.case("big")
    states, _ = _big_moves()
    assert states.shape == (42832, 3, 2)
    live = [tuple(tuple(int(v) for v in xy) for xy in s) for s in states[::97]]
    goal = next(i for i in range(t.info[0]) if t.cost[i] == 0)
    outside = ((0, 0), (9, 2), (3, 3))
    # the items after the sampled states: masked, an id outside the set, a movable outside its grid, a goal state, a dead end
    dead = next(i for i in range(t.info[0]) if t.cost[i] == -1)
    extra = [live[0], live[1], outside, t.store.states[goal], t.store.states[dead]]
    with PushSolutionTable(_puzzle("big")) as tab:
        n = len(live) + len(extra)
        pos = _pos(live + extra, tab.npad, tab.device)
        ids = torch.zeros(n, dtype=torch.int32, device=tab.device)
        mask = torch.ones(n, dtype=torch.uint8, device=tab.device)
        mask[len(live)] = 0
        ids[len(live) + 1] = 5
        fill = PushQuery(*(torch.full_like(x, 77) for x in tab.query(ids, pos)))  # what the skipped items must keep
        q = _host(tab.query(ids, pos, mask=mask, out=fill))
        for i, s in enumerate(live):
            assert _item(q, i) == TR.query(cp, t, s), i
        kept = TR.Query(77, 77, 77, (77, 77), 77, 77)
        k = len(live)
        assert _item(q, k) == kept and _item(q, k + 1) == kept
        assert _item(q, k + 2) == TR.NOT_IN_TABLE == TR.query(cp, t, outside)
        assert _item(q, k + 3) == TR.Query(goal, 0, -1, (0, 0), PUSH_NONE, -1) == TR.query(cp, t, extra[3])
        assert _item(q, k + 4) == TR.Query(dead, -1, -1, (0, 0), PUSH_NONE, -1) == TR.query(cp, t, extra[4])
        assert len({_item(q, i).index for i in range(len(live))}) > 100 and any(_item(q, i).walk > 3 for i in range(len(live)))
        # without puzzle_id and mask; without the maps: the same index and cost, action and walk left as they were
        q2 = _host(tab.query(None, pos[:k]))
        assert all(_item(q2, i) == _item(q, i) for i in range(k))
        q3 = _host(tab.query(None, pos[:k], actions=False))
        assert (q3.index == q2.index).all() and (q3.cost == q2.cost).all() and (q3.push_from == q2.push_from).all()
        assert (q3.push_action == q2.push_action).all() and (q3.action == -1).all() and (q3.walk == -1).all()
        # the wrapper's checks
        with pytest.raises(ValueError, match="pos must be"):
            tab.query(None, pos[:, :2])
        with pytest.raises(ValueError, match="PushQuery of an earlier query"):
            tab.query(None, pos, out=(q.index,))


def test_query_of_states_that_cannot_be_reached():
    """A table from the last state of `big`'s store -- a goal state with its boxes in corners: one state, no rows.  The puzzle's
    initial state cannot be reached from it: -1 / -2."""
    _, cp, _, t = TR.case("big")
    start = t.store.states[1259]
    t2 = TR.build(cp, start=start)
    assert TR.query(cp, t2, cp.initial_state) == TR.NOT_IN_TABLE
    with PushSolutionTable(_puzzle("big"), start=start) as tab:
        _check_table(tab, cp, t2)
        q = _host(tab.query(None, _pos([cp.initial_state, start], tab.npad, tab.device)))
        assert _item(q, 0) == TR.NOT_IN_TABLE and _item(q, 1) == TR.query(cp, t2, start)
        assert tab.optimal_plan() == ([] if t2.cost[0] == 0 else None)


def test_query_of_overlapping_live_states():
    """The successors of listed state 30 of (8, 16, 2): overlapping states, some with a movable outside the grid."""
    name = "shape (8, 16, 2) listed 30"
    _, cp, start, t = TR.case(name)
    live = [pm.next_state for pm in WR.region(cp, start).pushes] + [start]
    assert any(not WR.in_grid(cp, s) for s in live) and sum(WR.in_grid(cp, s) for s in live) > 5
    with PushSolutionTable(_puzzle(name), start=start) as tab:
        q = _host(tab.query(None, _pos(live, tab.npad, tab.device)))
        for i, s in enumerate(live):
            assert _item(q, i) == TR.query(cp, t, s), i


def test_mixed_batch_of_two_tables():
    names = ["big", "serpentine 14x13 overshoot"]
    cases = [TR.case(k) for k in names]
    B = 96
    vec = VecPushWorld([PushWorldPuzzle(text=c[0]) for c in cases], B, observation=None, max_steps=None, seed=3)
    vec.reset()
    rng = np.random.default_rng(11)
    for _ in range(14):  # a walk of random actions: live states all over both spaces
        vec.step(torch.as_tensor(rng.integers(0, 4, B).astype(np.uint8), device=vec.device))
    ids = vec.puzzle_id.cpu().numpy()
    assert set(ids.tolist()) == {0, 1}
    with vec.push_table(0) as t0, vec.push_table(1) as t1:
        q = _host(vec.push_cost_to_go([t0, t1]))
        only0 = _host(vec.push_cost_to_go([t0]))
        acts = vec.push_expert_actions([t0, t1]).cpu().numpy()
        pos = vec.states()
        for e in range(B):
            _, cp, _, t = cases[ids[e]]
            live = tuple(tuple(int(v) for v in xy) for xy in pos[e, :cp.num_movables])
            want = TR.query(cp, t, live)
            assert _item(q, e) == want and acts[e] == want.action
            assert _item(only0, e) == (want if ids[e] == 0 else TR.NOT_IN_TABLE)
        assert len({_item(q, e).index for e in range(B)}) > 10
        with PushSolutionTable(_puzzle("big")) as foreign:
            with pytest.raises(ValueError, match="made on this environment"):
                vec.push_cost_to_go([foreign])


# ---- 4. the query against the table in moves ---------------------------------------------------------------------------------------
def test_query_against_the_move_table():
    states, moves = _big_moves()
    with PushSolutionTable(_puzzle("big")) as tab:
        pos = torch.zeros((states.shape[0], tab.npad, 2), dtype=torch.int8, device=tab.device)
        pos[:, :3] = torch.as_tensor(states, device=tab.device)
        q = _host(tab.query(None, pos))
    dead = moves == 0xFFFF
    assert int(dead.sum()) == deep_puzzles.EXPECT["big"][2] == 14444
    assert ((q.cost == -1) == dead).all()
    assert ((q.cost == 0) == (moves == 0)).all()
    assert (q.cost[~dead] <= moves[~dead]).all()
    assert (q.cost != COST_UNKNOWN).all() and (q.index >= 0).all()
    assert ((q.action >= 0) == (q.cost > 0)).all() and ((q.walk >= 0) == (q.cost > 0)).all()


# ---- 5. the expert, end to end -----------------------------------------------------------------------------------------------------
def test_expert_end_to_end():
    states, _ = _big_moves()
    B = states.shape[0]
    pz = _puzzle("big")
    vec = VecPushWorld([pz], B, observation=None, max_steps=None)
    vec.reset()
    vec.pos[:, :3].copy_(torch.as_tensor(states, device=vec.device))
    goal = torch.as_tensor(np.asarray(pz.goal_state, np.int8), device=vec.device)
    with vec.push_table(0) as tab:
        cost = vec.push_cost_to_go([tab]).cost.clone()
        steps = torch.zeros(B, dtype=torch.int32, device=vec.device)
        pushes = torch.zeros(B, dtype=torch.int32, device=vec.device)
        never = cost <= 0  # dead ones and goal ones: -1 throughout
        for _ in range(8 * 36):
            a = vec.push_expert_actions([tab])
            assert bool((a[never] == -1).all())
            acting = a >= 0
            if not bool(acting.any()):
                break
            before = vec.pos.clone()
            vec.step(a.to(torch.uint8))  # (255: not an action, the environment is left untouched)
            steps += acting
            pushes += (vec.pos[:, 1:3] != before[:, 1:3]).any(dim=2).any(dim=1)
            assert bool((vec.pos[~acting] == before[~acting]).all())
        assert not bool((vec.push_expert_actions([tab]) >= 0).any())
        live = cost > 0
        assert int(live.sum()) == B - 14444 - int((cost == 0).sum())
        assert bool((vec.pos[live, 1] == goal[0]).all())
        assert bool((pushes[live] == cost[live]).all()) and bool((steps[live] <= cost[live] * 36).all())
        assert bool((steps[~live] == 0).all())


# ---- 6. room3 -------------------------------------------------------------------------------------------------------------------
def test_room3():
    text = deep_puzzles.room3()
    cp = c_oracle.COraclePuzzle(text)
    with PushSolutionTable(PushWorldPuzzle(text=text), max_states=1 << 16) as tab:
        assert tab.info == (42840, 316176, 1190, 15778, 10)
        S, R = tab.num_states, tab.num_rows
        dev = tab.device
        pos, canon = tab.states()
        goal = tab.search.links()[4].to(torch.int64)
        row_off, cost, best = tab.offsets(), tab.costs().to(torch.int64), tab.best().to(torch.int64)
        succ, frm, action, flags = tab.rows()
        assert int(cost[0]) == 6 and int(row_off[-1]) == R
        # the rows of every 40th state against the restatement: succ through a dictionary over the store's packed canonical states
        hpos, hcanon = pos.cpu().numpy(), canon.cpu().numpy()
        index = {(tuple(hcanon[i].tolist()),) + tuple(map(tuple, hpos[i, 1:4].tolist())): i for i in range(S)}
        assert len(index) == S
        hoff, hsucc, hfrm, hact, hflags = (x.cpu().numpy() for x in (row_off, succ, frm, action, flags))
        for i in range(0, S, 40):
            state = tuple(map(tuple, hpos[i, :4].tolist()))
            rows = WR.region(cp, state).pushes
            lo, hi = int(hoff[i]), int(hoff[i + 1])
            assert hi - lo == len(rows)
            assert [tuple(q) for q in hfrm[lo:hi].tolist()] == [pm.frm for pm in rows]
            assert hact[lo:hi].tolist() == [pm.action for pm in rows]
            assert (hflags[lo:hi] & 1).tolist() == [int(pm.goal) for pm in rows]
            assert hsucc[lo:hi].tolist() == [index[WR.canon(cp, pm.next_state)] for pm in rows]
        # the Bellman equations for every state and row, recomputed from the arrays read back: independent of the sweeps
        INF = 1 << 40
        succ = succ.to(torch.int64)
        assert bool(((succ >= 0) & (succ < S)).all())  # (no overlaps here: no row leaves the grid)
        npush = row_off[1:] - row_off[:-1]
        row_state = torch.repeat_interleave(torch.arange(S, device=dev), npush)
        cs = cost[succ]
        c = torch.where((flags & 1) != 0, torch.zeros_like(cs), torch.where(cs >= 0, cs, torch.full_like(cs, INF)))
        least = torch.full((S,), INF, dtype=torch.int64, device=dev).scatter_reduce(0, row_state, c, "amin")
        want = torch.where(goal != 0, torch.zeros_like(least), torch.where(least >= INF, torch.full_like(least, -1), least + 1))
        assert torch.equal(cost, want)
        mine = cost[row_state]
        optimal = (mine > 0) & (c == mine - 1)
        k = torch.arange(R, device=dev) - row_off[row_state]
        first = torch.full((S,), INF, dtype=torch.int64, device=dev).scatter_reduce(0, row_state[optimal], k[optimal], "amin")
        assert torch.equal(best, torch.where(first >= INF, torch.full_like(first, -1), first))
        bits = ((flags & 1) != 0).to(torch.uint8) | (optimal.to(torch.uint8) << 1) | ((c < INF).to(torch.uint8) << 2)
        assert torch.equal(flags, bits)
        assert (int((cost == 0).sum()), int((cost == -1).sum()), int(cost.max())) == tab.info[2:]
        plan = tab.optimal_plan()
        got, goals = tab.search._engine.plan_states(0, bytes(plan))
        assert goals[-1] == 1 and _pushing_steps(got) == 6


# ---- 7. optimal_plan ------------------------------------------------------------------------------------------------------------
def test_optimal_plan():
    for pz in (_puzzle("big"), PushWorldPuzzle(text=SEARCH_CASES["2 Obstacle"]())):
        with PushSolutionTable(pz) as tab:
            plan = tab.optimal_plan()
            c0 = int(tab.costs(0, 1).cpu()[0])
            assert c0 > 0 and pz.is_valid_plan(plan)
            got, goals = pz._engine().plan_states(0, bytes(plan))
            assert goals[-1] == 1 and not goals[:-1].any() and _pushing_steps(got) == c0
            with PushBreadthFirstSearch(pz) as bfs:  # the fewest pushes: the breadth-first search's
                bfs.solve()
                assert bfs.pushes == c0
    name = "shape (8, 16, 2) listed 30"
    _, cp, start, t = TR.case(name)
    with PushSolutionTable(_puzzle(name), start=start) as tab:
        plan = tab.optimal_plan()
        got, goals = _puzzle(name)._engine().plan_states(0, bytes(plan), start=np.ascontiguousarray(np.asarray(start, np.int8)))
        assert goals[-1] == 1 and _pushing_steps(got) == t.cost[0] == 1
        with pytest.raises(ValueError, match="one .x, y. pair per movable"):
            tab.optimal_plan(start[:-1])
    name = "shape (3, 12, 9) search start 3"
    _, cp, start, t = TR.case(name)
    assert t.cost[0] == -1
    with PushSolutionTable(_puzzle(name), start=start) as tab:
        assert tab.optimal_plan() is None and tab.info == t.info

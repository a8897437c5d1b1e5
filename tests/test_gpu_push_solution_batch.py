"""Cost-to-go tables over pushes of many small puzzles in one launch (pw_push_solve_batch_*, search.PushSolutionTableBatch,
VecPushWorld.push_tables / push_cost_to_go), compared BY STATE (tests/push_solution_batch_restatement.py) against
the plain-Python restatement of tests/push_table_restatement.py and against search.PushSolutionTable: the restated cases in one
launch, puzzles beyond the kernel's limits, the one-launch query, the caps and the pools, the ladder of the closed set (`room3`),
a mix of generated puzzles, the expert in pushes end to end, and a captured query."""
import numpy as np
import pytest
import torch

import deep_puzzles
import push_solution_batch_restatement as BR
import push_table_restatement as PT
import shape_states as SS
import walk_restatement as WR
from oracle import c_oracle
from pushworld_amd import generate
from pushworld_amd._capi import PUSH_DONE, PUSH_REFUSED
from pushworld_amd.puzzle import PushWorldPuzzle
from pushworld_amd.search import (TABLE_BUILT, TABLE_NOT_SEARCHED, TABLE_SUMMARY_ONLY, TABLE_TOO_MANY, PushQuery,
                                  PushSolutionTableBatch)
from pushworld_amd.vec_env import VecPushWorld

pytestmark = pytest.mark.gpu

# the restated cases of one set at NP 4: the (3, 12, 9) shape puzzle is listed twice, with two starts (the second overlaps)
NAMES = ["big", "corridor 7", "serpentine 14x14", "serpentine 14x13 overshoot", "shape (3, 12, 9) deep goal start",
         "shape (3, 12, 9) search start 3"]
PUZZLES = [0, 1, 2, 3, 4, 4]
_SHARED = {}


def _cases_vec():
    """One environment over the five puzzles of the cases; made once."""
    if "vec" not in _SHARED:
        texts = [PT.case(name)[0] for name in NAMES[:5]]
        assert PT.case(NAMES[5])[0] == texts[4]
        vec = VecPushWorld([PushWorldPuzzle(text=x) for x in texts], 8, observation=None, max_steps=None)
        assert vec.num_objects_padded == 4
        _SHARED["vec"] = vec
    return _SHARED["vec"]


def _starts():
    return [PT.case(name)[2] for name in NAMES]


def _want(name):
    """The restated table of a case as arrays; computed once and never changed."""
    key = ("arrays", name)
    if key not in _SHARED:
        _SHARED[key] = BR.of_restated(PT.case(name)[3])
    return _SHARED[key]


def _summary(batch):
    return [tuple(row) for row in batch.summary.cpu().numpy().tolist()]


def _check_item(batch, item, name):
    got = BR.of_batch(batch, item)
    m = BR.compare(got, _want(name))
    E = PT.EXPECT[name]
    assert BR.summary_of(got) == E
    assert _summary(batch)[item] == (E[0], E[1], E[4], E[5], E[6], E[7])
    return m


# ---- 1. the restated cases in one launch ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("groups_per_cu", [1, 8])
def test_restated_cases_in_one_launch(groups_per_cu):
    vec = _cases_vec()
    vec.engine.set_option("search_batch_groups_per_cu", groups_per_cu)
    try:
        with vec.push_tables(PUZZLES, starts=_starts(), max_states_each=2048) as batch:
            assert len(batch) == 6 and batch.status.cpu().tolist() == [TABLE_BUILT] * 6 and batch.missing == 0
            assert batch.states_needed == batch.pool_states == sum(PT.EXPECT[n][0] + 1 for n in NAMES)
            assert batch.rows_needed == batch.pool_rows == sum(PT.EXPECT[n][1] for n in NAMES)
            for item, name in enumerate(NAMES):
                _check_item(batch, item, name)
            assert batch.num_states.cpu().tolist() == [PT.EXPECT[n][0] for n in NAMES]
            assert batch.start_cost.cpu().tolist() == [PT.EXPECT[n][7] for n in NAMES]
            # the overlapping starts: rows that leave the grid, every state dead
            succ = batch.rows(5)[0].cpu().numpy()
            assert int((succ < 0).sum()) == 24 and (batch.costs(5).cpu().numpy() == -1).all()
    finally:
        vec.engine.set_option("search_batch_groups_per_cu", 0)


# ---- 2. beyond the limits --------------------------------------------------------------------------------------------------------------
def test_beyond_the_limits():
    """17 movables (the set pads to 32) and an 18-wide grid get status 3; the others are what they are alone.  The bytes of `pos`
    beyond a puzzle's movables are random."""
    wide = SS.CASES[2]
    texts = [deep_puzzles.pockets(), SS.text(wide), deep_puzzles.big(), deep_puzzles.corridor(7)]
    vec = VecPushWorld([PushWorldPuzzle(text=x) for x in texts], 4, observation=None, max_steps=None)
    assert vec.num_objects_padded == 32
    with vec.push_tables(max_states_each=2048) as batch:
        assert batch.status.cpu().tolist() == [TABLE_NOT_SEARCHED, TABLE_NOT_SEARCHED, TABLE_BUILT, TABLE_BUILT]
        assert batch.state_offset.cpu().tolist()[:2] == [-1, -1] and batch.row_offset.cpu().tolist()[:2] == [-1, -1]
        _check_item(batch, 2, "big")
        _check_item(batch, 3, "corridor 7")
        with pytest.raises(ValueError, match="no stored table"):
            batch.costs(0)
        # the query: the first N movables only
        rng = np.random.default_rng(5)
        _, cp, _, t = PT.case("big")
        m = BR.state_map(BR.of_batch(batch, 2), _want("big"))
        live = t.store.states[::41]
        pos = rng.integers(-128, 128, (len(live) + 2, 32, 2)).astype(np.int8)
        for i, s in enumerate(live):
            pos[i, :3] = np.asarray(s, np.int8)
        ids = torch.full((len(pos),), 2, dtype=torch.int32, device=vec.device)
        ids[-2], ids[-1] = 0, 1  # puzzles without a table: untouched
        fill = PushQuery(*(torch.full_like(x, 77) for x in batch.query(ids, torch.as_tensor(pos, device=vec.device))))
        q = _host(batch.query(ids, torch.as_tensor(pos, device=vec.device), out=fill))
        for i, s in enumerate(live):
            assert _item(q, i, m) == PT.query(cp, t, s)
        assert _item(q, len(live)) == KEPT and _item(q, len(live) + 1) == KEPT
        # npad below the set's 17 movables: PW_EINVAL before any launch, from the query and from a run with starts
        from pushworld_amd import _capi

        dpos = torch.as_tensor(pos, device=vec.device)
        for npad in (4, 8, 16):
            rc = _capi.lib.pw_push_solve_batch_query(batch.handle, _capi._ptr(ids), _capi._ptr(dpos), npad, None, 1, None, None,
                                                     None, None, None, None, None)
            assert rc == _capi.PW_EINVAL and "pw_push_solve_batch_query: npad is smaller" in _capi.last_error()
            rc = _capi.lib.pw_push_solve_batch_run(batch.handle, None, _capi._ptr(dpos), npad, 1, 64, None)
            assert rc == _capi.PW_EINVAL and "pw_push_solve_batch_run: npad is smaller" in _capi.last_error()
        assert batch.status.cpu().tolist()[2:] == [TABLE_BUILT, TABLE_BUILT]  # (the refused run left the last one as it was)


# ---- 3. the query ------------------------------------------------------------------------------------------------------------------------
KEPT = PT.Query(77, 77, 77, (77, 77), 77, 77)


def _host(q):
    return PushQuery(*(x.cpu().numpy() for x in q))


def _item(q, i, m=None):
    """Item i of a query in the restatement's terms: its index through the state map ``m`` (device state -> restated state)."""
    idx = int(q.index[i])
    if m is not None and idx >= 0:
        idx = int(m[idx])
    return PT.Query(idx, int(q.cost[i]), int(q.action[i]), tuple(int(v) for v in q.push_from[i]), int(q.push_action[i]), int(q.walk[i]))


def _pos(states, npad, device, rng):
    """The states as rows of the engine's layout; whatever lies beyond a state's movables is random."""
    pos = rng.integers(-128, 128, (len(states), npad, 2)).astype(np.int8)
    for i, s in enumerate(states):
        pos[i, :len(s)] = np.asarray(s, np.int64).astype(np.int8)
    return torch.as_tensor(pos, device=device)


def _live_states(cp, t, other, rng):
    """Live states of a case: every stored state as reached, the same boxes with the agent on other cells of the region, the
    stored states of `other` (the same puzzle from another start: mostly not in this table), a coordinate outside the grid."""
    live = [tuple(map(tuple, s)) for s in t.store.states]
    for s in live[::max(1, len(live) // 40)]:
        cells = sorted(WR.region(cp, s).dist)
        for k in rng.choice(len(cells), size=min(3, len(cells)), replace=False):
            live.append((cells[int(k)],) + s[1:])
    if other is not None:
        live += [tuple(map(tuple, s)) for s in other.store.states[::max(1, len(other.store.states) // 40)]]
    s = live[0]
    live.append(s[:-1] + ((cp.width, s[-1][1]),))
    live.append(s[:-1] + ((s[-1][0], -1),))
    live.append(((-3, s[0][1]),) + s[1:])
    return live


@pytest.mark.parametrize("case", range(6))
def test_query(case):
    vec = _cases_vec()
    name = NAMES[case]
    _, cp, start, t = PT.case(name)
    other = PT.case(NAMES[9 - case])[3] if case >= 4 else None
    rng = np.random.default_rng(100 + case)
    live = _live_states(cp, t, other, rng)
    want = [PT.query(cp, t, s) for s in live]
    assert sum(w == PT.NOT_IN_TABLE for w in want) >= 3 and sum(w.index >= 0 for w in want) >= t.info[0]
    if case >= 4:
        assert sum(w == PT.NOT_IN_TABLE for w in want) > 5
    n = len(live)
    # after the live states: a masked item, an id outside the set (two ways), a puzzle of the set without a table here
    extra = 4
    pos = _pos(live + [live[0]] * extra, 4, vec.device, rng)
    ids = torch.full((n + extra,), PUZZLES[case], dtype=torch.int32, device=vec.device)
    mask = torch.ones(n + extra, dtype=torch.uint8, device=vec.device)
    mask[n] = 0
    ids[n + 1], ids[n + 2], ids[n + 3] = 99, -1, (PUZZLES[case] + 1) % 5
    with vec.push_tables([PUZZLES[case]], starts=[start], max_states_each=2048) as batch:
        assert batch.status.cpu().tolist() == [TABLE_BUILT]
        m = BR.state_map(BR.of_batch(batch, 0), _want(name))
        fill = PushQuery(*(torch.full_like(x, 77) for x in batch.query(ids, pos)))
        q = _host(batch.query(ids, pos, mask=mask, out=fill))
        for i in range(n):
            assert _item(q, i, m) == want[i], (i, live[i])
        for i in range(n, n + extra):
            assert _item(q, i) == KEPT
        assert any(w.walk > 3 for w in want) or name not in ("big", "serpentine 14x14")
        # without walk and action (NULL pointers): the other four outputs are the same, these two are left as they were
        fill = PushQuery(*(torch.full_like(x, 77) for x in fill))
        q2 = _host(batch.query(ids, pos, mask=mask, out=fill, actions=False))
        assert (q2.index == q.index).all() and (q2.cost == q.cost).all() and (q2.push_from == q.push_from).all()
        assert (q2.push_action == q.push_action).all() and (q2.action == 77).all() and (q2.walk == 77).all()
        # npad below the set's movables is refused before any launch
        with pytest.raises(ValueError, match="pos must be"):
            batch.query(ids, pos[:, :2].contiguous())


def test_serpentine_walks_are_long():
    """The 16 x 16 limit: the best push of the serpentine's start is about a hundred cells away."""
    vec = _cases_vec()
    _, cp, _, t = PT.case("serpentine 14x14")
    want = PT.query(cp, t, cp.initial_state)
    assert want.walk > 90
    with vec.push_tables([2], max_states_each=64) as batch:
        ids = torch.full((1,), 2, dtype=torch.int32, device=vec.device)
        q = _host(batch.query(ids, _pos([cp.initial_state], 4, vec.device, np.random.default_rng(0))))
        assert _item(q, 0) == want


# ---- 4. the caps and the pools ------------------------------------------------------------------------------------------------------------
def test_caps_and_pools():
    vec = _cases_vec()
    S, R = PT.EXPECT["big"][:2]
    E = PT.EXPECT["big"]
    with vec.push_tables([0], max_states_each=S - 1) as batch:
        assert batch.status.cpu().tolist() == [TABLE_TOO_MANY] and batch.states_needed == 0 and batch.rows_needed == 0
        ids = torch.zeros(1, dtype=torch.int32, device=vec.device)
        q = batch.query(ids, vec.pos[:1].contiguous())
        assert int(q.index[0]) == -1 and int(q.cost[0]) == -2  # no stored table: untouched
    with vec.push_tables([0], max_states_each=S) as batch:
        assert batch.status.cpu().tolist() == [TABLE_BUILT]
        _check_item(batch, 0, "big")
    # pools one short: the summary is valid, nothing is stored
    for states, rows in ((S, R), (S + 1, R - 1)):
        with vec.push_tables([0, 1], max_states_each=2048, states=states, rows=rows) as batch:
            status = batch.status.cpu().tolist()
            assert sorted(status) == [TABLE_BUILT, TABLE_SUMMARY_ONLY] or status == [TABLE_SUMMARY_ONLY] * 2
            assert status[0] == TABLE_SUMMARY_ONLY  # (the three states of the corridor fit whichever comes first)
            assert _summary(batch)[0] == (E[0], E[1], E[4], E[5], E[6], E[7])
            assert batch.state_offset.cpu().tolist()[0] == -1 and batch.row_offset.cpu().tolist()[0] == -1
            assert (batch.states_needed, batch.rows_needed) == (S + 1 + 4, R + 2)
            with pytest.raises(ValueError, match="no stored table"):
                batch.keys(0)
    # a summary-only run sizes a storing run that leaves nothing out
    with PushSolutionTableBatch(vec, PUZZLES, starts=_starts(), max_states_each=2048, states=0, rows=0) as dry:
        assert dry.status.cpu().tolist() == [TABLE_SUMMARY_ONLY] * 6
        assert _summary(dry) == [(PT.EXPECT[n][0], PT.EXPECT[n][1], PT.EXPECT[n][4], PT.EXPECT[n][5], PT.EXPECT[n][6],
                                  PT.EXPECT[n][7]) for n in NAMES]
        need = (dry.states_needed, dry.rows_needed)
    with PushSolutionTableBatch(vec, PUZZLES, starts=_starts(), max_states_each=2048, states=need[0], rows=need[1]) as full:
        assert full.status.cpu().tolist() == [TABLE_BUILT] * 6 and (full.states_needed, full.rows_needed) == need
        _check_item(full, 5, NAMES[5])
    # a start outside its grid: status 3
    bad = ((1, 1), (cp_width("corridor 7"), 1))
    with vec.push_tables([1, 1], starts=[bad, None], max_states_each=64) as batch:
        assert batch.status.cpu().tolist() == [TABLE_NOT_SEARCHED, TABLE_BUILT]


def cp_width(name):
    return PT.case(name)[1].width


# ---- 5. the ladder ---------------------------------------------------------------------------------------------------------------------
def test_room3_leaves_lds():
    """42 840 canonical states and 316 176 rows in one workgroup: the closed set climbs from LDS to 2^16 and 2^20 slots."""
    pz = PushWorldPuzzle(text=deep_puzzles.room3())
    vec = VecPushWorld([pz], 1, observation=None, max_steps=None)
    with vec.push_table(0, max_states=1 << 16) as tab:
        assert tab.info == (42840, 316176, 1190, 15778, 10)
        want = BR.of_table(tab, 4)
    with vec.push_tables(max_states_each=1 << 16) as batch:
        assert batch.status.cpu().tolist() == [TABLE_BUILT]
        assert _summary(batch) == [(42840, 316176, 1190, 15778, 10, 6)]
        BR.compare(BR.of_batch(batch, 0), want)


# ---- 6. a mix of generated puzzles -----------------------------------------------------------------------------------------------------
MIX, MIX_CAP = 32, 2048
RESTATED = (0, 2, 10, 13, 23)  # at most 65 canonical states each


def _mix():
    """The environment over 32 host-generated Level-0 puzzles, its batch and the per-puzzle references; made once."""
    if "mix" not in _SHARED:
        g, d = generate.generate_level0_grids(MIX, random_seed=21, device=-1)
        texts = [generate.grid_to_text(g[i], d[i, 0], d[i, 1]) for i in range(MIX)]
        vec = VecPushWorld([PushWorldPuzzle(text=x) for x in texts], 256, observation=None, max_steps=None, seed=4)
        batch = vec.push_tables(max_states_each=MIX_CAP)
        refs = []
        for i in range(MIX):
            try:
                with vec.push_table(i, max_states=MIX_CAP) as tab:
                    refs.append(BR.of_table(tab, int(vec.pset.headers()[320 * i + 6])))
            except ValueError as e:
                assert "max_states" in str(e) or "full" in str(e)
                refs.append(None)
        _SHARED["mix"] = (texts, vec, batch, refs)
    return _SHARED["mix"]


def test_generated_mix():
    texts, vec, batch, refs = _mix()
    status = batch.status.cpu().tolist()
    assert status == [TABLE_BUILT if r is not None else TABLE_TOO_MANY for r in refs]
    assert sum(r is not None for r in refs) >= 24
    for i, ref in enumerate(refs):
        if ref is not None:
            got = BR.of_batch(batch, i)
            BR.compare(got, ref)
            assert _summary(batch)[i] == tuple(BR.summary_of(got)[k] for k in (0, 1, 4, 5, 6, 7))
    for i in RESTATED:
        t = PT.build(c_oracle.COraclePuzzle(texts[i]))
        assert t.info[0] <= 65
        BR.compare(BR.of_batch(batch, i), BR.of_restated(t))
    # the labels of the whole set from summaries alone
    pushes, states, share = generate.push_difficulty(vec.pset, max_states=MIX_CAP)
    built = np.array([r is not None for r in refs])
    summary = batch.summary.cpu().numpy()
    assert (pushes[built] == summary[built, 5]).all() and (states[built] == summary[built, 0]).all()
    assert (pushes[~built] == -1).all() and (states[~built] == 0).all() and np.isnan(share[~built]).all()
    assert np.allclose(share[built], summary[built, 3] / summary[built, 0])


# ---- 7. the expert in pushes, end to end ---------------------------------------------------------------------------------------------
def test_expert_end_to_end():
    texts, vec, batch, refs = _mix()
    B = vec.num_envs
    vec.reset()
    rng = np.random.default_rng(9)
    for _ in range(6):  # a few random moves: live states off the start states
        vec.step(torch.as_tensor(rng.integers(0, 4, B).astype(np.uint8), device=vec.device))
    q = vec.push_cost_to_go([batch])
    cost0 = q.cost.clone()
    covered = batch.covers(vec.puzzle_id)
    assert bool((cost0[~covered] == -2).all()) and bool((cost0[covered] >= -1).all()) and int((cost0 > 0).sum()) > 20
    cost = cost0.clone()
    pushes = torch.zeros(B, dtype=torch.int32, device=vec.device)
    for _ in range(int(cost0.max()) + 1):
        live = cost > 0
        if not bool(live.any()):
            break
        before = vec.pos.clone()
        _, _, term, _, _, status = vec.step_push(q.push_from.contiguous(), q.push_action.contiguous())
        # dead ends, goal states and states without a table hold no push (PUSH_NONE): refused, the environment is as it was
        assert bool((status[live] == PUSH_DONE).all()) and bool((status[~live] != PUSH_DONE).all())
        assert bool((status[cost < 0] == PUSH_REFUSED).all()) and bool((vec.pos[~live] == before[~live]).all())
        pushes += live
        q = vec.push_cost_to_go([batch])
        assert bool((q.cost[live] == cost[live] - 1).all())  # the cost falls by exactly 1 per push
        assert bool((q.cost[~live] == cost[~live]).all())
        assert bool(((term[live] != 0) == (q.cost[live] == 0)).all())  # and it is 0 exactly where the episode ends
        cost = q.cost.clone()
    solvable = cost0 > 0
    assert bool((cost[solvable] == 0).all()) and bool((pushes[solvable] == cost0[solvable]).all())
    assert bool((pushes[~solvable] == 0).all())
    # a mixed list: the batch of the even puzzles and one push_table of a puzzle outside it
    vec.reset()
    odd = next(i for i in range(1, MIX, 2) if refs[i] is not None)
    with vec.push_tables(list(range(0, MIX, 2)), max_states_each=MIX_CAP) as even, vec.push_table(odd, max_states=MIX_CAP) as tab:
        both = vec.push_cost_to_go([even, tab])
        whole = vec.push_cost_to_go([batch])
        ids = vec.puzzle_id
        own = ((ids % 2 == 0) & even.covers(ids)) | (ids == odd)
        assert int((ids == odd).sum()) > 0 and int(own.sum()) > int((ids == odd).sum())
        for name in ("cost", "push_from", "push_action", "walk", "action"):  # (index: each table numbers its own states)
            a, b = getattr(both, name), getattr(whole, name)
            assert bool((a[own] == b[own]).all()), name
        assert bool((both.cost[~own] == -2).all()) and bool((both.index[~own] == -1).all())
        assert bool((vec.push_expert_actions([even, tab]) == both.action).all())
    other = VecPushWorld([PushWorldPuzzle(text=texts[0])], 2, observation=None, max_steps=None)
    with other.push_tables(max_states_each=MIX_CAP) as foreign:
        with pytest.raises(ValueError, match="made on this environment"):
            vec.push_cost_to_go([foreign])
        for call in (vec.reset_from_push_tables, vec.optimal_push_demonstrations, vec.fewest_push_plans):
            with pytest.raises(ValueError, match="not supported here yet"):
                call([foreign])


# ---- 8. a captured query ------------------------------------------------------------------------------------------------------------------
def test_query_in_a_graph():
    """The query allocates nothing and does not synchronise: captured once, replayed twice on live states that move on."""
    texts, vec, batch, refs = _mix()
    vec.reset()
    ids, pos = vec.puzzle_id, vec.pos

    def sentinels():  # (environments whose puzzle has no table keep them)
        return PushQuery(*(torch.full_like(x, 55) for x in batch.query(ids, pos)))

    out = sentinels()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        batch.query(ids, pos, out=out)
    rng = np.random.default_rng(2)
    for _ in range(2):
        vec.step(torch.as_tensor(rng.integers(0, 4, vec.num_envs).astype(np.uint8), device=vec.device))
        want = _host(batch.query(ids, pos, out=sentinels()))
        for x in out:
            x.fill_(55)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(_host(out), want):
            assert (a == b).all()
        assert (want.index != 55).sum() > 100 and ((want.cost > 0) & (want.cost != 55)).sum() > 20

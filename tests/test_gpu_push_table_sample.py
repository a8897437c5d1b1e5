"""Drawing from the cost-to-go tables over pushes (pw_push_search_table_index / _sample / _plans / _emit,
search.PushSolutionTable.cost_index / sample / plans / demonstration_rows, VecPushWorld.reset_from_push_tables /
optimal_push_demonstrations) against the plain-Python restatement of tests/push_table_sample_restatement.py --
whose emitted states come from the C oracle's step alone --, against pw_step_push end to end, and on `room3` against the
table's own arrays recomputed with torch."""
import numpy as np
import pytest
import torch

import deep_puzzles
import push_table_restatement as TR
import push_table_sample_restatement as SR
import walk_restatement as WR
from pushworld_amd import _capi
from pushworld_amd.puzzle import PushWorldPuzzle
from pushworld_amd.search import PLANS_CUT, PLANS_NONE, PUSH_NONE, PushPlans, PushRows, PushSolutionTable, decode_push_choice
from pushworld_amd.vec_env import VecPushWorld
from test_gpu_push_search import _with_bits

pytestmark = pytest.mark.gpu

NAMES = list(TR.EXPECT)
_PZ, _TAB, _INDEX = {}, {}, {}
SENT = 77  # what every output holds before a launch


def _puzzle(name):
    if name not in _PZ:
        _PZ[name] = PushWorldPuzzle(text=TR.case(name)[0])
    return _PZ[name]


def _table(name):
    """The case's table on the device, built once and never changed by a test (tests that restart a search build their own)."""
    if name not in _TAB:
        _TAB[name] = PushSolutionTable(_puzzle(name), start=TR.case(name)[2])
    return _TAB[name]


def _index(name):
    if name not in _INDEX:
        _INDEX[name] = SR.cost_index(TR.case(name)[3])
    return _INDEX[name]


def _full(shape, dtype, dev, value=SENT):
    return torch.full(shape, value, dtype=dtype, device=dev)


def _state_pos(states, npad):
    pos = np.zeros((len(states), npad, 2), np.int8)
    for i, s in enumerate(states):
        pos[i, :len(s)] = np.asarray(s, np.int64).astype(np.int8)
    return pos


# ---- 1. the index ---------------------------------------------------------------------------------------------------------------
def _check_index(tab, t):
    sbc, cs = SR.cost_index(t)
    got = tab.cost_index()
    assert got[0].dtype == torch.int32 and got[1].dtype == torch.uint32
    assert got[0].cpu().tolist() == sbc and got[1].cpu().view(torch.int32).tolist() == cs
    again = tab.cost_index()  # idempotent: the same words
    assert torch.equal(again[0], got[0]) and torch.equal(again[1].view(torch.int32), got[1].view(torch.int32))
    return sbc, cs


@pytest.mark.parametrize("name", NAMES)
def test_index(name):
    _check_index(_table(name), TR.case(name)[3])


def test_index_is_gone_after_begin():
    _, cp, _, t = TR.case("big")
    with PushSolutionTable(_puzzle("big")) as tab:
        sbc, cs = _check_index(tab, t)
        h = tab.search._handle
        buf = torch.empty(t.info[0], dtype=torch.int32, device=tab.device)
        tab.search.begin()
        with pytest.raises(ValueError, match="pw_push_search_table_index_read.*no table"):
            h.table_index_read(buf, None)
        with pytest.raises(ValueError, match="pw_push_search_table_index.*no table"):
            h.table_index()
        while not tab.search.exhausted:
            tab.search.expand()
        assert h.solve() == tab.info
        with pytest.raises(ValueError, match="no index yet"):  # a new solve starts without an index
            h.table_index_read(buf, None)
        n = 4
        with pytest.raises(ValueError, match="pw_push_search_table_sample.*no index yet"):
            h.table_sample(None, None, n, tab.npad, 0, torch.zeros(n, dtype=torch.int32, device=tab.device), 0, 1, None, None,
                           torch.zeros((n, tab.npad, 2), dtype=torch.int8, device=tab.device),
                           torch.zeros(n, dtype=torch.int32, device=tab.device), None, None,
                           torch.zeros(n, dtype=torch.int32, device=tab.device), torch.zeros(n, dtype=torch.int32, device=tab.device))
        assert tab.cost_index()[0].cpu().tolist() == sbc


# ---- 2. the sample ---------------------------------------------------------------------------------------------------------------
def _check_sample(tab, cp, t, index, n, cost, seed, pid, other=(5,), masked=(7, 500)):
    """One sample launch over ``n`` environments with sentinels in every output, against the restatement word for word; then the
    round trip through the query."""
    sbc, cs = index
    dev, npad, N = tab.device, tab.npad, cp.num_movables
    ids = np.full(n, pid, np.int32)
    mask = np.ones(n, np.uint8)
    for i in other:
        if i < n:
            ids[i] = pid + 3
    for i in masked:
        if i < n:
            mask[i] = 0
    c0 = (np.arange(n) % 3).astype(np.int32)
    if isinstance(cost[0], np.ndarray):
        lo, hi = cost
        arg = (torch.as_tensor(lo, device=dev), torch.as_tensor(hi, device=dev))
    else:
        lo = np.full(n, cost[0])
        hi = np.full(n, (1 << 31) - 1 if cost[1] is None else cost[1])
        arg = cost
    pos, steps = _full((n, npad, 2), torch.int8, dev), _full((n,), torch.int32, dev)
    term, trunc = _full((n,), torch.uint8, dev), _full((n,), torch.uint8, dev)
    counter = torch.as_tensor(c0, device=dev)
    out = (_full((n,), torch.int32, dev), _full((n,), torch.int32, dev))
    got = tab.sample(torch.as_tensor(ids, device=dev), pos, steps, term, trunc, cost=arg, mask=torch.as_tensor(mask, device=dev),
                     seed=seed, counter=counter, out=out)
    assert got[0] is out[0] and got[1] is out[1]
    w_pos = np.full((n, npad, 2), SENT, np.int8)
    w_steps, w_flag, w_ctr = np.full(n, SENT, np.int32), np.full(n, SENT, np.uint8), c0.copy()
    w_state, w_cost = np.full(n, SENT, np.int32), np.full(n, SENT, np.int32)
    drawn = np.zeros(n, bool)
    for i in range(n):
        if not mask[i] or ids[i] != pid:
            continue
        s = SR.draw_state(seed, i, int(c0[i]) + 1, int(lo[i]), int(hi[i]), sbc, cs)
        if s is None:
            w_state[i] = w_cost[i] = -1
            continue
        drawn[i] = True
        w_ctr[i] += 1
        w_pos[i] = 0
        w_pos[i, :N] = np.asarray(t.store.states[s], np.int64).astype(np.int8)
        w_steps[i] = w_flag[i] = 0
        w_state[i], w_cost[i] = s, t.cost[s]
    assert (out[0].cpu().numpy() == w_state).all() and (out[1].cpu().numpy() == w_cost).all()
    assert (counter.cpu().numpy() == w_ctr).all()
    assert (pos.cpu().numpy() == w_pos).all()
    assert (steps.cpu().numpy() == w_steps).all()
    assert (term.cpu().numpy() == w_flag).all() and (trunc.cpu().numpy() == w_flag).all()
    if drawn.any():
        q = tab.query(None, pos, mask=torch.as_tensor(drawn.astype(np.uint8), device=dev), actions=False)
        assert (q.index.cpu().numpy()[drawn] == w_state[drawn]).all() and (q.cost.cpu().numpy()[drawn] == w_cost[drawn]).all()
    return w_state, drawn


@pytest.mark.parametrize("name", NAMES)
def test_sample(name):
    _, cp, _, t = TR.case(name)
    tab, mc, n = _table(name), t.info[4], 1000
    top = max(mc, 0)
    wide = np.arange(n, dtype=np.int64)
    bands = [(1, None), (top, top), (0, 0),
             (((wide * 3) % (mc + 56) - 5).astype(np.int32), ((wide * 7) % (mc + 56) - 5).astype(np.int32))]
    states = set()
    for k, cost in enumerate(bands):
        w_state, drawn = _check_sample(tab, cp, t, _index(name), n, cost, 11 + k, tab.puzzle_index)
        states |= set(w_state[drawn].tolist())
        if k < 3 and drawn.any():  # a scalar band draws inside it
            lo, hi = SR.clamp_band(cost[0], (1 << 31) - 1 if cost[1] is None else cost[1], mc)
            assert all(lo <= t.cost[s] <= hi for s in w_state[drawn].tolist())
    assert (len(states) > 0) == (mc >= 0) and all(t.cost[s] >= 0 for s in states)
    if name == "big":
        assert len(states) > 400


def test_sample_without_ids_and_flags():
    _, cp, _, t = TR.case("big")
    tab = _table("big")
    n, dev = 300, tab.device
    pos, steps = _full((n, tab.npad, 2), torch.int8, dev), _full((n,), torch.int32, dev)
    state, cost = tab.sample(None, pos, steps, cost=(2, 4), seed=5)
    sbc, cs = _index("big")
    want = [SR.draw_state(5, i, 1, 2, 4, sbc, cs) for i in range(n)]
    assert state.cpu().tolist() == want and cost.cpu().tolist() == [t.cost[s] for s in want]
    assert (steps == 0).all() and (pos.cpu().numpy()[:, :3] == np.asarray([t.store.states[s] for s in want], np.int8)).all()


# ---- 3. the plans ---------------------------------------------------------------------------------------------------------------
def _run_plans(tab, idx, tie, seed, plan_cap, ids=None, mask=None):
    dev, n = tab.device, len(idx)
    out = PushPlans(_full((n, plan_cap, 2), torch.int8, dev), _full((n, plan_cap), torch.uint8, dev),
                    _full((n, plan_cap), torch.int32, dev), _full((n,), torch.int32, dev))
    got = tab.plans(torch.as_tensor(np.asarray(idx, np.int32), device=dev), ids, mask=mask, tie=tie, seed=seed, plan_cap=plan_cap,
                    out=out)
    assert all(a is b for a, b in zip(got, out))
    return out


def _check_plans(tab, t, idx, tie, seed, plan_cap, skip=()):
    """The plans from the store indices ``idx`` (items of ``skip`` are of another puzzle or masked: see the callers)."""
    out = _run_plans(tab, idx, tie, seed, plan_cap)
    frm, act, node, length = (x.cpu().numpy() for x in out)
    plans = []
    for i, s in enumerate(idx):
        steps = SR.plan(t, s, 1 if tie == "uniform" else 0, seed, i)
        plans.append(steps)
        if steps is None or len(steps) > plan_cap:
            assert length[i] == (PLANS_NONE if steps is None else PLANS_CUT)
            k = 0
        else:
            k = len(steps)
            assert length[i] == k == t.cost[s]
            assert [tuple(v) for v in frm[i, :k].tolist()] == [st.frm for st in steps]
            assert act[i, :k].tolist() == [st.action for st in steps] and node[i, :k].tolist() == [st.node for st in steps]
        assert (frm[i, k:] == SENT).all() and (act[i, k:] == SENT).all() and (node[i, k:] == SENT).all()
    return out, plans


def _some_states(t, limit):
    S = t.info[0]
    return list(range(0, S, max(1, S // limit)))


@pytest.mark.parametrize("name", NAMES)
def test_plans(name):
    _, cp, _, t = TR.case(name)
    tab, S, mc = _table(name), t.info[0], t.info[4]
    cap = max(mc, 1)
    idx = _some_states(t, 1500) + [-1, S]
    out, plans = _check_plans(tab, t, idx, "lowest", 0, cap)
    # tie 0 is the chain of best: recomputed from the arrays read back
    row_off, best = tab.offsets().cpu().numpy(), tab.best().cpu().numpy()
    succ, frm, action, flags = (x.cpu().numpy() for x in tab.rows())
    for i, s in list(enumerate(idx))[:: max(1, len(idx) // 200)]:
        if plans[i]:
            cur = s
            for k, st in enumerate(plans[i]):
                r = row_off[cur] + best[cur]
                assert st == SR.Step(tuple(frm[r].tolist()), int(action[r]), cur)
                cur = int(succ[r])
            assert flags[r] & 1 or t.cost[cur] == 0
    assert out.length.cpu().tolist()[-2:] == [PLANS_NONE, PLANS_NONE]
    for seed in (3, 1 << 40):
        _check_plans(tab, t, idx, "uniform", seed, cap)
    # an item of another puzzle: -1 and nothing else; a masked item: untouched
    dev = tab.device
    ids = torch.full((len(idx),), tab.puzzle_index, dtype=torch.int32, device=dev)
    ids[0] = tab.puzzle_index + 1
    mask = torch.ones(len(idx), dtype=torch.uint8, device=dev)
    mask[1] = 0
    got = _run_plans(tab, idx, "lowest", 0, cap, ids=ids, mask=mask)
    assert int(got.length[0]) == PLANS_NONE and int(got.length[1]) == SENT
    assert bool((got.state[:2] == SENT).all()) and bool((got.push_action[:2] == SENT).all())
    assert torch.equal(got.length[2:], out.length[2:]) and torch.equal(got.state[2:], out.state[2:])


def test_plan_cap_cuts_exactly_the_longest():
    name = "shape (8, 16, 2) deep goal start"
    _, cp, _, t = TR.case(name)
    tab, S = _table(name), t.info[0]
    assert t.info[4] == 36
    cost = np.asarray(t.cost)
    keep = _run_plans(tab, list(range(S)), "lowest", 0, 36)
    assert (keep.length.cpu().numpy() == np.where(cost >= 0, cost, PLANS_NONE)).all()
    cut = _run_plans(tab, list(range(S)), "lowest", 0, 35)
    want = np.where(cost == 36, PLANS_CUT, np.where(cost >= 0, cost, PLANS_NONE))
    assert (cut.length.cpu().numpy() == want).all() and int((want == PLANS_CUT).sum()) > 0
    longest = torch.as_tensor(cost == 36, device=tab.device)
    assert bool((cut.state[longest] == SENT).all()) and bool((cut.push_from[longest] == SENT).all())
    assert torch.equal(cut.state[~longest], keep.state[~longest][:, :35])


# ---- 4. the emit ---------------------------------------------------------------------------------------------------------------
def _moved_inside_region(cp, t, node, k):
    """The stored state of ``node`` with the agent a few walk steps away, inside its region: the same node.  (From a start
    that overlaps something the way back may be closed: such a position is another node, and the stored state is kept.)"""
    state = t.store.states[node]
    reg = WR.region(cp, state)
    near = sorted(q for q, d in reg.dist.items() if d <= 3)
    moved = (near[k % len(near)],) + tuple(tuple(xy) for xy in state[1:])
    return moved if TR.query(cp, t, moved).index == node else tuple(tuple(xy) for xy in state)


def _check_rows(rows, want, npad, N, cap=None):
    T = len(want) if cap is None else cap
    want = want[:T]
    item, step, node, frm, act, cost, pos = (x.cpu().numpy() for x in rows[:7])
    assert item[:T].tolist() == [r.item for r in want] and step[:T].tolist() == [r.t for r in want]
    assert node[:T].tolist() == [r.node for r in want] and cost[:T].tolist() == [r.cost for r in want]
    assert [tuple(v) for v in frm[:T].tolist()] == [r.frm for r in want] and act[:T].tolist() == [r.action for r in want]
    assert (pos[:T] == _state_pos([r.pos for r in want], npad)).all()  # (zeros from the puzzle's movables on)


def _check_emit(tab, cp, t, states, tie="uniform", seed=5):
    dev, npad, N = tab.device, tab.npad, cp.num_movables
    live = [_moved_inside_region(cp, t, s, i) for i, s in enumerate(states)]
    assert any(a != tuple(tuple(xy) for xy in t.store.states[s]) for a, s in zip(live, states)) or len(states) < 10
    pos = torch.as_tensor(_state_pos(live, npad), device=dev)
    q = tab.query(None, pos, actions=False)
    assert q.index.cpu().tolist() == list(states)  # every agent position of the region is the same node
    cap = max(t.info[4], 1)
    plans = tab.plans(q.index, tie=tie, seed=seed, plan_cap=cap)
    steps = [SR.plan(t, s, 1 if tie == "uniform" else 0, seed, i) for i, s in enumerate(states)]
    want_live = [r for i, st in enumerate(steps) for r in SR.rows(cp, t, i, live[i], st or [])]
    want_stored = [r for i, st in enumerate(steps) for r in SR.rows(cp, t, i, None, st or [])]
    T = len(want_live)
    rows = tab.demonstration_rows(plans, pos=pos)
    assert rows.num_rows == T == int(plans.length.clamp(min=0).sum()) and int(rows.dropped.view(torch.int32)[0]) == 0
    _check_rows(rows, want_live, npad, N)
    rows = tab.demonstration_rows(plans)
    _check_rows(rows, want_stored, npad, N)
    # half the capacity: the other half stays as it was and is counted
    half = T // 2
    sent = PushRows(_full((T,), torch.int32, dev), _full((T,), torch.int32, dev), _full((T,), torch.int32, dev),
                    _full((T, 2), torch.int8, dev), _full((T,), torch.uint8, dev), _full((T,), torch.int32, dev),
                    _full((T, npad, 2), torch.int8, dev), torch.zeros(1, dtype=torch.int32, device=dev), T)
    if T > 0:
        got = tab.demonstration_rows(plans, pos=pos, rows_cap=half, out=sent)
        _check_rows(got, want_live, npad, N, cap=half)
        assert int(got.dropped[0]) == T - half
        for x in got[:7]:
            assert bool((x[half:] == SENT).all())
    return T


@pytest.mark.parametrize("name", NAMES)
def test_emit(name):
    _, cp, _, t = TR.case(name)
    T = _check_emit(_table(name), cp, t, _some_states(t, 60))
    assert (T > 0) == (t.info[4] > 0)


def test_emit_skips_masked_items_and_other_puzzles():
    _, cp, _, t = TR.case("big")
    tab, dev = _table("big"), _table("big").device
    states = [s for s in range(0, 1260, 40) if t.cost[s] > 0][:12]
    n = len(states)
    plans = tab.plans(torch.as_tensor(np.asarray(states, np.int32), device=dev), plan_cap=8)
    ids = torch.zeros(n, dtype=torch.int32, device=dev)
    ids[2] = 1
    mask = torch.ones(n, dtype=torch.uint8, device=dev)
    mask[4] = 0
    rows = tab.demonstration_rows(plans, puzzle_id=ids, mask=mask)
    want = [r for i, s in enumerate(states) if i not in (2, 4) for r in SR.rows(cp, t, i, None, SR.plan(t, s, 0, 0, i))]
    assert rows.num_rows == len(want)
    _check_rows(rows, want, tab.npad, 3)


# ---- 5. end to end against pw_step_push -------------------------------------------------------------------------------------------
def test_end_to_end_against_step_push():
    _, cp, _, t = TR.case("big")
    B = 270
    vec = VecPushWorld([_puzzle("big")], B, observation=None, max_steps=None, seed=9)
    dev = vec.device
    with vec.push_table(0) as tab:
        band = torch.as_tensor((np.arange(B) % 9).astype(np.int32), device=dev)
        vec.reset_from_push_tables([tab], cost=(band, band))
        assert torch.equal(vec.start_cost, band) and bool((vec.table_draws.view(torch.int32) == 1).all())
        q = vec.push_cost_to_go([tab])
        assert torch.equal(q.index, vec.start_row) and torch.equal(q.cost, vec.start_cost)
        assert set(vec.start_cost.cpu().tolist()) == set(range(9))  # all 8 costs, and goal states
        start = vec.pos.clone()
        plans = tab.plans(q.index, tie="uniform", seed=3, plan_cap=8)
        rows = tab.demonstration_rows(plans, pos=vec.pos)
        cost = plans.length
        assert torch.equal(cost, band)
        offset = torch.zeros(B + 1, dtype=torch.int64, device=dev)
        offset[1:] = torch.cumsum(cost.to(torch.int64), 0)
        assert rows.num_rows == int(offset[B])
        first = offset[:-1][cost > 0]
        assert torch.equal(rows.pos[first], start[cost > 0])
        for step in range(8):
            acting = cost > step
            action = torch.where(acting, plans.push_action[:, step], torch.full_like(plans.push_action[:, step], PUSH_NONE))
            _, _, term, _, _, status = vec.step_push(plans.push_from[:, step].contiguous(), action.contiguous())
            assert bool((status[acting] == _capi.PUSH_DONE).all()) and bool((status[~acting] == _capi.PUSH_REFUSED).all())
            more = cost > step + 1
            assert torch.equal(vec.pos[more], rows.pos[(offset[:-1] + step + 1)[more]])
            assert torch.equal(term[cost > 0].bool(), (cost <= step + 1)[cost > 0])  # first true at exactly macro step `cost`
        assert bool((vec.pos[cost == 0] == start[cost == 0]).all())
        # the same seed draws the same states; a second reset without a seed draws with the counters advanced
        again = VecPushWorld([_puzzle("big")], B, observation=None, max_steps=None, seed=9)
        with again.push_table(0) as tab2:
            again.reset_from_push_tables([tab2], cost=(band, band))
            assert torch.equal(again.pos, start) and torch.equal(again.start_row, q.index)
            again.reset_from_push_tables([tab2], cost=(1, None), mask=(band == 3))
            assert again.table_draws.view(torch.int32).cpu().tolist() == [2 if c == 3 else 1 for c in band.cpu().tolist()]
            assert bool((again.start_cost >= 0).all()) and torch.equal(again.pos[band != 3], start[band != 3])


# ---- 6. shapes --------------------------------------------------------------------------------------------------------------------
def _check_everything_small(tab, cp, t, pid):
    index = _check_index(tab, t)
    _check_sample(tab, cp, t, index, 200, (1, None), 21, pid, other=(5,), masked=(7,))
    states = [s for s in _some_states(t, 40) if t.cost[s] >= 0][:24]
    assert _check_emit(tab, cp, t, states) > 20


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
        assert tab.puzzle_index == index
        _check_everything_small(tab, cp, t, index)


def test_big_one_fingerprint_bit():
    _, cp, _, t = TR.case("big")
    pz = _puzzle("big")

    def run():
        with PushSolutionTable(pz, chunk=7) as tab:
            _check_everything_small(tab, cp, t, tab.puzzle_index)

    _with_bits(pz, 1, run)


# ---- 7. demonstrations over two tables ---------------------------------------------------------------------------------------------
def test_demonstrations_of_a_mixed_batch():
    names = ["big", "serpentine 14x13 overshoot"]
    cases = [TR.case(k) for k in names]
    B = 64
    vec = VecPushWorld([PushWorldPuzzle(text=c[0]) for c in cases], B, observation="cells", max_steps=None, seed=3)
    dev = vec.device
    with vec.push_table(0) as t0, vec.push_table(1) as t1:
        vec.reset_from_push_tables([t0, t1], cost=(0, None))
        ids = vec.puzzle_id.cpu().numpy()
        assert set(ids.tolist()) == {0, 1}
        start = vec.pos.clone()
        live = vec.states()
        mask = torch.ones(B, dtype=torch.uint8, device=dev)
        mask[3] = 0
        d = vec.optimal_push_demonstrations([t0, t1], tie="uniform", seed=4, mask=mask, masks=True)
        want = []
        for e in range(B):
            _, cp, _, t = cases[ids[e]]
            if e == 3:
                continue
            state = tuple(tuple(int(v) for v in xy) for xy in live[e, :cp.num_movables])
            node = TR.query(cp, t, state).index
            assert node == int(vec.start_row[e])
            want += SR.rows(cp, t, e, state, SR.plan(t, node, 1, 4, e) or [])
        assert d.num_rows == len(want) > B
        _check_rows((d.item, d.t, d.state, d.push_from, d.push_action, d.cost, d.pos), want, vec.num_objects_padded, 0)
        assert d.puzzle_id.cpu().tolist() == [int(ids[r.item]) for r in want]
        frm, action = decode_push_choice(d.choice, vec.pset.max_height, vec.pset.max_width)
        assert torch.equal(frm, d.push_from) and torch.equal(action, d.push_action)
        assert d.obs.shape[0] == d.num_rows and d.obs.dtype == torch.uint8
        # every row's push is a push move of the row's state
        x, y = d.push_from[:, 0].long(), d.push_from[:, 1].long()
        bits = d.push_mask[torch.arange(d.num_rows, device=dev), y, x]
        assert bool((((bits.long() >> d.push_action.long()) & 1) == 1).all())
        only0 = vec.optimal_push_demonstrations([t0], observation=None)
        assert set(only0.puzzle_id.cpu().tolist()) == {0} and only0.obs is None
        # step_push(choice=...) from the rows' states pushes: every environment's first row (an environment without rows
        # passes -1, which is no push move)
        first = d.t == 0
        env = d.item[first].long()
        choice = torch.full((B,), -1, dtype=torch.int64, device=dev)
        choice[env] = d.choice[first]
        states = start.clone()
        states[env] = d.pos[first]
        assert torch.equal(states, start)  # (row 0 of an environment is its live state)
        vec.set_states(states.cpu().numpy())
        *_, status = vec.step_push(choice=choice)
        has = torch.zeros(B, dtype=torch.bool, device=dev)
        has[env] = True
        assert bool((status[has] == _capi.PUSH_DONE).all()) and bool((status[~has] == _capi.PUSH_REFUSED).all())
        assert int(has.sum()) > B // 2 and bool((vec.pos[has][:, 1:] != start[has][:, 1:]).any(dim=2).any(dim=1).all())
        second = torch.nonzero(d.t == 1).squeeze(1)  # the state after the first push is the second row's
        assert second.numel() > 0 and torch.equal(vec.pos[d.item[second].long()], d.pos[second])
        with PushSolutionTable(_puzzle("big")) as foreign:
            with pytest.raises(ValueError, match="made on this environment"):
                vec.optimal_push_demonstrations([foreign])
            with pytest.raises(ValueError, match="made on this environment"):
                vec.reset_from_push_tables([foreign])


# ---- 8. capture -------------------------------------------------------------------------------------------------------------------
def test_capture_sample_and_plans():
    _, cp, _, t = TR.case("big")
    tab, n = _table("big"), 512
    dev = tab.device
    sbc, cs = _index("big")
    tab.cost_index()  # (the index is built outside the capture)
    pos, steps = torch.zeros((n, tab.npad, 2), dtype=torch.int8, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
    counter = torch.zeros(n, dtype=torch.int32, device=dev)
    out = (torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev))
    index = torch.zeros(n, dtype=torch.int32, device=dev)
    plans = PushPlans(torch.zeros((n, 8, 2), dtype=torch.int8, device=dev), torch.zeros((n, 8), dtype=torch.uint8, device=dev),
                      torch.zeros((n, 8), dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    g_sample, g_plans = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(g_sample):
        tab.sample(None, pos, steps, cost=(1, None), seed=13, counter=counter, out=out)
    with torch.cuda.graph(g_plans):
        tab.plans(index, tie="uniform", seed=2, plan_cap=8, out=plans)
    counter.zero_()
    for replay in (1, 2):
        g_sample.replay()
        index.copy_(out[0])
        g_plans.replay()
        torch.cuda.synchronize()
        want = [SR.draw_state(13, i, replay, 1, 1 << 30, sbc, cs) for i in range(n)]
        assert out[0].cpu().tolist() == want and counter.cpu().tolist() == [replay] * n
        # the eager calls with the same counters give the same words
        e_pos, e_steps = torch.zeros_like(pos), torch.zeros_like(steps)
        e_ctr = torch.full((n,), replay - 1, dtype=torch.int32, device=dev)
        e_state, e_cost = tab.sample(None, e_pos, e_steps, cost=(1, None), seed=13, counter=e_ctr)
        assert torch.equal(e_state, out[0]) and torch.equal(e_cost, out[1]) and torch.equal(e_pos, pos)
        eager = tab.plans(index, tie="uniform", seed=2, plan_cap=8)
        live = torch.arange(8, device=dev).unsqueeze(0) < plans.length.unsqueeze(1)
        assert torch.equal(eager.length, plans.length) and torch.equal(eager.length, out[1])
        assert torch.equal(eager.state[live], plans.state[live]) and torch.equal(eager.push_action[live], plans.push_action[live])
        assert torch.equal(eager.push_from[live], plans.push_from[live])


# ---- 9. room3 -------------------------------------------------------------------------------------------------------------------
def test_room3():
    text = deep_puzzles.room3()
    with PushSolutionTable(PushWorldPuzzle(text=text), max_states=1 << 16) as tab:
        assert tab.info == (42840, 316176, 1190, 15778, 10)
        S, mc, dev = tab.num_states, tab.max_cost, tab.device
        cost = tab.costs().to(torch.int64)
        sbc, cs = tab.cost_index()
        cs = cs.view(torch.int32).to(torch.int64)
        # the bucket sizes sum to info; every bucket holds its cost in ascending store index
        sizes = cs[1:] - cs[:-1]
        assert int(cs[0]) == 0 and int(cs[-1]) == S and int(sizes[0]) == 1190 and int(sizes[-1]) == 15778 and sizes.numel() == mc + 2
        assert torch.equal(sizes[:-1], torch.bincount(cost[cost >= 0], minlength=mc + 1))
        bucket = torch.where(cost >= 0, cost, torch.full_like(cost, mc + 1))
        order = torch.sort(bucket * S + torch.arange(S, device=dev)).indices  # (bucket, store index) ascending
        assert torch.equal(sbc.to(torch.int64), order)
        # the plans from every 40th state: as long as the cost, and the cost falls by one per push along succ
        idx = torch.arange(0, S, 40, dtype=torch.int32, device=dev)
        row_off, best = tab.offsets(), tab.best().to(torch.int64)
        succ, frm, action, flags = tab.rows()
        succ = succ.to(torch.int64)
        for tie in ("lowest", "uniform"):
            plans = tab.plans(idx, tie=tie, seed=6, plan_cap=mc)
            c = cost[idx.long()]
            assert torch.equal(plans.length.to(torch.int64), torch.where(c >= 0, c, torch.full_like(c, PLANS_NONE)))
            cur = idx.long().clone()
            for step in range(mc):
                on = c > step
                node = plans.state[:, step].to(torch.int64)
                assert torch.equal(node[on], cur[on]) and torch.equal(cost[cur[on]], (c - step)[on])
                # the row of the push: the state's rows hold it, it is optimal, and its successor is the next node
                lo, hi = row_off[node[on]], row_off[node[on] + 1]
                if tie == "lowest":
                    r = lo + best[node[on]]
                else:
                    r = torch.empty_like(lo)
                    for k in range(int(on.sum())):  # (a few hundred items: the row with this push among the state's rows)
                        rs = torch.arange(int(lo[k]), int(hi[k]), device=dev)
                        hit = (frm[rs] == plans.push_from[on][k, step]).all(dim=1) & (action[rs] == plans.push_action[on][k, step])
                        r[k] = rs[hit][0]
                assert bool(((flags[r] & 2) != 0).all())
                assert torch.equal(frm[r], plans.push_from[on][:, step]) and torch.equal(action[r], plans.push_action[on][:, step])
                goal_row = (flags[r] & 1) != 0
                assert bool((c[on][goal_row] == step + 1).all())
                nxt = cur.clone()
                nxt[on] = torch.where(goal_row, cur[on], succ[r])
                cur = nxt
        rows = tab.demonstration_rows(plans)
        assert rows.num_rows == int(plans.length.clamp(min=0).sum()) and int(rows.dropped.view(torch.int32)[0]) == 0
        assert bool((rows.cost >= 1).all()) and torch.equal(cost[rows.state.long()], rows.cost.to(torch.int64))
        q = tab.query(None, rows.pos, actions=False)  # the emitted states are the nodes the pushes are made from
        assert torch.equal(q.index, rows.state)

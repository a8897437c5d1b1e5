"""Drawing from the batched cost-to-go tables over pushes (pw_push_solve_batch_index / _sample / _plans / _emit,
search.PushSolutionTableBatch.build_index / cost_index / sample / plans / demonstration_rows, VecPushWorld.reset_from_push_tables /
optimal_push_demonstrations / fewest_push_plans with batches) against the plain-Python restatement of
tests/push_batch_sample_restatement.py -- whose emitted states come from the C oracle's step alone.

Everything is compared BY STATE (key), never by state number: the batched kernel numbers the states of a layer as its schedule
has it.  ``_map(batch, item)`` takes a device state number to the restatement's."""
import numpy as np
import pytest
import torch

import deep_puzzles
import push_batch_sample_restatement as XR
import push_solution_batch_restatement as BR
import push_table_restatement as PT
import walk_restatement as WR
from pushworld_amd import _capi, generate
from pushworld_amd.puzzle import PushWorldPuzzle
from pushworld_amd.search import (PLANS_CUT, PLANS_NONE, PUSH_NONE, REPLAY_VALID, TABLE_BUILT, PushPlans, PushRows, replay_plans)
from pushworld_amd.vec_env import VecPushWorld

pytestmark = pytest.mark.gpu

# the six restated cases of one set at NP 4: the (3, 12, 9) shape puzzle is listed twice, with two starts (the second overlaps
# and is all dead).  A puzzle listed twice is answered from its higher item: order "A" draws puzzle 4 from the all-dead item,
# order "B" (the two starts swapped) from the one with costs up to 3.  Puzzle 5 of the set has no item in either.
NAMES = {"A": ["big", "corridor 7", "serpentine 14x14", "serpentine 14x13 overshoot", "shape (3, 12, 9) deep goal start",
               "shape (3, 12, 9) search start 3"]}
NAMES["B"] = NAMES["A"][:4] + NAMES["A"][:3:-1]
PUZZLES = [0, 1, 2, 3, 4, 4]
NO_ITEM = 5
SENT = 77  # what every output holds before a launch
_SHARED = {}


# a puzzle with more movables, appended as puzzle 6 (never an item), pads the set to 8, 16 or 32
PAD_EXTRA = {4: None, 8: 4, 16: 10, 32: deep_puzzles.POCKETS_EXTRA}


def _vec(npad=4):
    if ("vec", npad) not in _SHARED:
        texts = [PT.case(name)[0] for name in NAMES["A"][:5]] + [deep_puzzles.corridor(7)]
        if PAD_EXTRA[npad]:
            texts.append(deep_puzzles.pockets(PAD_EXTRA[npad]))
        vec = VecPushWorld([PushWorldPuzzle(text=x) for x in texts], 8, observation=None, max_steps=None)
        assert vec.num_objects_padded == npad
        _SHARED[("vec", npad)] = vec
    return _SHARED[("vec", npad)]


def _batch(order="A", groups_per_cu=0, npad=4):
    """The indexed batch of the six cases, built once per (order, workgroups per CU, npad) and never changed by a test."""
    key = ("batch", order, groups_per_cu, npad)
    if key not in _SHARED:
        vec = _vec(npad)
        vec.engine.set_option("search_batch_groups_per_cu", groups_per_cu)
        try:
            batch = vec.push_tables(PUZZLES, starts=[PT.case(n)[2] for n in NAMES[order]], max_states_each=2048, index=True)
        finally:
            vec.engine.set_option("search_batch_groups_per_cu", 0)
        assert batch.indexed and batch.status.cpu().tolist() == [TABLE_BUILT] * 6 and batch.max_cost_stored == 8
        assert batch.npad == npad
        _SHARED[key] = batch
    return _SHARED[key]


def _case(name):
    """(cp, t, keys, (states_by_cost, cost_start)) of a restated case; computed once and never changed."""
    key = ("case", name)
    if key not in _SHARED:
        _, cp, _, t = PT.case(name)
        keys = XR.keys_of_table(t)
        _SHARED[key] = (cp, t, keys, XR.cost_index(t, keys))
    return _SHARED[key]


def _map(batch, order, item):
    """int64 [S]: the restatement's state of device state i of ``item``."""
    key = ("map", id(batch), item)
    if key not in _SHARED:
        t = _case(NAMES[order][item])[1]
        _SHARED[key] = BR.state_map(BR.of_batch(batch, item), BR.of_restated(t))
    return _SHARED[key]


def _item_of(pid):
    """The item that answers for puzzle ``pid``: the higher one of a puzzle listed twice, None without one."""
    return max((i for i, p in enumerate(PUZZLES) if p == pid), default=None)


def _full(shape, dtype, dev, value=SENT):
    return torch.full(shape, value, dtype=dtype, device=dev)


def _state_pos(states, npad):
    pos = np.zeros((len(states), npad, 2), np.int8)
    for i, s in enumerate(states):
        pos[i, :len(s)] = np.asarray(s, np.int64).astype(np.int8)
    return pos


# ---- 1. the index ---------------------------------------------------------------------------------------------------------------
def _index_as_keys(batch, order):
    """Per item (the keys in states_by_cost order, cost_start), checked against the restatement word for word."""
    out = []
    for item, name in enumerate(NAMES[order]):
        _, t, keys, (sbc, cs) = _case(name)
        got = batch.cost_index(item)
        assert got[0].dtype == torch.int32 and got[1].dtype == torch.uint32
        dev_keys = batch.keys(item).cpu().numpy().astype(np.uint64)
        got_sbc = got[0].cpu().numpy()
        assert sorted(got_sbc.tolist()) == list(range(t.info[0]))
        as_keys = dev_keys[got_sbc].tolist()
        assert as_keys == [keys[i] for i in sbc], name
        assert got[1].cpu().view(torch.int32).tolist() == cs, name
        out.append((as_keys, cs))
    return out


@pytest.mark.parametrize("order", ["A", "B"])
def test_index(order):
    one = _index_as_keys(_batch(order, 1), order)
    eight = _index_as_keys(_batch(order, 8), order)
    assert one == eight == _index_as_keys(_batch(order, 0), order)  # identical as keys whatever the launch geometry
    assert [len(cs) for _, cs in one] == [PT.EXPECT[n][6] + 3 for n in NAMES[order]]
    assert one[NAMES[order].index("shape (3, 12, 9) search start 3")][1] == [0, 261]


def test_index_is_idempotent_and_gone_after_a_run():
    vec = _vec()
    dev, lib, p = vec.device, _capi.lib, _capi._ptr
    with vec.push_tables(PUZZLES, starts=[PT.case(n)[2] for n in NAMES["A"]], max_states_each=2048) as batch:
        assert not batch.indexed and batch.max_cost_stored == -1
        n = 4
        ids, ctr = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
        pos, steps = torch.zeros((n, 4, 2), dtype=torch.int8, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
        with pytest.raises(ValueError, match="pw_push_solve_batch_sample: no index yet"):
            batch.sample(ids, pos, steps, counter=ctr)
        assert batch.build_index() is batch and batch.indexed and batch.max_cost_stored == 8
        first = _index_as_keys(batch, "A")
        assert batch.build_index() is batch and _index_as_keys(batch, "A") == first  # a second build: the same words
        a, b = batch.cost_index(0), batch.cost_index(0)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
        # a new run on the handle discards the index
        _capi.check(lib.pw_push_solve_batch_run(batch.handle, p(batch._ids), p(batch._starts), batch.npad, 6, 2048,
                                                batch._stream()))
        buf = torch.empty(1260, dtype=torch.int32, device=dev)
        rc = lib.pw_push_solve_batch_index_read(batch.handle, 0, p(buf), None, batch._stream())
        assert rc == _capi.PW_EINVAL and "pw_push_solve_batch_index_read: no index yet" in _capi.last_error()
        with pytest.raises(ValueError, match="pw_push_solve_batch_sample: no index yet"):
            batch.sample(ids, pos, steps, counter=ctr)
        batch.indexed = False
        assert _index_as_keys(batch.build_index(), "A") == first  # rebuilt: the same keys, whatever the numbers are now
        # no item, an item out of bounds
        for item in (-1, 6):
            rc = lib.pw_push_solve_batch_index_read(batch.handle, item, p(buf), None, batch._stream())
            assert rc == _capi.PW_EINVAL and "item out of bounds" in _capi.last_error()
    with vec.push_tables([0], max_states_each=64, states=0, rows=0) as dry:  # summaries only
        with pytest.raises(ValueError, match="pw_push_solve_batch_index: nothing stored"):
            dry.build_index()
    with vec.push_tables([0], max_states_each=64) as small:  # beyond the cap: pools of size 0 again
        with pytest.raises(ValueError, match="pw_push_solve_batch_index: nothing stored"):
            small.build_index()


def test_npad_below_the_sets_movables_is_refused():
    """A set padded to 32 by a puzzle with 17 movables: PW_EINVAL before any launch from the sample and the emit."""
    vec = VecPushWorld([PushWorldPuzzle(text=deep_puzzles.pockets()), PushWorldPuzzle(text=deep_puzzles.corridor(7))], 4,
                       observation=None, max_steps=None)
    assert vec.num_objects_padded == 32
    lib, p, dev = _capi.lib, _capi._ptr, vec.device
    with vec.push_tables(max_states_each=64, index=True) as batch:
        assert batch.status.cpu().tolist()[1] == TABLE_BUILT and batch.max_cost_stored == 2
        x = torch.zeros(4096, dtype=torch.int32, device=dev)
        for npad in (4, 8, 16):
            rc = lib.pw_push_solve_batch_sample(batch.handle, p(x), None, 1, npad, 0, p(x), 0, 1, None, None, p(x), p(x), None, None,
                                                p(x), p(x), None)
            assert rc == _capi.PW_EINVAL and "pw_push_solve_batch_sample: npad is smaller" in _capi.last_error()
            rc = lib.pw_push_solve_batch_emit(batch.handle, p(x), None, 1, npad, p(x), p(x), p(x), 1, p(x), None, p(x), 1, p(x), p(x),
                                              p(x), p(x), p(x), p(x), p(x), p(x), None)
            assert rc == _capi.PW_EINVAL and "pw_push_solve_batch_emit: npad is smaller" in _capi.last_error()
        # at the set's own npad the corridor draws its three states (the canonical ones: 32 pairs, zeros from the second on)
        ids = torch.ones(64, dtype=torch.int32, device=dev)
        pos, steps = _full((64, 32, 2), torch.int8, dev), _full((64,), torch.int32, dev)
        state, cost = batch.sample(ids, pos, steps, cost=(0, None), seed=1)
        assert set(cost.cpu().tolist()) == {0, 1, 2} and bool((pos[:, 2:] == 0).all()) and bool((steps == 0).all())
        q = batch.query(ids, pos, actions=False)
        assert torch.equal(q.index, state) and torch.equal(q.cost, cost)


# ---- 2. the sample ---------------------------------------------------------------------------------------------------------------
N_ENVS = 1000


def _sample_inputs():
    ids = (np.arange(N_ENVS) % 6).astype(np.int32)  # puzzle 5: no item
    mask = np.ones(N_ENVS, np.uint8)
    ids[[13, 500]] = 99, -1  # foreign ids
    mask[[7, 8, 9, 10, 11, 12, 600]] = 0  # masked environments of every puzzle
    c0 = (np.arange(N_ENVS) % 3).astype(np.int32)
    return ids, mask, c0


def _run_sample(batch, cost, seed):
    dev, npad = batch.device, batch.npad
    ids, mask, c0 = _sample_inputs()
    arg = (torch.as_tensor(cost[0], device=dev), torch.as_tensor(cost[1], device=dev)) if isinstance(cost[0], np.ndarray) else cost
    pos, steps = _full((N_ENVS, npad, 2), torch.int8, dev), _full((N_ENVS,), torch.int32, dev)
    term, trunc = _full((N_ENVS,), torch.uint8, dev), _full((N_ENVS,), torch.uint8, dev)
    counter = torch.as_tensor(c0, device=dev)
    out = (_full((N_ENVS,), torch.int32, dev), _full((N_ENVS,), torch.int32, dev))
    t_ids = torch.as_tensor(ids, device=dev)
    got = batch.sample(t_ids, pos, steps, term, trunc, cost=arg, mask=torch.as_tensor(mask, device=dev), seed=seed, counter=counter,
                       out=out)
    assert got[0] is out[0] and got[1] is out[1]
    return t_ids, pos, steps, term, trunc, counter, out


def _check_sample(batch, order, cost, seed):
    """One sample launch over the mixed set with sentinels in every output, against the restatement; the round trip."""
    ids, mask, c0 = _sample_inputs()
    npad = batch.npad
    if isinstance(cost[0], np.ndarray):
        lo, hi = cost
    else:
        lo, hi = np.full(N_ENVS, cost[0]), np.full(N_ENVS, (1 << 31) - 1 if cost[1] is None else cost[1])
    t_ids, pos, steps, term, trunc, counter, out = _run_sample(batch, cost, seed)
    state = out[0].cpu().numpy()
    w_pos = np.full((N_ENVS, npad, 2), SENT, np.int8)
    w_steps, w_flag, w_ctr = np.full(N_ENVS, SENT, np.int32), np.full(N_ENVS, SENT, np.uint8), c0.copy()
    w_cost = np.full(N_ENVS, SENT, np.int32)
    drawn = np.zeros(N_ENVS, bool)
    per_item = {}
    for i in range(N_ENVS):
        item = _item_of(int(ids[i]))
        if not mask[i] or item is None:
            assert state[i] == SENT
            continue
        cp, t, keys, (sbc, cs) = _case(NAMES[order][item])
        s = XR.draw_state(seed, i, int(c0[i]) + 1, int(lo[i]), int(hi[i]), sbc, cs)
        if s is None:
            assert state[i] == -1
            w_cost[i] = -1
            continue
        drawn[i] = True
        w_ctr[i] += 1
        w_pos[i] = 0
        w_pos[i, :cp.num_movables] = np.asarray(XR.canonical(t, s), np.int64).astype(np.int8)
        w_steps[i] = w_flag[i] = 0
        w_cost[i] = t.cost[s]
        assert 0 <= state[i] < t.info[0] and _map(batch, order, item)[state[i]] == s, (i, item)  # by state
        per_item.setdefault(item, set()).add(s)
    assert (out[1].cpu().numpy() == w_cost).all()
    assert (counter.cpu().numpy() == w_ctr).all()
    assert (pos.cpu().numpy() == w_pos).all()
    assert (steps.cpu().numpy() == w_steps).all()
    assert (term.cpu().numpy() == w_flag).all() and (trunc.cpu().numpy() == w_flag).all()
    if drawn.any():
        q = batch.query(t_ids, pos, mask=torch.as_tensor(drawn.astype(np.uint8), device=batch.device), actions=False)
        assert (q.index.cpu().numpy()[drawn] == state[drawn]).all() and (q.cost.cpu().numpy()[drawn] == w_cost[drawn]).all()
    return per_item, drawn


def _bands():
    wide = np.arange(N_ENVS, dtype=np.int64)
    return [(1, None), (8, 8), (0, 0), (2, 3),
            (((wide * 3) % 64 - 5).astype(np.int32), ((wide * 7) % 64 - 5).astype(np.int32))]  # hi < lo, below 0, beyond every mc


@pytest.mark.parametrize("order", ["A", "B"])
def test_sample(order):
    batch = _batch(order, 0)
    seen = {}
    for k, cost in enumerate(_bands()):
        per_item, drawn = _check_sample(batch, order, cost, 11 + k)
        assert drawn.sum() > 300
        for item, states in per_item.items():
            seen.setdefault(item, set()).update(states)
            if k < 4:  # a scalar band draws inside it, clamped to the item's own costs
                t = _case(NAMES[order][item])[1]
                lo, hi = XR.SR.clamp_band(cost[0], (1 << 31) - 1 if cost[1] is None else cost[1], t.info[4])
                assert all(lo <= t.cost[s] <= hi for s in states)
    dead = NAMES[order].index("shape (3, 12, 9) search start 3")
    assert set(seen) == {0, 1, 2, 3} | ({5} - {dead}) and len(seen[0]) > 150  # the all-dead item draws nothing, a lower item is never asked
    assert all(_case(NAMES[order][item])[1].cost[s] >= 0 for item, states in seen.items() for s in states)


@pytest.mark.parametrize("order", ["A", "B"])
def test_sample_is_the_same_state_at_1_and_8_workgroups_per_cu(order):
    cost, seed = _bands()[4], 5
    one, eight = _run_sample(_batch(order, 1), cost, seed), _run_sample(_batch(order, 8), cost, seed)
    assert torch.equal(one[1], eight[1])  # pos: the states
    assert torch.equal(one[5], eight[5]) and torch.equal(one[6][1], eight[6][1])  # the counters and the costs
    drawn = one[6][0] >= 0
    assert int(drawn.sum()) > 300 and torch.equal(one[6][0] < 0, eight[6][0] < 0)
    _check_sample(_batch(order, 8), order, cost, seed)


# ---- 3. the plans ---------------------------------------------------------------------------------------------------------------
def _plan_items(batch, order):
    """(puzzle id, item, device state) of one launch: every stored state of the small answering items and 256 states of `big`,
    then an index outside the item (two ways), a puzzle without an item and a foreign id."""
    items = []
    for pid in range(5):
        item = _item_of(pid)
        S = PT.EXPECT[NAMES[order][item]][0]
        for d in (range(S) if pid else [(k * 4919) % S for k in range(256)]):  # (4919 is prime: 256 distinct states of `big`)
            items.append((pid, item, d))
    return items + [(0, 0, -1), (0, 0, 1260), (1, 1, 3), (NO_ITEM, None, 0), (99, None, 0), (-1, None, 0)]


def _run_plans(batch, items, tie, seed, plan_cap, mask=None):
    dev, n = batch.device, len(items)
    out = PushPlans(_full((n, plan_cap, 2), torch.int8, dev), _full((n, plan_cap), torch.uint8, dev),
                    _full((n, plan_cap), torch.int32, dev), _full((n,), torch.int32, dev))
    ids = torch.as_tensor(np.asarray([x[0] for x in items], np.int32), device=dev)
    idx = torch.as_tensor(np.asarray([x[2] for x in items], np.int32), device=dev)
    got = batch.plans(idx, ids, mask=mask, tie=tie, seed=seed, plan_cap=plan_cap, out=out)
    assert all(a is b for a, b in zip(got, out))
    return out


def _check_plans(batch, order, items, tie, seed, plan_cap):
    out = _run_plans(batch, items, tie, seed, plan_cap)
    frm, act, node, length = (x.cpu().numpy() for x in out)
    cut = 0
    for i, (pid, item, d) in enumerate(items):
        steps = None
        if item is not None and 0 <= d < PT.EXPECT[NAMES[order][item]][0]:
            t = _case(NAMES[order][item])[1]
            m = _map(batch, order, item)
            steps = XR.plan(t, int(m[d]), 1 if tie == "uniform" else 0, seed, i)
        if steps is None or len(steps) > plan_cap:
            assert length[i] == (PLANS_NONE if steps is None else PLANS_CUT), (i, pid, d)
            cut += steps is not None
            k = 0
        else:
            k = len(steps)
            assert length[i] == k == t.cost[int(m[d])]
            assert [tuple(v) for v in frm[i, :k].tolist()] == [st.frm for st in steps]
            assert act[i, :k].tolist() == [st.action for st in steps]
            assert m[node[i, :k]].tolist() == [st.node for st in steps] and (k == 0 or node[i, 0] == d)  # by state
        assert (frm[i, k:] == SENT).all() and (act[i, k:] == SENT).all() and (node[i, k:] == SENT).all()
    return out, cut


@pytest.mark.parametrize("order", ["A", "B"])
def test_plans(order):
    batch = _batch(order, 0)
    items = _plan_items(batch, order)
    assert len(items) > 256 + 3 + 3 + 3 + 8
    out, cut = _check_plans(batch, order, items, "lowest", 0, 8)
    assert cut == 0 and out.length.cpu().tolist()[-6:] == [PLANS_NONE] * 6 and int(out.length.max()) == 8
    for seed in (3, 1 << 40):
        _, cut = _check_plans(batch, order, items, "uniform", seed, 8)
        assert cut == 0
    # plan_cap one below the largest cost cuts exactly the longest; at 2, the deep shape's cost 3 as well
    _, cut = _check_plans(batch, order, items, "lowest", 0, 7)
    cost8 = sum(1 for pid, item, d in items if pid == 0 and 0 <= d < 1260 and
                _case("big")[1].cost[int(_map(batch, order, 0)[d])] == 8)
    assert cut == cost8 > 0
    _, cut2 = _check_plans(batch, order, items, "uniform", 9, 2)
    assert cut2 > cut + (order == "B")  # (order B answers puzzle 4 from the item with a state of cost 3)
    # a masked item is untouched
    mask = torch.ones(len(items), dtype=torch.uint8, device=batch.device)
    mask[[0, 5]] = 0
    got = _run_plans(batch, items, "lowest", 0, 8, mask=mask)
    assert got.length[[0, 5]].cpu().tolist() == [SENT, SENT] and bool((got.state[[0, 5]] == SENT).all())
    keep = mask.bool()
    assert torch.equal(got.length[keep], out.length[keep]) and torch.equal(got.state[keep], out.state[keep])


# ---- 4. the emit ---------------------------------------------------------------------------------------------------------------
def _moved_inside_region(cp, t, node, k):
    """The canonical state of ``node`` with the agent on another cell of its region: the same node.  (From a start that
    overlaps something the way back may be closed: such a position is another node, and the canonical state is kept.)"""
    state = XR.canonical(t, node)
    cells = sorted(WR.region(cp, state).dist)
    moved = (cells[(3 * k + 1) % len(cells)],) + state[1:]
    return moved if PT.query(cp, t, moved).index == node else state


def _check_rows(rows, want, maps, npad, cap=None):
    """``want``: (item of the batch, Row) pairs; ``row_state`` is compared through the item's state map."""
    T = len(want) if cap is None else cap
    want = want[:T]
    item, step, node, frm, act, cost, pos = (x.cpu().numpy() for x in rows[:7])
    assert item[:T].tolist() == [r.item for _, r in want] and step[:T].tolist() == [r.t for _, r in want]
    assert [int(maps[b][node[k]]) for k, (b, _) in enumerate(want)] == [r.node for _, r in want]
    assert cost[:T].tolist() == [r.cost for _, r in want]
    assert [tuple(v) for v in frm[:T].tolist()] == [r.frm for _, r in want] and act[:T].tolist() == [r.action for _, r in want]
    assert (pos[:T] == _state_pos([r.pos for _, r in want], npad)).all()  # (zeros from the puzzle's movables on)


def _check_emit(batch, order, tie="uniform", seed=5):
    dev, npad = batch.device, batch.npad
    # restated states with a plan, of every answering item; live: other cells of their regions
    chosen = []
    for pid in range(5):
        item = _item_of(pid)
        cp, t, _, _ = _case(NAMES[order][item])
        S = t.info[0]
        for s in range(0, S, max(1, S // 40)):
            chosen.append((pid, item, s))
    chosen += [(NO_ITEM, None, 0), (99, None, 0)]
    live = []
    for k, (pid, item, s) in enumerate(chosen):
        if item is None:
            live.append(((1, 1), (2, 1)))
            continue
        cp, t, _, _ = _case(NAMES[order][item])
        live.append(_moved_inside_region(cp, t, s, k))
    assert sum(a != XR.canonical(_case(NAMES[order][it])[1], s) for a, (_, it, s) in zip(live, chosen) if it is not None) > 20
    n = len(chosen)
    maps = {item: _map(batch, order, item) for _, item, _ in chosen if item is not None}
    ids = torch.as_tensor(np.asarray([c[0] for c in chosen], np.int32), device=dev)
    pos = torch.as_tensor(_state_pos(live, npad), device=dev)
    q = batch.query(ids, pos, actions=False)
    index = q.index.cpu().numpy()
    for k, (pid, item, s) in enumerate(chosen):  # every agent position of the region is the same node
        assert (index[k] == -1) if item is None else (maps[item][index[k]] == s)
    plans = batch.plans(q.index, ids, tie=tie, seed=seed, plan_cap=8)
    steps = [XR.plan(_case(NAMES[order][item])[1], s, 1, seed, k) if item is not None else None
             for k, (pid, item, s) in enumerate(chosen)]
    want_live, want_stored = [], []
    for k, (pid, item, s) in enumerate(chosen):
        if steps[k]:
            cp, t, _, _ = _case(NAMES[order][item])
            want_live += [(item, r) for r in XR.rows(cp, t, k, live[k], steps[k])]
            want_stored += [(item, r) for r in XR.rows(cp, t, k, None, steps[k])]
    T = len(want_live)
    assert T > 50 and T == int(plans.length.clamp(min=0).sum())
    rows = batch.demonstration_rows(plans, pos=pos, puzzle_id=ids)
    assert rows.num_rows == T and int(rows.dropped.view(torch.int32)[0]) == 0
    _check_rows(rows, want_live, maps, npad)
    rows = batch.demonstration_rows(plans, puzzle_id=ids)  # pos NULL: row 0 is the unpacked key
    assert rows.num_rows == T
    _check_rows(rows, want_stored, maps, npad)
    # half the capacity: the other half stays as it was and is counted
    half = T // 2
    sent = PushRows(_full((T,), torch.int32, dev), _full((T,), torch.int32, dev), _full((T,), torch.int32, dev),
                    _full((T, 2), torch.int8, dev), _full((T,), torch.uint8, dev), _full((T,), torch.int32, dev),
                    _full((T, npad, 2), torch.int8, dev), torch.zeros(1, dtype=torch.int32, device=dev), T)
    got = batch.demonstration_rows(plans, pos=pos, puzzle_id=ids, rows_cap=half, out=sent)
    _check_rows(got, want_live, maps, npad, cap=half)
    assert int(got.dropped[0]) == T - half
    for x in got[:7]:
        assert bool((x[half:] == SENT).all())
    # a plan_state outside its item is dropped and counted; a masked item and an item without a table write nothing
    bad = PushPlans(plans.push_from, plans.push_action, plans.state.clone(), plans.length)
    first = next(k for k in range(n) if steps[k])
    bad.state[first, 0] = 5000
    mask = torch.ones(n, dtype=torch.uint8, device=dev)
    other = next(k for k in range(first + 1, n) if steps[k])
    mask[other] = 0
    offset = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    torch.cumsum(plans.length.clamp(min=0), 0, out=offset[1:])
    sent = PushRows(*(x.fill_(SENT) if isinstance(x, torch.Tensor) else x for x in sent[:7]),
                    torch.zeros(1, dtype=torch.int32, device=dev), T)
    got = batch.demonstration_rows(bad, pos=pos, puzzle_id=ids, mask=mask, offset=offset, out=sent)
    assert int(got.dropped[0]) == 1
    skipped = torch.zeros(T, dtype=torch.bool, device=dev)
    skipped[int(offset[first])] = True
    skipped[int(offset[other]):int(offset[other + 1])] = True
    assert bool((got.t[skipped] == SENT).all()) and bool((got.t[~skipped] != SENT).all())


@pytest.mark.parametrize("order", ["A", "B"])
def test_emit(order):
    _check_emit(_batch(order, 0), order)


@pytest.mark.parametrize("npad", [8, 16, 32])
def test_sample_and_emit_padded(npad):
    """The same six cases in a set padded to 8, 16 and 32 (the 16-byte stores of the state writer, the live state's words beyond
    the key's four, zeros from a puzzle's movables on): the sample and the rows against the restatement, as at npad 4."""
    batch = _batch("B", 0, npad)
    _, drawn = _check_sample(batch, "B", (1, None), 21)
    assert drawn.sum() > 300
    _check_emit(batch, "B")


# ---- 5. end to end on generated puzzles -------------------------------------------------------------------------------------------
MIX, MIX_CAP, MIX_ENVS = 16, 2048, 256


def _mix():
    """The environment over 16 host-generated Level-0 puzzles, its indexed batch and the per-puzzle tables; made once."""
    if "mix" not in _SHARED:
        g, d = generate.generate_level0_grids(MIX, random_seed=21, device=-1)
        texts = [generate.grid_to_text(g[i], d[i, 0], d[i, 1]) for i in range(MIX)]
        vec = VecPushWorld([PushWorldPuzzle(text=x) for x in texts], MIX_ENVS, observation=None, max_steps=None, seed=4)
        batch = vec.push_tables(max_states_each=MIX_CAP, index=True)
        built = [i for i, s in enumerate(batch.status.cpu().tolist()) if s == TABLE_BUILT]
        tables = {i: vec.push_table(i, max_states=MIX_CAP) for i in built}
        assert len(built) >= 8 and batch.max_cost_stored == max(int(t.max_cost) for t in tables.values())
        _SHARED["mix"] = (vec, batch, tables)
    return _SHARED["mix"]


def test_reset_from_a_batch_and_solve():
    vec, batch, tables = _mix()
    B, dev = vec.num_envs, vec.device
    vec.reset_from_push_tables([batch], cost=(1, None), seed=6)
    covered = batch.covers(vec.puzzle_id)
    cost0 = vec.start_cost.clone()
    drawn = cost0 > 0
    # (a generated set is not filtered for solvability: an environment draws exactly where its puzzle's table has a cost >= 1)
    solvable = covered & (batch.max_cost[vec.puzzle_id.long()] >= 1)
    assert torch.equal(drawn, solvable) and int(drawn.sum()) >= 3 * (B // MIX) and bool((cost0[~solvable] == -1).all())
    draws = vec.table_draws.view(torch.int32)
    assert bool((draws[cost0 >= 0] == 1).all()) and bool((draws[cost0 < 0] == 0).all())
    assert bool((vec.steps == 0).all())
    q = vec.push_cost_to_go([batch])
    assert torch.equal(q.index[drawn], vec.start_row[drawn]) and torch.equal(q.cost[drawn], cost0[drawn])
    # the same draw from the per-puzzle tables is another STATE in general (their buckets are in store order): only the costs
    # are drawn from the same bands
    cost, pushes = q.cost.clone(), torch.zeros(B, dtype=torch.int32, device=dev)
    for _ in range(int(cost0.max())):
        live = drawn & (cost > 0)
        action = torch.where(live, q.push_action, torch.full_like(q.push_action, PUSH_NONE))
        _, _, term, _, _, status = vec.step_push(q.push_from.contiguous(), action.contiguous())
        assert bool((status[live] == _capi.PUSH_DONE).all())
        pushes += live
        q = vec.push_cost_to_go([batch])
        assert bool((q.cost[live] == cost[live] - 1).all()) and bool(((term[live] != 0) == (q.cost[live] == 0)).all())
        cost = q.cost.clone()
    assert bool((cost[drawn] == 0).all()) and torch.equal(pushes[drawn], cost0[drawn])  # solved in exactly start_cost pushes
    # a band per environment, a mask, and the counters: a second reset draws with the counters advanced
    band = torch.as_tensor(((np.arange(B) // MIX) % 4).astype(np.int32), device=dev)  # (every puzzle gets every band)
    again = (band == 2)
    before = vec.pos.clone()
    vec.reset_from_push_tables([batch], cost=(band, band), mask=again)
    assert torch.equal(vec.pos[~again], before[~again])
    took = again & (vec.start_cost >= 0)
    assert torch.equal(took, again & solvable) and int(took.sum()) >= 8 and bool((vec.start_cost[took] <= 2).all())
    assert bool((vec.table_draws.view(torch.int32)[took & drawn] == 2).all())


@pytest.mark.parametrize("tie", ["lowest", "uniform"])
def test_demonstrations_equal_the_per_table_ones(tie):
    vec, batch, tables = _mix()
    B, dev = vec.num_envs, vec.device
    vec.reset_from_push_tables([batch], cost=(1, None), seed=8)
    rng = np.random.default_rng(3)
    for _ in range(3):  # a few random moves: live states off the canonical ones
        vec.step(torch.as_tensor(rng.integers(0, 4, B).astype(np.uint8), device=dev))
    start = vec.pos.clone()
    mask = torch.ones(B, dtype=torch.uint8, device=dev)
    mask[5] = 0
    d = vec.optimal_push_demonstrations([batch], tie=tie, seed=4, mask=mask, observation=None)
    ref = vec.optimal_push_demonstrations(list(tables.values()), tie=tie, seed=4, mask=mask, observation=None)
    assert d.num_rows == ref.num_rows > B // 4 and int((d.item == 5).sum()) == 0
    for name in ("item", "t", "pos", "push_from", "push_action", "cost", "choice", "puzzle_id"):  # (state: each numbers its own)
        assert torch.equal(getattr(d, name), getattr(ref, name)), name
    # the rows' states are the nodes: looked up in the batch they give the row's state number and cost
    q = batch.query(d.puzzle_id, d.pos, actions=False)
    assert torch.equal(q.index, d.state) and torch.equal(q.cost, d.cost)
    # step_push(choice=...) from the first rows lowers the cost by 1
    first = d.t == 0
    env = d.item[first].long()
    assert torch.equal(d.pos[first], start[env])  # (row 0 of an environment is its live state)
    choice = torch.full((B,), -1, dtype=torch.int64, device=dev)
    choice[env] = d.choice[first]
    *_, status = vec.step_push(choice=choice)
    has = torch.zeros(B, dtype=torch.bool, device=dev)
    has[env] = True
    assert int(has.sum()) >= B // MIX and bool((status[has] == _capi.PUSH_DONE).all()) and bool((status[~has] == _capi.PUSH_REFUSED).all())
    after = vec.push_cost_to_go([batch]).cost
    assert torch.equal(after[env], d.cost[first] - 1)
    second = torch.nonzero(d.t == 1).squeeze(1)  # the state after the first push is the second row's
    assert second.numel() > 0 and torch.equal(vec.pos[d.item[second].long()], d.pos[second])


def test_fewest_push_plans_equal_the_per_table_ones():
    vec, batch, tables = _mix()
    vec.reset_from_push_tables([batch], cost=(1, None), seed=9)
    r = vec.fewest_push_plans([batch])
    ref = vec.fewest_push_plans(list(tables.values()))
    assert torch.equal(r.plans, ref.plans) and torch.equal(r.plan_len, ref.plan_len) and torch.equal(r.pushes, ref.pushes)
    ok = r.plan_len > 0
    assert int(ok.sum()) >= 3 * (vec.num_envs // MIX) and torch.equal(r.pushes[ok], vec.start_cost[ok]) and int(r.plan_len.max()) <= 1024
    verdict = replay_plans(vec, vec.puzzle_id, r.plans, r.plan_len, pos=vec.pos, mask=ok.to(torch.uint8), rows=False).verdict
    assert bool((verdict[ok] == REPLAY_VALID).all())


def test_a_mixed_list_of_a_batch_and_a_table():
    vec, batch, tables = _mix()
    B = vec.num_envs
    odd = next(i for i in range(1, MIX, 2) if i in tables and int(tables[i].max_cost) >= 1)
    with vec.push_tables(list(range(0, MIX, 2)), max_states_each=MIX_CAP, index=True) as even:
        ids = vec.puzzle_id
        own = ((ids % 2 == 0) & even.covers(ids)) | (ids == odd)
        assert int((ids == odd).sum()) > 0 and int(own.sum()) > int((ids == odd).sum()) and int((~own).sum()) > 0
        mixed = [even, tables[odd]]
        # reset: the batch's environments draw what the whole batch draws (the same puzzle, start, seed, environment and count)
        vec.reset_from_push_tables([batch], cost=(1, None), seed=12)
        whole_pos, whole_cost = vec.pos.clone(), vec.start_cost.clone()
        vec.reset_from_push_tables(mixed, cost=(1, None), seed=12)
        in_even = own & (ids != odd)
        assert torch.equal(vec.pos[in_even], whole_pos[in_even]) and torch.equal(vec.start_cost[in_even], whole_cost[in_even])
        assert bool((vec.start_cost[~own] == -1).all()) and bool((vec.start_cost[ids == odd] >= 1).all())
        # demonstrations and plans from these states: on the list's own environments what the whole batch gives
        d = vec.optimal_push_demonstrations(mixed, observation=None)
        ref = vec.optimal_push_demonstrations([batch], observation=None)
        keep = own[ref.item.long()]
        assert d.num_rows == int(keep.sum()) > 0 and bool(own[d.item.long()].all())
        for name in ("item", "t", "pos", "push_from", "push_action", "cost", "choice"):
            assert torch.equal(getattr(d, name), getattr(ref, name)[keep]), name
        r, whole = vec.fewest_push_plans(mixed), vec.fewest_push_plans([batch])
        assert torch.equal(r.plan_len[own], whole.plan_len[own]) and torch.equal(r.plans[own], whole.plans[own])
        assert bool((r.plan_len[~own] == -1).all()) and int((r.plan_len[own] > 0).sum()) >= 2 * (B // MIX)
    other = VecPushWorld([PushWorldPuzzle(text=deep_puzzles.corridor(7))], 2, observation=None, max_steps=None)
    with other.push_tables(max_states_each=64, index=True) as foreign:
        for call in (vec.reset_from_push_tables, vec.optimal_push_demonstrations, vec.fewest_push_plans):
            with pytest.raises(ValueError, match="made on this environment"):
                call([foreign])


# ---- 6. capture -------------------------------------------------------------------------------------------------------------------
def test_capture_sample_and_plans():
    """The sample and the plans allocate nothing and do not synchronise: each captured once, replayed twice on states that move
    on (the counters advance, the plans start from what the sample drew)."""
    order = "B"
    batch = _batch(order, 0)
    dev, n = batch.device, 512
    ids = torch.as_tensor((np.arange(n) % 6).astype(np.int32), device=dev)
    pos, steps = torch.zeros((n, batch.npad, 2), dtype=torch.int8, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)
    counter = torch.zeros(n, dtype=torch.int32, device=dev)
    out = (torch.full((n,), -1, dtype=torch.int32, device=dev), torch.full((n,), -1, dtype=torch.int32, device=dev))
    index = torch.zeros(n, dtype=torch.int32, device=dev)
    plans = PushPlans(torch.zeros((n, 8, 2), dtype=torch.int8, device=dev), torch.zeros((n, 8), dtype=torch.uint8, device=dev),
                      torch.zeros((n, 8), dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    g_sample, g_plans = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(g_sample):
        batch.sample(ids, pos, steps, cost=(1, None), seed=13, counter=counter, out=out)
    with torch.cuda.graph(g_plans):
        batch.plans(index, ids, tie="uniform", seed=2, plan_cap=8, out=plans)
    counter.zero_()
    has = torch.as_tensor(np.array([_item_of(int(p)) is not None for p in ids.cpu().tolist()]), device=dev)
    last = None
    for replay in (1, 2):
        g_sample.replay()
        index.copy_(out[0])
        g_plans.replay()
        torch.cuda.synchronize()
        assert counter.cpu().tolist() == [replay if h else 0 for h in has.cpu().tolist()]
        state = out[0].cpu().numpy()
        for i in range(0, n, 7):
            item = _item_of(int(ids[i]))
            if item is not None:
                sbc, cs = _case(NAMES[order][item])[3]
                assert _map(batch, order, item)[state[i]] == XR.draw_state(13, i, replay, 1, 1 << 30, sbc, cs)
        # the eager calls with the same counters give the same words
        e_pos, e_steps = torch.zeros_like(pos), torch.zeros_like(steps)
        e_ctr = torch.where(has, torch.full_like(counter, replay - 1), torch.zeros_like(counter))
        e_state, e_cost = batch.sample(ids, e_pos, e_steps, cost=(1, None), seed=13, counter=e_ctr)
        assert torch.equal(e_state, out[0]) and torch.equal(e_cost, out[1]) and torch.equal(e_pos, pos)
        eager = batch.plans(index, ids, tie="uniform", seed=2, plan_cap=8)
        live = torch.arange(8, device=dev).unsqueeze(0) < plans.length.unsqueeze(1)
        assert torch.equal(eager.length[has], plans.length[has]) and torch.equal(plans.length[has], out[1][has])
        assert torch.equal(eager.state[live], plans.state[live]) and torch.equal(eager.push_action[live], plans.push_action[live])
        assert torch.equal(eager.push_from[live], plans.push_from[live]) and int(live.sum()) > n
        assert last is None or not torch.equal(last, pos)  # the states moved on
        last = pos.clone()

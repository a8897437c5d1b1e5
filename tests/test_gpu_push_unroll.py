"""Pushes unrolled into primitive actions on the device (pw_push_unroll_count / _write / _plans, search.unroll_pushes /
push_rows_to_plans, VecPushWorld.fewest_push_plans, PushSolutionTable.primitive_plans) against the restatement
of tests/push_unroll_restatement.py, against the parent actions of pw_walk_regions' own maps, against pw_step_push and pw_step,
and end to end through the plan replay's verdicts."""
import numpy as np
import pytest
import torch

import deep_puzzles
import push_table_restatement as TR
import push_unroll_restatement as UR
import shape_states
import walk_restatement as WR
from oracle import c_oracle
from pushworld_amd import _capi
from pushworld_amd.puzzle import PushWorldPuzzle
from pushworld_amd.search import PUSH_NONE, REPLAY_CUT, REPLAY_VALID, PushSolutionTable, replay_plans, unroll_pushes, walk_regions
from pushworld_amd.vec_env import VecPushWorld
from test_gpu_push_step import _first_rows, _level1_vec, _serpentine_region

pytestmark = pytest.mark.gpu

NAMES = list(TR.EXPECT)
SENT = 0xEE  # what every byte around and inside `actions` holds before a launch
GUARD = 64


def _pos(states, npad):
    pos = np.zeros((len(states), npad, 2), np.int8)
    for i, s in enumerate(states):
        pos[i, :len(s)] = np.asarray(s, np.int64).astype(np.int8)
    return pos


def _run(engine, ids, pos, frm, act, mask=None):
    """count and write over device tensors with sentinels in and around every output, then write again with half the capacity:
    (length, offset, actions) as numpy arrays."""
    dev, n = engine.device, int(ids.shape[0])
    length = torch.full((n,), -7, dtype=torch.int32, device=dev)
    offset = torch.full((n + 1,), -7, dtype=torch.int64, device=dev)
    engine.push_unroll_count(ids, pos, frm, act, mask, length, offset)
    off = offset.cpu().numpy()
    total = int(off[n])
    ln = length.cpu().numpy()
    assert off[0] == 0 and (np.diff(off) == np.maximum(ln, 0)).all()
    buf = torch.full((total + 2 * GUARD,), SENT, dtype=torch.uint8, device=dev)
    dropped = torch.full((1,), -7, dtype=torch.int64, device=dev)
    engine.push_unroll_write(ids, pos, frm, act, mask, offset, total, buf[GUARD:GUARD + total], dropped)
    got = buf.cpu().numpy()
    assert (got[:GUARD] == SENT).all() and (got[GUARD + total:] == SENT).all() and int(dropped[0]) == 0
    actions = got[GUARD:GUARD + total]
    assert (actions <= 3).all()  # every byte of every span was written
    half = total // 2
    buf2 = torch.full((total + 2 * GUARD,), SENT, dtype=torch.uint8, device=dev)
    engine.push_unroll_write(ids, pos, frm, act, mask, offset, half, buf2[GUARD:GUARD + half], dropped)
    got2 = buf2.cpu().numpy()
    assert (got2[GUARD:GUARD + half] == actions[:half]).all() and (got2[GUARD + half:] == SENT).all() and (got2[:GUARD] == SENT).all()
    assert int(dropped[0]) == total - half
    return ln, off, actions


def _check(engine, cps, items, npad):
    """``items``: (puzzle id, state, (frm, action), mask bit, region or None).  Every length, offset and action byte against the
    restatement."""
    dev = engine.device
    ids = torch.as_tensor(np.asarray([it[0] for it in items], np.int32), device=dev)
    pos = torch.as_tensor(_pos([it[1] for it in items], npad), device=dev)
    frm = torch.as_tensor(np.asarray([it[2][0] for it in items], np.int64).astype(np.int8).reshape(-1, 2), device=dev)
    act = torch.as_tensor(np.asarray([it[2][1] for it in items], np.uint8), device=dev)
    bits = [it[3] for it in items]
    mask = None if all(bits) else torch.as_tensor(np.asarray(bits, np.uint8), device=dev)
    seqs = [UR.unroll(cps[it[0]] if 0 <= it[0] < len(cps) else None, it[1], it[2][0], it[2][1], masked=not it[3], reg=it[4])
            for it in items]
    w_len, w_off, w_act = UR.flatten(seqs)
    ln, off, actions = _run(engine, ids, pos, frm, act, mask)
    assert ln.tolist() == w_len, [(i, a, b) for i, (a, b) in enumerate(zip(ln.tolist(), w_len)) if a != b][:5]
    assert off.tolist() == w_off and actions.tolist() == w_act
    return seqs


def _invalid_items(pid, cp, state, reg, n_puzzles):
    """One refused item of every kind from ``state`` (a kind the state has no example of is left out), with the kinds' names."""
    state = tuple(tuple(xy) for xy in state)
    out = []
    outside = next(((x, y) for y in range(cp.height) for x in range(cp.width) if (x, y) not in reg.dist), None)
    steps = WR._steps(cp, state[1:])
    walk = next(((q, a) for (q, a), (_, moved) in sorted(steps.items()) if q in reg.dist and list(moved) == [0]), None)
    still = next(((q, a) for (q, a), (_, moved) in sorted(steps.items()) if q in reg.dist and len(moved) == 0), None)
    if outside is not None:
        out.append(("outside R", (pid, state, (outside, 1), 1, reg)))
    if walk is not None:
        out.append(("a walk move", (pid, state, walk, 1, reg)))
    if still is not None:
        out.append(("displaces nothing", (pid, state, still, 1, reg)))
    q0 = state[0]
    out.append(("outside the grid", (pid, state, ((cp.width, 1), 1), 1, reg)))
    out.append(("negative", (pid, state, ((-1, -128), 1), 1, reg)))
    if reg.pushes:
        pm = reg.pushes[0]
        out.append(("action 4", (pid, state, (pm.frm, 4), 1, reg)))
        out.append(("PUSH_NONE", (pid, state, (pm.frm, PUSH_NONE), 1, reg)))
        out.append(("masked", (pid, state, (pm.frm, pm.action), 0, reg)))
        out.append(("id outside the set", (n_puzzles, state, (pm.frm, pm.action), 1, None)))
        out.append(("id outside the set", (-1, state, (pm.frm, pm.action), 1, None)))
        bad = list(state)
        bad[-1] = (cp.width, bad[-1][1])
        out.append(("a movable outside its grid", (pid, tuple(bad), (pm.frm, pm.action), 1, None)))
    else:
        out.append(("PUSH_NONE", (pid, state, (q0, PUSH_NONE), 1, reg)))
    return out


def _paths_from_maps(reg, rows, offset, total):
    """Every row's L out of pw_walk_regions' own maps, with torch on the device: the definition of path(R, from)."""
    dev = rows.item.device
    wm = reg.walk_map.view(torch.int16).to(torch.int64) & 0xFFFF
    item, x, y = rows.item.long(), rows.frm[:, 0].long(), rows.frm[:, 1].long()
    out = torch.full((total,), SENT, dtype=torch.uint8, device=dev)
    base = offset[:-1]
    out[base + rows.walk.long()] = rows.action
    dx = torch.tensor([-1, 1, 0, 0], device=dev)
    dy = torch.tensor([0, 0, -1, 1], device=dev)
    for _ in range(int(rows.walk.max()) if rows.num_rows else 0):
        e = wm[item, y, x]
        d, a = e & 0xFFF, e >> 12
        on = (d > 0) & (e != 0xFFFF)
        out[(base + d - 1)[on]] = a[on].to(torch.uint8)
        x = torch.where(on, x - dx[a & 3], x)
        y = torch.where(on, y - dy[a & 3], y)
    return out


# ---- 1. the ten table cases -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_table_cases(name):
    text, cp, start, t = TR.case(name)
    with PushSolutionTable(PushWorldPuzzle(text=text), start=start) as tab:
        engine, dev, npad = tab.search._engine, tab.device, tab.npad
        S = tab.num_states
        assert S == t.info[0]
        stored = tab.states()[0]
        assert tab.puzzle_index == 0
        ids = torch.zeros(S, dtype=torch.int32, device=dev)
        reg = walk_regions(engine, ids, stored, maps=True)
        rows = reg.pushes()
        T = rows.num_rows
        assert T == t.info[1]
        # (a) every push row that pw_walk_pushes lists from the stored states, as the wrapper takes them: the length is the
        # row's walk + 1, the bytes are the parent actions of pw_walk_regions' own map followed by the push
        row_pos = stored[rows.item.long()].contiguous()
        row_ids = torch.zeros(T, dtype=torch.int32, device=dev)
        u = unroll_pushes(engine, row_ids, rows.frm, rows.action, pos=row_pos)
        assert torch.equal(u.length, rows.walk + 1) and u.num_actions == int((rows.walk + 1).sum())
        assert torch.equal(u.actions, _paths_from_maps(reg, rows, u.offset, u.num_actions))
        # (b) every push row of every stored state and one refused choice of every kind, against the restatement
        assert (stored.cpu().numpy() == _pos(t.store.states, npad)).all()
        items, kinds = [], set()
        for i in range(S):
            state = t.store.states[i]
            r = WR.region(cp, state)
            items += [(0, state, (pm.frm, pm.action), 1, r) for pm in r.pushes]
            if i == 0:
                bad = _invalid_items(0, cp, state, r, 1)
                kinds = {k for k, _ in bad}
                items += [it for _, it in bad]
        assert {"outside R", "outside the grid", "PUSH_NONE"} <= kinds
        seqs = _check(engine, [cp], items, npad)
        assert sum(s is not None for s in seqs) == T and sum(s is None for s in seqs) >= len(kinds)


# ---- 2. the longest walk in the suite --------------------------------------------------------------------------------------------
def test_longest_walk():
    cp, reg = _serpentine_region()
    assert len(reg.pushes) == 1 and reg.pushes[0].walk == 1948
    pm = reg.pushes[0]
    vec = VecPushWorld([PushWorldPuzzle(text=deep_puzzles.serpentine(62, 61))], 1, observation=None, max_steps=None)
    s0 = cp.initial_state
    items = [(0, s0, (pm.frm, pm.action), 1, reg), (0, s0, (pm.frm, pm.action ^ 1), 1, reg), (0, s0, (pm.frm, pm.action), 1, reg)]
    seqs = _check(vec.engine, [cp], items, vec.num_objects_padded)
    assert len(seqs[0]) == 1949 and seqs[1] is None and seqs[2] == seqs[0]
    # NULL pos is the initial state
    dev = vec.device
    u = unroll_pushes(vec, torch.zeros(1, dtype=torch.int32, device=dev),
                      torch.as_tensor(np.asarray([pm.frm], np.int8), device=dev),
                      torch.as_tensor(np.asarray([pm.action], np.uint8), device=dev))
    assert u.num_actions == 1949 and u.actions.cpu().tolist() == seqs[0]


# ---- 3. shape limits -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", shape_states.CASES, ids=[str(c) for c in shape_states.CASES])
def test_shapes_and_overlapping_states(case):
    cp = shape_states.puzzle(case)
    vec = VecPushWorld([PushWorldPuzzle(text=shape_states.text(case))], 1, observation=None, max_steps=None)
    assert vec.num_objects_padded == shape_states.PADDING[case]
    listed = shape_states.states(case)
    items = []
    for k, ls in enumerate(listed):
        reg = shape_states.region(case, ls.state)
        items += [(0, ls.state, (pm.frm, pm.action), 1, reg) for pm in reg.pushes]
        if k < 3:
            items += [it for _, it in _invalid_items(0, cp, ls.state, reg, 1)]
    assert any(shape_states.overlapping(cp, it[1]) and it[4] is not None and it[4].pushes for it in items)
    seqs = _check(vec.engine, [cp], items, vec.num_objects_padded)
    assert sum(s is not None for s in seqs) > 20 and any(s is None for s in seqs) and max(len(s) for s in seqs if s) > 3


@pytest.mark.parametrize("tables", ["all", "big", "none"])
@pytest.mark.parametrize("npad, index", [(4, 0), (8, 1), (16, 1), (32, 2)])
def test_big_padded(npad, index, tables):
    """`big` as puzzle `index` of a set padded to `npad` by puzzles with more movables, under the three forms of the step tables."""
    _, cp, _, t = TR.case("big")
    extra = {4: None, 8: 4, 16: 10, 32: deep_puzzles.POCKETS_EXTRA}[npad]
    texts = [deep_puzzles.pockets(extra)] * max(index, 1) if extra else []
    texts.insert(index, deep_puzzles.big())
    cps = [cp if k == index else c_oracle.COraclePuzzle(x) for k, x in enumerate(texts)]
    vec = VecPushWorld([PushWorldPuzzle(text=x) for x in texts], len(texts), observation=None, max_steps=None,
                       engine_options={"step_tables": tables})
    assert vec.num_objects_padded == npad
    items = []
    for i in range(0, t.info[0], 60):
        state = t.store.states[i]
        reg = WR.region(cp, state)
        items += [(index, state, (pm.frm, pm.action), 1, reg) for pm in reg.pushes]
    for pid, c in enumerate(cps):  # the other puzzles of the set too, from their initial states
        if pid != index:
            reg = WR.region(c, c.initial_state)
            items += [(pid, c.initial_state, (pm.frm, pm.action), 1, reg) for pm in reg.pushes]
    items += [it for _, it in _invalid_items(index, cp, t.store.states[0], WR.region(cp, t.store.states[0]), len(texts))]
    seqs = _check(vec.engine, cps, items, npad)
    assert sum(s is not None for s in seqs) > 50


# ---- 4. agreement with pw_step_push and pw_step -----------------------------------------------------------------------------------
def test_agreement_with_step_push_and_step():
    B = 64
    cps, vec = _level1_vec(B, max_steps=None)
    _, twin = _level1_vec(B, max_steps=None)
    vec.reset()
    twin.reset()
    dev = vec.device
    gen = torch.Generator().manual_seed(5)
    for _ in range(6):
        a = torch.randint(0, 4, (B,), generator=gen, dtype=torch.uint8).to(dev)
        vec.step(a)
        twin.step(a)
    assert torch.equal(vec.pos, twin.pos) and not bool(vec.terminated.any())
    frm, act = _first_rows(vec)
    act[3], act[9] = PUSH_NONE, 4                       # refused choices among the valid ones
    frm[11] = 0                                         # the border wall: outside every region
    u = unroll_pushes(vec, vec.puzzle_id, frm, act, pos=vec.pos)
    assert u.num_actions == int(u.length.clamp(min=0).sum()) and int((u.length > 0).sum()) > B // 2
    _, _, _, _, moves, status = vec.step_push(frm, act)
    assert torch.equal(moves, u.length.clamp(min=0))
    assert torch.equal(status == _capi.PUSH_REFUSED, u.length == -1) and bool((status[u.length > 0] == _capi.PUSH_DONE).all())
    assert [int(u.length[k]) for k in (3, 9, 11)] == [-1, -1, -1]
    # the twin batch stepped by pw_step, one launch per action of L (an environment whose L has ended is put back)
    longest = int(u.length.max())
    assert 1 < longest < 64
    for k in range(longest):
        on = u.length > k
        at = (u.offset[:-1] + k).clamp(max=u.num_actions - 1)
        action = torch.where(on, u.actions[at], torch.zeros_like(u.actions[at]))
        before = twin.pos.clone()
        twin.step(action.contiguous())
        twin.pos.copy_(torch.where(on[:, None, None], twin.pos, before))
    assert torch.equal(twin.pos, vec.pos)


# ---- 5. end to end on `big` --------------------------------------------------------------------------------------------------------
def _restated_plans(cp, d, B):
    """Per environment the concatenated restated L of its emitted rows (``d``: optimal_push_demonstrations' namespace)."""
    item, frm, act = d.item.cpu().tolist(), d.push_from.cpu().tolist(), d.push_action.cpu().tolist()
    pos = d.pos.cpu().numpy()
    out = [[] for _ in range(B)]
    walks = [0] * B
    for r in range(d.num_rows):
        state = tuple(tuple(int(v) for v in xy) for xy in pos[r, :cp.num_movables])
        reg = WR.region(cp, state)
        seq = UR.unroll(cp, state, frm[r], act[r], reg=reg)
        assert seq is not None and len(seq) == reg.dist[tuple(frm[r])] + 1
        out[item[r]] += seq
        walks[item[r]] += reg.dist[tuple(frm[r])] + 1
    return out, walks


def test_end_to_end_on_big():
    _, cp, _, t = TR.case("big")
    B = 270
    vec = VecPushWorld([PushWorldPuzzle(text=deep_puzzles.big())], B, observation=None, max_steps=None, seed=9)
    dev = vec.device
    with vec.push_table(0) as tab:
        band = torch.as_tensor((np.arange(B) % 9).astype(np.int32), device=dev)
        vec.reset_from_push_tables([tab], cost=(band, band))
        dead = [i for i, c in enumerate(t.cost) if c == -1][:5]
        for k, i in enumerate(dead):  # a few dead ends among them
            vec.pos[200 + k, :3] = torch.as_tensor(np.asarray(t.store.states[i], np.int8), device=dev)
        q = vec.push_cost_to_go([tab])
        cost = q.cost.clone()
        assert set(cost.cpu().tolist()) == set(range(-1, 9))  # all 8 costs, goal states and dead ends
        mask = torch.ones(B, dtype=torch.uint8, device=dev)
        mask[17] = 0
        live = (cost >= 0) & (mask != 0)
        r = vec.fewest_push_plans([tab], mask=mask)
        assert r.plans.shape == (B, 1024) and r.plans.dtype == torch.uint8 and r.plan_len.dtype == r.pushes.dtype == torch.int32
        assert bool((r.plan_len[~live] == -1).all()) and bool((r.pushes[~live] == 0).all())
        assert torch.equal(r.pushes[live], cost[live]) and bool((r.plan_len[cost == 0] == 0).all())
        assert bool((r.plan_len[live & (cost > 0)] >= cost[live & (cost > 0)]).all())
        # the reference's verdict, from the live states
        rep = replay_plans(vec, vec.puzzle_id, r.plans, r.plan_len, pos=vec.pos, rows=False)
        assert bool((rep.verdict[live] == REPLAY_VALID).all()) and torch.equal(rep.first_goal[live], r.plan_len[live])
        assert bool((rep.verdict[~live] == _capi.REPLAY_NONE).all())
        # every byte: the restated walks of the emitted rows, concatenated
        d = vec.optimal_push_demonstrations([tab], observation=None, mask=mask)
        want, walks = _restated_plans(cp, d, B)
        plans, plan_len = r.plans.cpu().numpy(), r.plan_len.cpu().tolist()
        for e in range(B):
            if bool(live[e]):
                assert plan_len[e] == walks[e] == len(want[e]) and plans[e, :plan_len[e]].tolist() == want[e], e
                assert (plans[e, plan_len[e]:] == 0).all()
        # the table's own entry point gives the same arrays
        p2, l2, n2 = tab.primitive_plans(vec.pos, puzzle_id=vec.puzzle_id, mask=mask)
        assert torch.equal(p2, r.plans) and torch.equal(l2, r.plan_len) and torch.equal(n2, r.pushes)
        # every step of every plan as a primitive demonstration row
        full = replay_plans(vec, vec.puzzle_id, r.plans, r.plan_len, pos=vec.pos)
        assert full.num_rows == int(r.plan_len.clamp(min=0).sum()) and int(full.done.sum()) == int((live & (cost > 0)).sum())
        # a plan_cap one short of the longest plan: CUT for exactly those plans
        longest = int(r.plan_len.max())
        short = vec.fewest_push_plans([tab], mask=mask, plan_cap=longest - 1)
        assert torch.equal(short.plan_len, r.plan_len) and torch.equal(short.plans, r.plans[:, :longest - 1])
        rep = replay_plans(vec, vec.puzzle_id, short.plans, short.plan_len, pos=vec.pos, rows=False)
        assert torch.equal(rep.verdict == REPLAY_CUT, r.plan_len == longest) and int((rep.verdict == REPLAY_CUT).sum()) > 0
        assert bool((rep.verdict[live & (r.plan_len < longest)] == REPLAY_VALID).all())
        # a push_cap one short of the largest cost: no plan for exactly those environments
        fewer = vec.fewest_push_plans([tab], mask=mask, push_cap=7)
        assert torch.equal(fewer.plan_len == -1, ~live | (cost == 8)) and int((live & (cost == 8)).sum()) > 0
        keep = live & (cost < 8)
        assert torch.equal(fewer.plan_len[keep], r.plan_len[keep]) and torch.equal(fewer.plans[keep], r.plans[keep])
        # ---- tie rules: other optimal rows, plans as valid and as many pushes
        for seed in (3, 4):
            u = vec.fewest_push_plans([tab], tie="uniform", seed=seed, mask=mask)
            rep = replay_plans(vec, vec.puzzle_id, u.plans, u.plan_len, pos=vec.pos, rows=False)
            assert bool((rep.verdict[live] == REPLAY_VALID).all()) and torch.equal(rep.first_goal[live], u.plan_len[live])
            assert torch.equal(u.pushes, r.pushes) and bool((u.plan_len[~live] == -1).all())
        assert not torch.equal(u.plans, r.plans)


def test_two_tables_and_a_foreign_puzzle():
    names = ["big", "serpentine 14x13 overshoot"]
    cases = [TR.case(k) for k in names]
    B = 64
    vec = VecPushWorld([PushWorldPuzzle(text=c[0]) for c in cases], B, observation=None, max_steps=None, seed=3)
    with vec.push_table(0) as t0, vec.push_table(1) as t1:
        vec.reset_from_push_tables([t0, t1], cost=(0, None))
        ids = vec.puzzle_id
        assert set(ids.cpu().tolist()) == {0, 1}
        cost = vec.push_cost_to_go([t0, t1]).cost
        assert bool((cost >= 0).all())
        r = vec.fewest_push_plans([t0, t1], plan_cap=256)
        rep = replay_plans(vec, ids, r.plans, r.plan_len, pos=vec.pos, rows=False)
        assert bool((rep.verdict == REPLAY_VALID).all()) and torch.equal(rep.first_goal, r.plan_len)
        assert torch.equal(r.pushes, cost) and bool((r.plan_len[cost == 0] == 0).all())
        assert int(r.plan_len[ids == 1].max()) > 50  # the walk along the serpentine
        only0 = vec.fewest_push_plans([t0], plan_cap=256)  # puzzle 1 is foreign to the only table
        assert bool((only0.plan_len[ids == 1] == -1).all()) and torch.equal(only0.plan_len[ids == 0], r.plan_len[ids == 0])
        assert torch.equal(only0.plans[ids == 0], r.plans[ids == 0]) and bool((only0.pushes[ids == 1] == 0).all())
        with PushSolutionTable(PushWorldPuzzle(text=cases[0][0])) as foreign:
            with pytest.raises(ValueError, match="made on this environment"):
                vec.fewest_push_plans([foreign])


def test_gather_refuses_and_cuts():
    """pw_push_unroll_plans by itself over hand-made rows of corridor(7): the restatement of the concatenation."""
    cp = c_oracle.COraclePuzzle(deep_puzzles.corridor(7))
    vec = VecPushWorld([PushWorldPuzzle(text=deep_puzzles.corridor(7))], 1, observation=None, max_steps=None)
    dev, npad = vec.device, vec.num_objects_padded
    s0, s1, s2 = cp.initial_state, ((5, 1), (6, 1)), ((7, 1), (5, 1))
    choices = [(s0, (4, 1), 1), (s0, (4, 1), 0), (s1, (5, 1), 1), (s2, (6, 1), 0), (s0, (0, 0), PUSH_NONE), (s0, (4, 1), 1)]
    seqs = [UR.unroll(cp, s, f, a) for s, f, a in choices]
    item_offset = [0, 2, 4, 4, 5, 6, 6]
    T = len(choices)
    ids = torch.zeros(T, dtype=torch.int32, device=dev)
    pos = torch.as_tensor(_pos([c[0] for c in choices], npad), device=dev)
    frm = torch.as_tensor(np.asarray([c[1] for c in choices], np.int8), device=dev)
    act = torch.as_tensor(np.asarray([c[2] for c in choices], np.uint8), device=dev)
    u = unroll_pushes(vec, ids, frm, act, pos=pos)
    assert (u.length.cpu().tolist(), u.offset.cpu().tolist(), u.actions.cpu().tolist()) == UR.flatten(seqs)
    off = torch.as_tensor(np.asarray(item_offset, np.int64), device=dev)
    m = len(item_offset) - 1
    for plan_cap in (2, 3, 8):
        plans = torch.full((m, plan_cap), SENT, dtype=torch.uint8, device=dev)
        plan_len = torch.full((m,), -7, dtype=torch.int32, device=dev)
        vec.engine.push_unroll_plans(off, u.length, u.offset, u.actions, T, u.num_actions, plans, plan_len)
        w_plans, w_len = UR.plans(item_offset, seqs, plan_cap)
        assert plan_len.cpu().tolist() == w_len == [-1, 3, 0, -1, 4, 0]
        for j, w in enumerate(w_plans):
            assert plans[j].cpu().tolist() == w + [SENT] * (plan_cap - len(w))
    # rows outside 0 .. T, and bytes the writing call dropped: no plan
    wild = torch.as_tensor(np.asarray([0, 1, 9, 2, 3], np.int64), device=dev)
    plans = torch.full((4, 8), SENT, dtype=torch.uint8, device=dev)
    plan_len = torch.full((4,), -7, dtype=torch.int32, device=dev)
    vec.engine.push_unroll_plans(wild, u.length, u.offset, u.actions, T, u.num_actions, plans, plan_len)
    assert plan_len.cpu().tolist() == [4, -1, -1, 1]
    plans = torch.full((m, 8), SENT, dtype=torch.uint8, device=dev)
    plan_len = torch.full((m,), -7, dtype=torch.int32, device=dev)
    vec.engine.push_unroll_plans(off, u.length, u.offset, u.actions, T, 7, plans, plan_len)  # (the last span lies beyond 7 bytes)
    assert plan_len.cpu().tolist() == [-1, 3, 0, -1, -1, 0] and plans[1, :3].cpu().tolist() == [1, 0, 0]
    assert bool((plans[4] == SENT).all())


# ---- 6. room3 -------------------------------------------------------------------------------------------------------------------
def test_room3():
    B = 4096
    vec = VecPushWorld([PushWorldPuzzle(text=deep_puzzles.room3())], B, observation=None, max_steps=None, seed=5)
    with vec.push_table(0, max_states=1 << 16) as tab:
        assert tab.info == (42840, 316176, 1190, 15778, 10)
        vec.reset_from_push_tables([tab], cost=(0, None))
        cost = vec.start_cost
        assert int(cost.min()) == 0 and int(cost.max()) > 5
        r = vec.fewest_push_plans([tab])
        rep = replay_plans(vec, vec.puzzle_id, r.plans, r.plan_len, pos=vec.pos, rows=False)
        assert bool((rep.verdict == REPLAY_VALID).all()) and torch.equal(rep.first_goal, r.plan_len)
        assert torch.equal(r.pushes, cost) and bool((r.plan_len >= cost).all()) and int(r.plan_len.max()) < 1024


# ---- 7. capture -----------------------------------------------------------------------------------------------------------------
def test_captured_count_and_write_equal_eager():
    B = 256
    cps, vec = _level1_vec(B, max_steps=None)
    vec.reset()
    dev = vec.device
    gen = torch.Generator().manual_seed(8)
    for _ in range(5):
        vec.step(torch.randint(0, 4, (B,), generator=gen, dtype=torch.uint8).to(dev))
    engine = vec.engine
    frm, act = _first_rows(vec)
    pos = vec.pos.clone()
    eager = unroll_pushes(vec, vec.puzzle_id, frm, act, pos=pos)  # (also the warm-up: the first call sizes the workspace)
    cap = eager.num_actions
    assert cap > B
    length = torch.zeros(B, dtype=torch.int32, device=dev)
    offset = torch.zeros(B + 1, dtype=torch.int64, device=dev)
    actions = torch.zeros(cap, dtype=torch.uint8, device=dev)
    dropped = torch.zeros(1, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    g_count, g_write = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(g_count):
        engine.push_unroll_count(vec.puzzle_id, pos, frm, act, None, length, offset)
    with torch.cuda.graph(g_write):
        engine.push_unroll_write(vec.puzzle_id, pos, frm, act, None, offset, cap, actions, dropped)
    for replay in range(2):
        length.fill_(-7), offset.fill_(-7), actions.fill_(SENT), dropped.fill_(-7)
        g_count.replay()
        g_write.replay()
        torch.cuda.synchronize()
        assert torch.equal(length, eager.length) and torch.equal(offset, eager.offset), replay
        assert torch.equal(actions, eager.actions) and int(dropped[0]) == 0, replay

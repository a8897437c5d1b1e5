"""Stepping by pushes with the mask kept, on the device (pw_step_push_mask, VecPushWorld.step_push_mask / observe_pushes, the
push-mode facades): in lockstep with pw_step_push + pw_push_mask + pw_walk_regions, against the restatement of
tests/push_env_restatement.py, on views that went stale behind the call's back, under the stuck rule, captured, and through the
facades.  Every comparison covers every environment of its batch."""
import numpy as np
import pytest
import torch

import deep_puzzles
import push_env_restatement as ER
import push_step_restatement as SR
import shape_states as SS
import walk_restatement as WR
from oracle import c_oracle
from pushworld_amd import _capi, _compat
from pushworld_amd.puzzle import PushWorldPuzzle
from pushworld_amd.search import PUSH_NONE, decode_push_choice
from pushworld_amd.vec_env import VecPushWorld
from pushworld_amd.vector_env import PushWorldPushDmVectorEnv, PushWorldPushVectorEnv, _load_pool
from test_gpu_push_step import Rig, _bits, _first_rows, _level1_vec, _serpentine_region
from test_gpu_walk import SEALED, TABLES, WIDE, _corner_texts, _level, _level0
from test_walk_host import HAND

pytestmark = pytest.mark.gpu

STUCK_CORRIDOR = "G0 . A M0 .\n"  # one push to the right puts M0 against the border: no push move is left, and it is not solved
STEP_FIELDS = ("pos", "steps", "reward", "dgoals", "terminated", "truncated")
VIEW_FIELDS = ("push_view_mask", "push_view_count", "push_walk_map", "push_region_size", "_push_view_pos", "_push_view_id")


def _same(a, b):
    """Bit for bit (a float64 tensor by its bits)."""
    if a.dtype == torch.float64:
        a, b = a.view(torch.int64), b.view(torch.int64)
    if a.dtype == torch.uint16:
        a, b = a.view(torch.int16), b.view(torch.int16)
    return a.shape == b.shape and torch.equal(a, b)


# ---- 1. lockstep with the existing entry points -------------------------------------------------------------------------------
def _draw(wide, gen):
    """(push_from, push_action) drawn from the expanded mask ``wide`` [B, 4, H, W]; about one in eight replaced by a cell that
    is no push move, PUSH_NONE or an action of 7."""
    B, _, H, W = wide.shape
    flat = wide.reshape(B, -1).to(torch.float32)
    has = flat.sum(1, keepdim=True) > 0
    choice = torch.multinomial(torch.where(has, flat, torch.ones_like(flat)), 1, generator=gen).squeeze(1)
    other = torch.multinomial(1.0 - flat, 1, generator=gen).squeeze(1)  # (a mask is never all ones: the border cells)
    swap = torch.randint(0, 8, (B,), generator=gen, device=wide.device) == 0
    kind = torch.randint(0, 3, (B,), generator=gen, device=wide.device)
    choice = torch.where(swap & (kind == 0), other, choice)
    choice = torch.where(swap & (kind == 1), torch.full_like(choice, -1), choice)
    frm, act = decode_push_choice(choice, H, W)
    act = torch.where(swap & (kind == 2), torch.full_like(act, 7), act)
    return frm, act.contiguous(), int((swap & (kind == 2)).sum())


def _pair(texts, B, tables, **kw):
    puzzles = [PushWorldPuzzle(text=t) for t in texts]
    ids = [i % len(texts) for i in range(B)]
    return [VecPushWorld(puzzles, B, puzzle_ids=ids, observation=None, engine_options={"step_tables": tables}, **kw)
            for _ in range(2)]


def _assert_lockstep(one, two, out, t):
    """``one`` after step_push_mask (``out``) against ``two`` after step_push, push_mask and walk_regions(maps=True)."""
    mask = two.push_mask()
    reg = two.walk_regions(maps=True)
    for name in STEP_FIELDS:
        assert _same(getattr(one, name), getattr(two, name)), (name, t)
    assert _same(out.moves, two.push_moves_taken) and _same(out.status, two.push_status), t
    assert _same(out.mask, mask) and _same(out.num_pushes, two.num_pushes), t
    assert _same(one.push_walk_map, reg.walk_map) and _same(one.push_region_size, reg.region_size), t
    assert out.reward is one.reward and out.terminated is one.terminated and out.truncated is one.truncated and out.obs is None
    assert one.counters() == two.counters(), t
    return mask


@pytest.mark.parametrize("B", [1, 65, 300])
@pytest.mark.parametrize("tables", TABLES)
@pytest.mark.parametrize("npad", [4, 8, 16, 32])
def test_lockstep_with_step_push_and_push_mask(npad, tables, B):
    texts = [t for t in _corner_texts(npad) if npad > 4 or c_oracle.COraclePuzzle(t).num_movables <= 4]
    one, two = _pair(texts, B, tables, max_steps=12, autoreset=True)
    assert one.num_objects_padded == npad
    one.reset()
    two.reset()
    one.counters_reset()
    two.counters_reset()
    gen = torch.Generator(device=one.device).manual_seed(1000 * npad + B)
    # observe: the views of the first states
    mask, count = one.observe_pushes()
    assert _same(mask, two.push_mask()) and _same(count, two.num_pushes)
    assert _same(one.pos, two.pos) and one.counters() == two.counters()
    seen, sevens = set(), 0
    for t in range(40):
        frm, act, n7 = _draw(two.push_mask(expanded=True), gen)
        sevens += n7
        out = one.step_push_mask(frm, act)
        two.step_push(frm, act)
        _assert_lockstep(one, two, out, t)
        seen |= set(out.status.cpu().tolist())
        # the view is the one of the state that is left
        assert _same(one._push_view_id, one.puzzle_id)
    if B == 300:
        assert seen == {SR.REFUSED, SR.DONE, SR.CUT, SR.RESET} and sevens > 0
        c = one.counters()
        assert c["env_steps"] > B * 10 and c["episodes_ended"] > B


# ---- 2. against the restatement -------------------------------------------------------------------------------------------------
class EnvRig(Rig):
    """``test_gpu_push_step.Rig`` for pw_step_push_mask: ``run`` performs one call over a batch of (puzzle id, state, steps,
    flags, choice) and compares every output and every entry of every view with the restatement.  ``primed``: the views are made
    current first by the observe call (all PUSH_NONE, no flags), so the step is looked up in them; otherwise every view is
    invalid on entry and filled with sentinels."""

    def __init__(self, texts, tables="all", max_steps=None):
        super().__init__(texts, tables, max_steps)
        self.map_h, self.map_w = self.vec.pset.max_height, self.vec.pset.max_width

    def run(self, ids, states, choices, steps=None, term=None, trunc=None, flags=0, pad=0, primed=False):
        n, dev = len(ids), self.dev
        steps = [0] * n if steps is None else list(steps)
        term = [0] * n if term is None else list(term)
        trunc = [0] * n if trunc is None else list(trunc)
        pos_in = np.full((n, self.npad, 2), pad, np.int8)
        for i, s in enumerate(states):
            pos_in[i, :len(s)] = np.asarray(s, np.int8)
        t_ids = torch.as_tensor(np.asarray(ids, np.int32), device=dev)
        t_from = torch.as_tensor(np.asarray([c[0] for c in choices], np.int8).reshape(n, 2), device=dev)
        t_act = torch.as_tensor(np.asarray([c[1] for c in choices], np.uint8), device=dev)
        t_pos = torch.as_tensor(pos_in, device=dev)
        t_steps = torch.as_tensor(np.asarray(steps, np.int32), device=dev)
        t_term = torch.as_tensor(np.asarray(term, np.uint8), device=dev)
        t_trunc = torch.as_tensor(np.asarray(trunc, np.uint8), device=dev)
        t_reward = torch.full((n,), 77.0, dtype=torch.float64, device=dev)
        t_dgoals = torch.full((n,), 77, dtype=torch.int8, device=dev)
        t_moves = torch.full((n,), -7, dtype=torch.int32, device=dev)
        t_status = torch.full((n,), 77, dtype=torch.int8, device=dev)
        v_mask = torch.full((n, self.map_h, self.map_w), 0xAB, dtype=torch.uint8, device=dev)
        v_count = torch.full((n,), -7, dtype=torch.int32, device=dev)
        v_map = torch.full((n, self.map_h, self.map_w), 0x1234, dtype=torch.int16, device=dev).view(torch.uint16)
        v_size = torch.full((n,), -7, dtype=torch.int32, device=dev)
        v_pos = torch.full((n, self.npad, 2), 99, dtype=torch.int8, device=dev)
        v_id = torch.full((n,), -1, dtype=torch.int32, device=dev)
        view = (v_mask, v_count, v_map, v_size, v_pos, v_id)
        eng = self.vec.engine
        if primed:
            none_from = torch.zeros((n, 2), dtype=torch.int8, device=dev)
            none_act = torch.full((n,), PUSH_NONE, dtype=torch.uint8, device=dev)
            eng.step_push_mask(t_ids, none_from, none_act, t_pos, t_steps, None, None, t_term, t_trunc, None, None, *view, 0)
            assert (t_pos.cpu().numpy() == pos_in).all() and t_steps.cpu().tolist() == steps
            assert t_term.cpu().tolist() == term and t_trunc.cpu().tolist() == trunc
        eng.step_push_mask(t_ids, t_from, t_act, t_pos, t_steps, t_reward, t_dgoals, t_term, t_trunc, t_moves, t_status, *view,
                           flags)
        pos, got_steps, reward, dgoals, got_term, got_trunc, moves, status = (
            x.cpu().numpy() for x in (t_pos, t_steps, t_reward, t_dgoals, t_term, t_trunc, t_moves, t_status))
        g_mask, g_count, g_size, g_vpos, g_vid = (x.cpu().numpy() for x in (v_mask, v_count, v_size, v_pos, v_id))
        g_map = v_map.view(torch.int16).cpu().numpy().view(np.uint16)
        out = []
        for i in range(n):
            cp = self.cp(ids[i])
            clamped = self.cps[min(max(ids[i], 0), len(self.cps) - 1) if ids[i] >= 0 else len(self.cps) - 1]
            live = cp is not None and WR.in_grid(cp, states[i])
            st = ER.step(cp, ids[i], SR.Env(states[i], steps[i], term[i], trunc[i]), choices[i][0], choices[i][1],
                         max_steps=self.max_steps, autoreset=bool(flags & _capi.STEP_AUTORESET),
                         end_stuck=bool(flags & _capi.PUSH_END_STUCK), initial=clamped.initial_state,
                         reg=self.region(ids[i], states[i]) if live else None,
                         region_of=lambda s, pid=ids[i]: self.region(pid, s))
            out.append(st)
            want = st.result
            if want.status == SR.REFUSED:
                assert (pos[i] == pos_in[i]).all(), i  # untouched, whatever the row held
            else:
                m = len(want.state)
                rest = 0 if want.status == SR.RESET else pos_in[i, m:]
                assert (pos[i, :m] == np.asarray(want.state, np.int8)).all() and (pos[i, m:] == rest).all(), (i, ids[i], choices[i])
            got = (got_steps[i], int(_bits(reward[i])), dgoals[i], got_term[i], got_trunc[i], moves[i], status[i])
            assert got == (want.steps, int(_bits(want.reward)), want.dgoals, want.terminated, want.truncated, want.moves,
                           want.status), (i, ids[i], choices[i], got, want)
            # the view of the state that is left: every entry
            w_mask, w_map = ER.dense(st.view, self.map_h, self.map_w)
            assert (g_mask[i] == w_mask).all() and (g_map[i] == w_map).all(), (i, ids[i], choices[i])
            assert (g_count[i], g_size[i], g_vid[i]) == (st.view.num_pushes, st.view.region_size, st.view.pid), (i, ids[i])
            k = len(st.view.pos)
            assert (g_vpos[i, :k] == np.asarray(st.view.pos, np.int8).reshape(k, 2)).all() and (g_vpos[i, k:] == 0).all(), i
        return out


@pytest.mark.parametrize("primed", [False, True], ids=["stale", "current"])
@pytest.mark.parametrize("tables", TABLES)
@pytest.mark.parametrize("npad", [4, 8, 16, 32])
def test_every_push_row_once(npad, tables, primed):
    texts = [t for t in _corner_texts(npad) if npad > 4 or c_oracle.COraclePuzzle(t).num_movables <= 4]
    rig = EnvRig(texts, tables)
    assert rig.npad == npad and HAND in texts and WIDE in texts
    ids, states, choices = [], [], []
    for pid, cp in enumerate(rig.cps):
        for pm in rig.region(pid, cp.initial_state).pushes:
            ids.append(pid)
            states.append(cp.initial_state)
            choices.append((pm.frm, pm.action))
    out = rig.run(ids, states, choices, pad=-7, primed=primed)
    assert len(ids) >= len(texts) and sum(st.result.status == SR.DONE for st in out) > len(out) // 2
    assert max(st.result.moves for st in out) > 3 and any(st.result.terminated for st in out)
    assert any(st.view.num_pushes == 0 for st in out) and any(st.view.num_pushes > 2 for st in out)


REFUSALS = [  # (id, state or None for the initial one, choice) on [corridor(8), HAND]
    (0, None, ((10, 1), 1)), (0, None, ((-1, 1), 1)), (0, None, ((5, -128), 1)), (0, None, ((127, 127), 1)),
    (0, None, ((9, 1), 1)), (0, None, ((7, 1), 1)), (0, None, ((3, 1), 1)), (0, None, ((1, 1), 0)), (0, None, ((5, 1), 4)),
    (0, None, ((5, 1), PUSH_NONE)), (-1, None, ((5, 1), 1)), (2, None, ((5, 1), 1)), (1 << 20, None, ((5, 1), 1)),
    (0, ((1, 1), (10, 1)), ((5, 1), 1)), (0, ((1, 1), (6, -1)), ((5, 1), 1)), (1, None, ((6, 2), 1)), (1, None, ((2, 1), 3)),
]


@pytest.mark.parametrize("primed", [False, True], ids=["stale", "current"])
def test_refusals_and_resets(primed):
    rig = EnvRig([deep_puzzles.corridor(8), HAND], max_steps=50)
    items = [(0, None, ((5, 1), 1))] + REFUSALS + [(1, None, ((2, 1), 1)), (0, None, ((5, 1), 1))]
    n = len(items)
    ids = [it[0] for it in items]
    states = [it[1] if it[1] is not None else rig.cps[it[0] if it[0] in (0, 1) else 0].initial_state for it in items]
    choices = [it[2] for it in items]
    out = rig.run(ids, states, choices, steps=[20 + i for i in range(n)], term=[9] * n, trunc=[5] * n, pad=-7, primed=primed)
    assert [st.result.status for st in out] == [SR.DONE] + [SR.REFUSED] * (n - 3) + [SR.DONE, SR.DONE]
    assert [st.view == ER.SKIPPED for st in out] == [10 < i < 16 for i in range(n)]
    # with autoreset: reset where a flag is set, and the view is the initial state's (an id outside the set resets as the
    # clamped id, as pw_step, and its view is the skipped one)
    flags = [0 if i % 2 else 1 for i in range(n)]
    out = rig.run(ids, states, choices, steps=[3] * n, term=flags, trunc=[0] * n, flags=_capi.STEP_AUTORESET, pad=5, primed=primed)
    assert [st.result.status for st in out[:4]] == [SR.RESET, SR.REFUSED, SR.RESET, SR.REFUSED]
    assert out[12].result.status == SR.RESET and out[12].result.state == rig.cps[1].initial_state and out[12].view == ER.SKIPPED
    assert out[2].view == ER.view_of(rig.cps[0], 0, rig.cps[0].initial_state)


@pytest.mark.parametrize("primed", [False, True], ids=["stale", "current"])
@pytest.mark.parametrize("max_steps", [1, 3, 4, 5, 6])
def test_cuts_on_the_corridor(max_steps, primed):
    rig = EnvRig([deep_puzzles.corridor(8)], max_steps=max_steps)
    s0 = rig.cps[0].initial_state
    out = rig.run([0] * 4, [s0] * 4, [((5, 1), 1)] * 4, steps=[0, 1, 2, 9], primed=primed)
    first = out[0].result
    assert first.moves == min(5, max_steps) and first.status == (SR.DONE if max_steps >= 5 else SR.CUT)
    assert out[3].result.moves == 1 and out[3].result.status == SR.CUT and out[3].result.steps == 10
    assert out[3].view.walk_map[(2, 1)] == 0  # the agent stands one cell on


@pytest.mark.parametrize("primed", [False, True], ids=["stale", "current"])
@pytest.mark.parametrize("max_steps", [None, 1, 1000, 1948, 1949])
def test_cuts_on_the_serpentine(max_steps, primed):
    """A parent chain of 1 948 links: with current views the cut follows it through the walk map in memory."""
    cp, reg = _serpentine_region()
    rig = EnvRig([deep_puzzles.serpentine(62, 61)], max_steps=max_steps)
    rig.cps[0] = cp  # (the session's oracle: its step cache is shared with the other serpentine tests)
    rig._regions[(0, cp.initial_state)] = reg
    pm = reg.pushes[0]
    assert pm.walk == 1948 > 64
    out = rig.run([0, 0], [cp.initial_state] * 2, [(pm.frm, pm.action), (pm.frm, pm.action ^ 1)], primed=primed)
    res = out[0].result
    assert res.moves == (1949 if max_steps is None else min(1949, max_steps))
    assert res.status == (SR.DONE if max_steps in (None, 1949) else SR.CUT)
    assert out[1].result.status == SR.REFUSED and out[1].view.region_size == len(reg.dist) > 1900
    if max_steps not in (None, 1949):
        assert reg.dist[res.state[0]] == max_steps and out[0].view.region_size == len(reg.dist)


@pytest.mark.parametrize("primed", [False, True], ids=["stale", "current"])
def test_goal_states_on_entry(primed):
    no_goal = "A . . M0 .\n. . . . .\n"
    rig = EnvRig([HAND, no_goal])
    hand, free = rig.cps
    m0 = hand.py.names.index("m0")
    goal = tuple((2, 2) if k == 0 else ((4, 2) if k == m0 else xy) for k, xy in enumerate(hand.initial_state))
    assert hand.py.is_goal_state(goal) and free.num_goals == 0
    ids, states, choices = [], [], []
    for pid, s in ((0, goal), (1, free.initial_state)):
        for pm in rig.region(pid, s).pushes:
            ids.append(pid)
            states.append(s)
            choices.append((pm.frm, pm.action))
    out = rig.run(ids, states, choices, primed=primed)
    walked = [st.result for st, c, s in zip(out, choices, states) if tuple(c[0]) != tuple(s[0])]
    pushed = [st.result for st, c, s in zip(out, choices, states) if tuple(c[0]) == tuple(s[0])]
    assert walked and all((r.status, r.moves, r.reward, r.terminated) == (SR.CUT, 1, 10.0, 1) for r in walked)
    assert pushed and all(r.status == SR.DONE and r.moves == 1 for r in pushed)


class ShapeEnvRig(EnvRig):
    """``EnvRig`` over a case of shape_states: its oracle puzzle and its regions are the session's."""

    def __init__(self, case, max_steps=None):
        super().__init__([SS.text(case)], "all", max_steps)
        self.case = case
        self.cps = [SS.puzzle(case)]

    def region(self, pid, state):
        return SS.region(self.case, state)


# rows per listed state: all of them on the small boards; on the 64-wide frame the last one (the restatement floods the region of
# every state that is left in plain Python: once per session, shape_states keeps the regions)
SHAPE_ROWS = {SS.CASES[0]: None, SS.CASES[2]: None, SS.CASES[5]: 1}
SHAPE_CUT = {SS.CASES[0]: 5, SS.CASES[2]: 5, SS.CASES[5]: 30}  # test_gpu_push_step_shapes.CUT_MAX_STEPS


@pytest.mark.parametrize("primed", [False, True], ids=["stale", "current"])
@pytest.mark.parametrize("cut", [False, True], ids=["whole", "cut"])
@pytest.mark.parametrize("case", list(SHAPE_ROWS), ids=[str(c) for c in SHAPE_ROWS])
def test_overlapping_states(case, cut, primed):
    cp = SS.puzzle(case)
    rig = ShapeEnvRig(case, max_steps=SHAPE_CUT[case] if cut else None)
    assert rig.npad == SS.PADDING[case] and rig.map_h == SS.FRAME[case]
    ids, states, choices = [], [], []
    for listed in SS.states(case):
        rows = SS.region(case, listed.state).pushes
        if SHAPE_ROWS[case]:
            rows = rows[-SHAPE_ROWS[case]:]
        for pm in rows:
            ids.append(0)
            states.append(listed.state)
            choices.append((pm.frm, pm.action))
    assert len(ids) >= 8 and any(SS.overlapping(cp, s) for s in states)
    out = rig.run(ids, states, choices, steps=[i % 3 for i in range(len(ids))] if cut else None, pad=-7, primed=primed)
    assert all(st.result.status in (SR.DONE, SR.CUT) for st in out)
    if cut:
        assert any(st.result.status == SR.CUT and st.result.moves >= 2 for st in out)
    else:
        assert all(st.result.status == SR.DONE for st in out)
        if case == SS.CASES[0]:  # pushes that carry a movable out of its grid: the view of such a state is the skipped one
            assert sum(st.view == ER.SKIPPED for st in out) == 15


# ---- 3. views that went stale behind the call's back --------------------------------------------------------------------------
def _twin(vec, texts, **kw):
    """A second environment in the state of ``vec`` whose views are all invalid."""
    other = VecPushWorld([PushWorldPuzzle(text=t) for t in texts], vec.num_envs, observation=None, **kw)
    other.reset()
    for name in ("puzzle_id", "pos", "steps", "terminated", "truncated"):
        getattr(other, name).copy_(getattr(vec, name))
    other._push_view()
    assert bool((other._push_view_id == -1).all())
    return other


def _assert_same_call(vec, other, frm, act, **kw):
    a = vec.step_push_mask(frm, act, **kw)
    b = other.step_push_mask(frm, act, **kw)
    for name in STEP_FIELDS + VIEW_FIELDS:
        assert _same(getattr(vec, name), getattr(other, name)), name
    assert _same(a.moves, b.moves) and _same(a.status, b.status)
    return a


STALE_TEXTS = [deep_puzzles.corridor(8), HAND, "A . . M0 . G0 .\n", "A . W M0 . G0 .\n"]


def _stale_vec(B=96, ids=None):
    vec = VecPushWorld([PushWorldPuzzle(text=t) for t in STALE_TEXTS], B, observation=None, max_steps=30,
                       puzzle_ids=[i % 2 for i in range(B)] if ids is None else ids)
    vec.reset()
    return vec


@pytest.mark.parametrize("how", ["invalidated", "step", "set_states"])
def test_stale_views_are_rebuilt(how):
    vec = _stale_vec()
    B, dev = vec.num_envs, vec.device
    vec.observe_pushes()
    first = vec.push_view_mask.clone()
    if how == "invalidated":
        vec._push_view_id.fill_(-1)
    elif how == "step":  # the agents of the even environments (the corridor) walk one cell to the right
        vec.step(torch.as_tensor(np.asarray([1 if e % 2 == 0 else 0 for e in range(B)], np.uint8), device=dev))
    else:
        pos = vec.states()
        pos[::4, 0] = (3, 1)  # the corridor's agents, two cells on
        vec.set_states(pos)
    other = _twin(vec, STALE_TEXTS, max_steps=30)
    frm, act = _first_rows(vec)
    out = _assert_same_call(vec, other, frm, act)
    assert bool((out.status == SR.DONE).all())
    assert _same(out.mask, vec.push_mask()) and not _same(out.mask, first)
    reg = vec.walk_regions(maps=True)
    assert _same(vec.push_walk_map, reg.walk_map) and _same(vec.push_region_size, reg.region_size)


def test_puzzle_id_changed_under_equal_positions():
    """Puzzles 2 and 3 have the same initial positions; in 3 a wall seals the agent off from M0."""
    B = 64
    vec = _stale_vec(B, ids=[2] * B)
    dev = vec.device
    vec.observe_pushes()
    assert bool((vec.push_view_count == 1).all())
    ids = np.asarray([3 if e % 3 == 0 else 2 for e in range(B)], np.int32)
    vec.set_puzzle_ids(ids)
    assert bool((vec._push_view_pos == vec.pos).all())  # the position bytes say "current"
    other = _twin(vec, STALE_TEXTS, max_steps=30)
    frm = torch.as_tensor(np.asarray([[3, 1]] * B, np.int8), device=dev)
    act = torch.ones((B,), dtype=torch.uint8, device=dev)
    out = _assert_same_call(vec, other, frm, act)
    assert out.status.cpu().tolist() == [SR.REFUSED if e % 3 == 0 else SR.DONE for e in range(B)]
    assert out.num_pushes.cpu().tolist() == [0 if e % 3 == 0 else 1 for e in range(B)]
    assert _same(vec._push_view_id, vec.puzzle_id) and _same(out.mask, vec.push_mask())


def test_bytes_beyond_the_movables_do_not_make_a_view_stale():
    """The corridor has 2 movables in rows of 4.  Whether a view was taken as current shows in a view the test has emptied: the
    choice is looked up there and refused; a rebuilt view would allow it."""
    B = 64
    vec = _stale_vec(B, ids=[0] * B)
    vec.observe_pushes()
    assert vec.num_objects_padded == 4
    vec.pos[:, 2:] = -7
    filled = vec.push_view_mask.clone()
    vec.push_view_mask[::2] = 0
    frm, act = _first_rows(vec)
    out = vec.step_push_mask(frm, act)
    assert out.status.cpu().tolist() == [SR.REFUSED if e % 2 == 0 else SR.DONE for e in range(B)]
    assert bool((vec.pos[:, 2:] == -7).all())
    # and one byte inside the movables does
    vec.push_view_mask[::2] = filled[::2]
    vec.push_view_mask[::4] = 0
    vec._push_view_pos[::4, 1, 0] += 1
    out = vec.step_push_mask(frm, act)
    assert out.status.cpu().tolist() == [SR.DONE if e % 2 == 0 else SR.REFUSED for e in range(B)]
    assert _same(out.mask, vec.push_mask())


def test_refusal_with_a_current_view_changes_nothing():
    vec = _stale_vec()
    B, dev = vec.num_envs, vec.device
    vec.observe_pushes()
    before = {name: getattr(vec, name).clone() for name in STEP_FIELDS[:2] + STEP_FIELDS[4:] + VIEW_FIELDS}
    # a walk move of the corridor / a cell outside HAND's region, PUSH_NONE, an action of 7
    frm = torch.as_tensor(np.asarray([[3, 1], [5, 3], [0, 0], [1, 1]] * (B // 4), np.int8), device=dev)
    act = torch.as_tensor(np.asarray([1, 1, PUSH_NONE, 7] * (B // 4), np.uint8), device=dev)
    out = vec.step_push_mask(frm, act, end_stuck=True)
    assert bool((out.status == SR.REFUSED).all()) and bool((out.moves == 0).all()) and bool((out.reward == 0).all())
    for name, was in before.items():
        assert _same(getattr(vec, name), was), name
    assert _same(out.mask, vec.push_mask()) and _same(out.num_pushes, vec.num_pushes)
    assert vec.observe_pushes()[0] is vec.push_view_mask and _same(vec.push_view_mask, before["push_view_mask"])


# ---- 4. the stuck rule ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("primed", [False, True], ids=["stale", "current"])
def test_end_stuck(primed):
    rig = EnvRig([SEALED, STUCK_CORRIDOR, deep_puzzles.corridor(8)], max_steps=50)
    sealed, stuck, cor = rig.cps
    assert stuck.initial_state == ((3, 1), (4, 1)) and len(rig.region(1, stuck.initial_state).pushes) == 1
    left = ((4, 1), (5, 1))  # after the push: nothing more to push
    assert not rig.region(1, left).pushes and not stuck.py.is_goal_state(left)
    items = [  # (id, state, choice, terminated, truncated)
        (0, sealed.initial_state, ((1, 1), 1), 0, 0),         # refused, and stuck
        (0, sealed.initial_state, ((1, 1), PUSH_NONE), 0, 0),
        (0, sealed.initial_state, ((1, 1), 1), 1, 0),         # a flag is set already: left alone
        (0, sealed.initial_state, ((1, 1), 1), 0, 1),
        (1, stuck.initial_state, ((3, 1), 1), 0, 0),          # the last push
        (1, left, ((4, 1), 1), 0, 0),                         # stuck on entry
        (1, stuck.initial_state, ((3, 1), 0), 0, 0),          # a walk move: refused, not stuck
        (2, cor.initial_state, ((5, 1), 1), 0, 0),            # an ordinary push
        (2, ((7, 1), (8, 1)), ((7, 1), 1), 0, 0),             # M0 on its goal and against the border, flags clear: stuck
        (7, cor.initial_state, ((5, 1), 1), 0, 0),            # skipped: no push move either
    ]
    args = ([it[0] for it in items], [it[1] for it in items], [it[2] for it in items])
    kw = dict(steps=[4] * len(items), term=[it[3] for it in items], trunc=[it[4] for it in items], primed=primed)
    for flags in (_capi.PUSH_END_STUCK, _capi.PUSH_END_STUCK | _capi.STEP_AUTORESET, 0, _capi.STEP_AUTORESET):
        rig.vec.counters_reset()
        out = rig.run(*args, flags=flags, **kw)
        counts = ER.Counts()
        for st in out:
            counts.add_step(st)
        c = rig.vec.counters()
        assert (c["env_steps"], c["episodes_ended"], c["episodes_solved"]) == (counts.env_steps, counts.ended, counts.solved)
        auto = bool(flags & _capi.STEP_AUTORESET)
        if flags & _capi.PUSH_END_STUCK:
            # (under autoreset items 2 and 3 are reset -- into the sealed state: stuck at once)
            assert [st.stuck for st in out] == [True, True, auto, auto, True, True, False, False, True, True]
            assert out[4].result.status == SR.DONE and out[4].result.truncated == 1 and out[4].result.moves == 1
            assert counts.ended == sum(st.stuck for st in out)
        else:
            assert not any(st.stuck for st in out) and counts.ended == 0
            assert out[4].result.truncated == 0 and out[5].result.truncated == 0


def test_end_stuck_then_reset_on_the_next_call():
    B = 8
    vec = VecPushWorld([PushWorldPuzzle(text=STUCK_CORRIDOR)], B, observation=None, autoreset=True)
    vec.reset()
    vec.counters_reset()
    frm = torch.as_tensor(np.asarray([[3, 1]] * B, np.int8), device=vec.device)
    act = torch.ones((B,), dtype=torch.uint8, device=vec.device)
    start = vec.pos.clone()
    out = vec.step_push_mask(frm, act, end_stuck=True)
    assert bool((out.status == SR.DONE).all()) and bool((out.truncated == 1).all()) and bool((out.terminated == 0).all())
    assert bool((out.num_pushes == 0).all()) and vec.counters()["episodes_ended"] == B
    out = vec.step_push_mask(frm, act, end_stuck=True)
    assert bool((out.status == SR.RESET).all()) and bool((out.truncated == 0).all()) and _same(vec.pos, start)
    assert bool((out.num_pushes == 1).all()) and vec.counters()["episodes_ended"] == B
    # without the flag the stuck environments stay where they are, call after call
    out = vec.step_push_mask(frm, act)
    out = vec.step_push_mask(frm, act)
    assert bool((out.status == SR.REFUSED).all()) and bool((out.truncated == 0).all()) and bool((out.num_pushes == 0).all())


# ---- 5. capture -----------------------------------------------------------------------------------------------------------------
def test_captured_step_push_mask_equals_eager():
    B = 256
    kw = dict(max_steps=15, autoreset=True)
    cps, eager = _level1_vec(B, **kw)
    _, graphed = _level1_vec(B, **kw)
    eager.reset()
    graphed.reset()
    dev = eager.device
    static_from = torch.zeros((B, 2), dtype=torch.int8, device=dev)
    static_act = torch.zeros((B,), dtype=torch.uint8, device=dev)
    frm, act = _first_rows(eager)
    # warm-up on a side stream (the first call sizes the workspace and allocates the views), then the capture of one call
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        static_from.copy_(frm)
        static_act.copy_(act)
        graphed.step_push_mask(static_from, static_act, end_stuck=True)
    torch.cuda.current_stream(dev).wait_stream(s)
    eager.step_push_mask(frm, act, end_stuck=True)
    assert torch.equal(eager.pos, graphed.pos)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graphed.step_push_mask(static_from, static_act, end_stuck=True)
    # (the captured call ran nothing: both stand where the warm-up left them)
    for r in range(2):
        frm, act = _first_rows(eager)
        static_from.copy_(frm)
        static_act.copy_(act)
        g.replay()
        out = eager.step_push_mask(frm, act, end_stuck=True)
        for name in STEP_FIELDS + VIEW_FIELDS + ("push_moves_taken", "push_status"):
            assert _same(getattr(eager, name), getattr(graphed, name)), (name, r)
        assert int((out.status == _capi.PUSH_DONE).sum()) > B // 2
    assert _same(eager.push_view_mask, eager.push_mask())


# ---- 6. the facades -------------------------------------------------------------------------------------------------------------
def _mix():
    texts = [_level0("level0/walls/train/level_0_walls_train_1732.pwp"), _level(1, "Single Obstacle"), _level(1, "Two Goals"),
             _level(1, "Simple Tool")]
    return [PushWorldPuzzle(text=t) for t in texts]


def _by_hand(puzzles, B, max_steps, seed):
    """The ``VecPushWorld`` a push-mode facade wraps, to be driven through step_push and push_mask with the stuck rule applied
    by the test."""
    _, pad = _load_pool(puzzles, False)
    return VecPushWorld(puzzles, B, max_steps=max_steps, observation="uint8", pad_cells=pad, autoreset=True, resample=True,
                        seed=seed, incremental=True)


def _hand_step(hand, choice):
    obs, reward, term, trunc, moves, status = hand.step_push(choice=choice)
    mask = hand.push_mask()
    stuck = (hand.num_pushes == 0) & (term == 0) & (trunc == 0)
    hand.truncated.copy_(torch.where(stuck, torch.ones_like(trunc), trunc))  # the stuck rule
    return obs, reward, term, hand.truncated, moves, status, mask


def _choose(action_mask, gen):
    flat = action_mask.to(torch.float32)
    has = flat.sum(1, keepdim=True) > 0
    return torch.multinomial(torch.where(has, flat, torch.ones_like(flat)), 1, generator=gen).squeeze(1)


def test_gym_facade_against_the_environment_driven_by_hand():
    B, T, MAX, SEED = 64, 30, 10, 5
    puzzles = _mix()
    env = PushWorldPushVectorEnv(puzzles, B, max_steps=MAX, observation="uint8", seed=SEED)
    hand = _by_hand(puzzles, B, MAX, SEED)
    H, W = hand.pset.max_height, hand.pset.max_width
    assert env.single_action_space.n == 4 * H * W and env.action_space.shape == (B,)
    obs, info = env.reset(seed=SEED)
    assert _same(obs, hand.reset(seed=SEED)) and _same(info["push_mask"], hand.push_mask())
    assert _same(info["action_mask"], hand.push_mask(expanded=True).reshape(B, -1)) and info["action_mask"].dtype == torch.bool
    assert bool((info["moves"] == 0).all()) and bool((info["status"] == 0).all()) and _same(info["puzzle_id"], hand.puzzle_id)
    gen = torch.Generator(device=hand.device).manual_seed(11)
    seen = set()
    for t in range(T):
        choice = _choose(info["action_mask"], gen)
        obs, reward, term, trunc, info = env.step(choice)
        h_obs, h_reward, h_term, h_trunc, h_moves, h_status, h_mask = _hand_step(hand, choice)
        assert _same(obs, h_obs) and _same(reward, h_reward) and _same(term, h_term) and _same(trunc, h_trunc), t
        assert _same(info["push_mask"], h_mask) and _same(info["num_pushes"], hand.num_pushes), t
        assert _same(info["action_mask"], hand.push_mask(expanded=True).reshape(B, -1)), t
        assert _same(info["moves"], h_moves) and _same(info["status"], h_status), t
        assert _same(info["puzzle_id"], hand.puzzle_id) and _same(info["puzzle_state"], hand.pos), t
        assert _same(info["stuck"], (hand.num_pushes == 0) & (h_term == 0)), t
        seen |= set(info["status"].cpu().tolist())
    env.check_actions()  # every choice was a push move (or its environment had none, or was reset)
    assert {SR.DONE, SR.RESET} <= seen and _same(env.render(), hand.obs)
    env.close()


def test_dm_facade_against_the_environment_driven_by_hand():
    B, T, MAX, SEED = 64, 30, 10, 5
    puzzles = _mix()
    env = PushWorldPushDmVectorEnv(puzzles, B, max_steps=MAX, observation="uint8", seed=SEED)
    hand = _by_hand(puzzles, B, MAX, SEED)
    H, W = hand.pset.max_height, hand.pset.max_width
    assert env.action_spec().num_values == 4 * H * W
    spec = env.observation_spec()
    assert tuple(spec["action_mask"].shape) == (4 * H * W,) and tuple(spec["board"].shape) == tuple(hand.obs.shape[1:])
    ts = env.reset(seed=SEED)
    assert _same(ts.observation["board"], hand.reset(seed=SEED))
    assert _same(ts.observation["action_mask"], hand.push_mask(expanded=True).reshape(B, -1))
    assert bool((ts.step_type == int(_compat.StepType.FIRST)).all()) and bool((ts.discount == 1).all())
    gen = torch.Generator(device=hand.device).manual_seed(12)
    was_done = torch.zeros((B,), dtype=torch.bool, device=hand.device)
    kinds = set()
    for t in range(T):
        choice = _choose(ts.observation["action_mask"], gen)
        ts = env.step(choice)
        h_obs, h_reward, h_term, h_trunc, _, h_status, _ = _hand_step(hand, choice)
        done = (h_term != 0) | (h_trunc != 0)
        assert _same(was_done, h_status == SR.RESET), t
        want_type = torch.where(was_done, 0, torch.where(done, 2, 1)).to(torch.int32)
        assert _same(ts.step_type, want_type) and _same(ts.discount, torch.where(done & ~was_done, 0.0, 1.0).to(torch.float64)), t
        assert _same(ts.reward, h_reward) and _same(ts.observation["board"], h_obs), t
        assert _same(ts.observation["action_mask"], hand.push_mask(expanded=True).reshape(B, -1)), t
        was_done = done
        kinds |= set(ts.step_type.cpu().tolist())
    assert kinds == {0, 1, 2}
    env.check_actions()


def test_refused_choices_are_reported():
    puzzles = [PushWorldPuzzle(text=deep_puzzles.corridor(8))]
    env = PushWorldPushVectorEnv(puzzles, 4, observation="uint8")
    _, info = env.reset()
    push = int(info["action_mask"][0].nonzero()[0, 0])
    good = torch.full((4,), push, dtype=torch.int64, device=env.vec.device)
    state = env.vec.pos.clone()
    bad = good.clone()
    bad[2] = 0  # (LEFT from the border cell (0, 0): no push move)
    _, reward, term, trunc, info = env.step(bad)
    assert info["status"].cpu().tolist() == [SR.DONE, SR.DONE, SR.REFUSED, SR.DONE] and float(reward[2]) == 0.0
    assert _same(env.vec.pos[2], state[2]) and not bool(term[2]) and not bool(trunc[2])
    with pytest.raises(ValueError, match="action space"):
        env.check_actions()
    env.check_actions()  # read and cleared
    with pytest.raises(ValueError, match="action space"):
        env.step(np.asarray([0, 1, env.single_action_space.n, 2]))  # a host array is range-checked at once
    host = PushWorldPushVectorEnv(puzzles, 4, observation="uint8", to_numpy=True)
    _, info = host.reset()
    assert isinstance(info["action_mask"], np.ndarray) and info["action_mask"].dtype == np.bool_
    out = host.step(np.full((4,), push, np.int64))
    assert isinstance(out[0], np.ndarray) and out[2].dtype == np.bool_ and out[4]["status"].tolist() == [SR.DONE] * 4
    with pytest.raises(ValueError, match="action space"):
        host.step(np.asarray([push, 0, push, push], np.int64))  # raises at once


def test_stuck_environments_are_reset_on_the_following_step():
    env = PushWorldPushVectorEnv([PushWorldPuzzle(text=STUCK_CORRIDOR)], 4, observation="uint8")
    first, info = env.reset()
    first = first.clone()
    assert not bool(info["stuck"].any()) and bool((info["num_pushes"] == 1).all())
    choice = torch.full((4,), int(info["action_mask"][0].nonzero()[0, 0]), dtype=torch.int64, device=env.vec.device)
    obs, reward, term, trunc, info = env.step(choice)
    assert bool(info["stuck"].all()) and bool((trunc == 1).all()) and bool((term == 0).all()) and not _same(obs, first)
    assert bool((info["status"] == SR.DONE).all()) and not bool(info["action_mask"].any())
    obs, reward, term, trunc, info = env.step(choice)
    assert bool((info["status"] == SR.RESET).all()) and _same(obs, first) and bool((reward == 0).all())
    assert not bool(info["stuck"].any()) and bool((trunc == 0).all())
    env.check_actions()
    # an initial state without a push move: stuck from the start, truncated by the first step, reset and stuck again after it
    sealed = PushWorldPushVectorEnv([PushWorldPuzzle(text=SEALED)], 4, observation="uint8")
    _, info = sealed.reset()
    assert bool(info["stuck"].all()) and bool((info["num_pushes"] == 0).all())
    _, _, _, trunc, info = sealed.step(choice * 0)
    assert bool((trunc == 1).all()) and bool((info["status"] == SR.REFUSED).all())
    _, _, _, trunc, info = sealed.step(choice * 0)
    assert bool((trunc == 1).all()) and bool((info["status"] == SR.RESET).all()) and bool(info["stuck"].all())
    sealed.check_actions()  # there was nothing valid to choose

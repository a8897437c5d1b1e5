"""Stepping by pushes on the device (pw_step_push / pw_push_mask, VecPushWorld.step_push / push_mask, search.push_mask;
DESIGN.md K19) against the restatement of tests/push_step_restatement.py over the C oracle's environment step.  Every output of
every environment is compared field by field -- pos over the puzzle's movables with its zero padding, steps, reward by its bits,
dgoals, both flags, moves and status."""
import numpy as np
import pytest
import torch

import deep_puzzles
import push_step_restatement as SR
import shape_states
import walk_restatement as WR
from oracle import c_oracle
from pushworld_amd import _capi
from pushworld_amd.puzzle import PushWorldPuzzle
from pushworld_amd.search import PUSH_NONE, SolutionTable, push_mask, walk_regions
from pushworld_amd.vec_env import VecPushWorld
from test_gpu_walk import BENCH, TABLES, WIDE, _bench, _bench_states, _corner_texts, _level
from test_walk_host import HAND

pytestmark = pytest.mark.gpu


def _bits(x):
    return np.asarray(x, np.float64).view(np.int64)


class Rig:
    """A puzzle set on the device and its oracles; ``run`` performs one pw_step_push over a batch of (puzzle id, state, steps,
    flags, choice) and compares every output with the restatement."""

    def __init__(self, texts, tables="all", max_steps=None):
        self.texts = list(texts)
        self.cps = [c_oracle.COraclePuzzle(t) for t in self.texts]
        self.max_steps = max_steps
        self.vec = VecPushWorld([PushWorldPuzzle(text=t) for t in self.texts], len(self.texts), observation=None,
                                max_steps=max_steps, engine_options={"step_tables": tables})
        self.dev, self.npad = self.vec.device, self.vec.num_objects_padded
        self._regions = {}

    def cp(self, pid):
        return self.cps[pid] if 0 <= pid < len(self.cps) else None

    def region(self, pid, state):
        key = (pid, tuple(map(tuple, state)))
        if key not in self._regions:
            self._regions[key] = WR.region(self.cps[pid], key[1])
        return self._regions[key]

    def run(self, ids, states, choices, steps=None, term=None, trunc=None, flags=0, pad=0):
        """``pad``: what the input rows hold beyond the states' movables (a sentinel shows who wrote there).  Returns the
        restatement's results."""
        n = len(ids)
        steps = [0] * n if steps is None else list(steps)
        term = [0] * n if term is None else list(term)
        trunc = [0] * n if trunc is None else list(trunc)
        pos_in = np.full((n, self.npad, 2), pad, np.int8)
        for i, s in enumerate(states):
            pos_in[i, :len(s)] = np.asarray(s, np.int8)
        dev = self.dev
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
        self.vec.engine.step_push(t_ids, t_from, t_act, t_pos, t_steps, t_reward, t_dgoals, t_term, t_trunc, t_moves, t_status,
                                  flags)
        pos, got_steps, reward, dgoals, got_term, got_trunc, moves, status = (
            x.cpu().numpy() for x in (t_pos, t_steps, t_reward, t_dgoals, t_term, t_trunc, t_moves, t_status))
        results = []
        for i in range(n):
            cp = self.cp(ids[i])
            clamped = self.cps[min(max(ids[i], 0), len(self.cps) - 1) if ids[i] >= 0 else len(self.cps) - 1]
            live = cp is not None and WR.in_grid(cp, states[i])
            want = SR.macro_step(cp, SR.Env(states[i], steps[i], term[i], trunc[i]), choices[i][0], choices[i][1],
                                 max_steps=self.max_steps, autoreset=bool(flags & _capi.STEP_AUTORESET),
                                 initial=clamped.initial_state, reg=self.region(ids[i], states[i]) if live else None)
            results.append(want)
            if want.status == SR.REFUSED:
                assert (pos[i] == pos_in[i]).all(), i  # untouched, whatever the row held
            else:
                m = len(want.state)
                # the padding: zeroed by a reset (as pw_step), else as it came in (zeros, or the test's sentinel)
                rest = 0 if want.status == SR.RESET else pos_in[i, m:]
                assert (pos[i, :m] == np.asarray(want.state, np.int8)).all() and (pos[i, m:] == rest).all(), (i, ids[i], choices[i])
            got = (got_steps[i], int(_bits(reward[i])), dgoals[i], got_term[i], got_trunc[i], moves[i], status[i])
            assert got == (want.steps, int(_bits(want.reward)), want.dgoals, want.terminated, want.truncated, want.moves,
                           want.status), (i, ids[i], choices[i], got, want)
        return results


# ---- 1. every push row once -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tables", TABLES)
@pytest.mark.parametrize("npad", [4, 8, 16, 32])
def test_every_push_row_once(npad, tables):
    texts = [t for t in _corner_texts(npad) if npad > 4 or c_oracle.COraclePuzzle(t).num_movables <= 4]
    rig = Rig(texts, tables)
    assert rig.npad == npad and HAND in texts and WIDE in texts
    if npad == 32:
        assert rig.cps[-1].num_movables == 17
    ids, states, choices = [], [], []
    for pid, cp in enumerate(rig.cps):
        for pm in rig.region(pid, cp.initial_state).pushes:
            ids.append(pid)
            states.append(cp.initial_state)
            choices.append((pm.frm, pm.action))
    results = rig.run(ids, states, choices)
    # every row is executed: cut only where the initial state is a goal state already (a puzzle without goals) and the row walks
    at_goal = [bool(rig.cps[pid].py.is_goal_state(s)) for pid, s in zip(ids, states)]
    assert len(ids) >= len(texts)
    assert all(r.status == (SR.CUT if g and r.moves == 1 and tuple(c[0]) != tuple(s[0]) else SR.DONE)
               for r, g, c, s in zip(results, at_goal, choices, states))
    assert max(r.moves for r in results) > 3 and any(r.terminated for r in results) and any(r.dgoals for r in results)
    # the successors the rows promise
    at = 0
    for pid, cp in enumerate(rig.cps):
        for pm in rig.region(pid, cp.initial_state).pushes:
            if results[at].status == SR.DONE:
                assert results[at].state == pm.next_state and results[at].moves == pm.walk + 1
            at += 1
    assert sum(r.status == SR.DONE for r in results) > len(results) // 2


# ---- 2. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_among_valid_choices():
    rig = Rig([deep_puzzles.corridor(8), HAND], max_steps=50)
    cor, hand = rig.cps
    s0, h0 = cor.initial_state, hand.initial_state
    push = ((5, 1), 1)
    items = [  # (id, state, choice)
        (0, s0, push),                       # valid
        (0, s0, ((10, 1), 1)),               # a position outside the grid
        (0, s0, ((-1, 1), 1)),
        (0, s0, ((5, -128), 1)),
        (0, s0, ((127, 127), 1)),
        (0, s0, ((9, 1), 1)),                # inside the frame, on the border wall
        (0, s0, ((7, 1), 1)),                # outside the region: behind the box
        (0, s0, ((3, 1), 1)),                # a walk move
        (0, s0, ((1, 1), 0)),                # a move that displaces nothing
        (0, s0, (push[0], 4)),               # actions outside 0..3
        (0, s0, (push[0], PUSH_NONE)),
        (-1, s0, push),                      # puzzle ids outside the set
        (2, s0, push),
        (1 << 20, s0, push),
        (0, ((1, 1), (10, 1)), push),        # a movable outside its grid
        (0, ((1, 1), (6, -1)), push),
        (1, h0, ((6, 2), 1)),                # the 2-cell agent would leave its grid
        (1, h0, ((2, 1), 3)),                # the transitive stop: nothing moves
        (1, h0, ((2, 1), 1)),                # valid
        (0, s0, ((5, 1), 1)),                # valid
    ]
    n = len(items)
    results = rig.run([it[0] for it in items], [it[1] for it in items], [it[2] for it in items], steps=[20 + i for i in range(n)],
                      term=[9] * n, trunc=[5] * n, pad=-7)  # sentinels in the flags, the steps and the rows' padding
    status = [r.status for r in results]
    assert status == [SR.DONE] + [SR.REFUSED] * (n - 3) + [SR.DONE, SR.DONE]
    assert all(r.steps == 20 + i and (r.terminated, r.truncated) == (9, 5) for i, r in enumerate(results) if r.status == SR.REFUSED)
    # with autoreset the same refusals are refused again where the flags are clear, and reset where they are set
    flags = [0 if i % 2 else 1 for i in range(n)]
    results = rig.run([it[0] for it in items], [it[1] for it in items], [it[2] for it in items], steps=[3] * n, term=flags,
                      trunc=[0] * n, flags=_capi.STEP_AUTORESET, pad=5)
    assert [r.status for r in results[:4]] == [SR.RESET, SR.REFUSED, SR.RESET, SR.REFUSED]
    assert results[12].status == SR.RESET and results[12].state == hand.initial_state  # id 2 resets as the clamped id, as pw_step


# ---- 3. cuts ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_steps", [1, 3, 4, 5, 6])
def test_cuts_on_the_corridor(max_steps):
    rig = Rig([deep_puzzles.corridor(8)], max_steps=max_steps)
    s0 = rig.cps[0].initial_state
    entry = [0, 1, 2, 9]  # steps on entry: also at and beyond max_steps (no autoreset: the first step truncates)
    results = rig.run([0] * 4, [s0] * 4, [((5, 1), 1)] * 4, steps=entry)
    first = results[0]
    want_moves = min(5, max_steps)
    assert first.moves == want_moves and first.truncated == int(max_steps <= 5)
    assert first.status == (SR.DONE if max_steps >= 5 else SR.CUT)
    assert first.state == (((6, 1), (7, 1)) if max_steps >= 5 else ((1 + want_moves, 1), (6, 1)))
    assert results[3].moves == 1 and results[3].status == SR.CUT and results[3].steps == 10


_SERP = {}


def _serpentine_region():
    if not _SERP:
        cp = c_oracle.COraclePuzzle(deep_puzzles.serpentine(62, 61))
        _SERP["cp"], _SERP["reg"] = cp, WR.region(cp, cp.initial_state)
    return _SERP["cp"], _SERP["reg"]


@pytest.mark.parametrize("max_steps", [None, 1, 1000, 1948, 1949])
def test_cuts_on_the_serpentine(max_steps):
    cp, reg = _serpentine_region()
    assert len(reg.pushes) == 1 and reg.pushes[0].walk == 1948
    rig = Rig([deep_puzzles.serpentine(62, 61)], max_steps=max_steps)
    rig._regions[(0, cp.initial_state)] = reg
    pm = reg.pushes[0]
    res = rig.run([0, 0], [cp.initial_state] * 2, [(pm.frm, pm.action), (pm.frm, pm.action ^ 1)])[0]
    assert res.moves == (1949 if max_steps is None else min(1949, max_steps))
    assert res.status == (SR.DONE if max_steps in (None, 1949) else SR.CUT)
    if max_steps is None:  # 1 949 sequential additions
        total = 0.0
        for _ in range(1949):
            total += -0.01
        assert int(_bits(res.reward)) == int(_bits(total)) and res.reward != 1949 * -0.01
    else:
        assert res.truncated == 1 and res.state[0] == (pm.next_state[0] if max_steps == 1949 else
                                                       _ancestor(reg, pm.frm, max_steps))


def _ancestor(reg, q, layer):
    q = tuple(q)
    while reg.dist[q] > layer:
        dx, dy = WR.DISPLACEMENTS[reg.parent[q]]
        q = (q[0] - dx, q[1] - dy)
    return q


# ---- 4. autoreset -------------------------------------------------------------------------------------------------------------------
LEVEL1 = ["Single Obstacle", "Two Goals", "2 Obstacle", "Simple Tool"]


def _level1_vec(B, **kw):
    texts = [_level(1, name) for name in LEVEL1]
    cps = [c_oracle.COraclePuzzle(t) for t in texts]
    vec = VecPushWorld([PushWorldPuzzle(text=t) for t in texts], B, puzzle_ids=[i % 4 for i in range(B)], observation=None, **kw)
    return cps, vec


def _live(vec, cps, pos, e):
    cp = cps[e % 4]
    return tuple(tuple(int(v) for v in xy) for xy in pos[e, :cp.num_movables])


def _compare_vec(vec, cps, want, out):
    """The environment's buffers after a macro step against the restatement's results ``want``."""
    obs, reward, term, trunc, moves, status = out
    assert obs is None
    pos, steps = vec.states(), vec.steps.cpu().numpy()
    reward, dgoals, term, trunc, moves, status = (x.cpu().numpy() for x in (reward, vec.dgoals, term, trunc, moves, status))
    for e, w in enumerate(want):
        m = len(w.state)
        assert (pos[e, :m] == np.asarray(w.state, np.int8)).all() and (pos[e, m:] == 0).all(), e
        got = (steps[e], int(_bits(reward[e])), dgoals[e], term[e], trunc[e], moves[e], status[e])
        assert got == (w.steps, int(_bits(w.reward)), w.dgoals, w.terminated, w.truncated, w.moves, w.status), (e, got, w)


def test_autoreset_over_forty_macro_steps():
    B, T, MAX = 64, 40, 12
    cps, vec = _level1_vec(B, max_steps=MAX, autoreset=True)
    vec.reset()
    vec.counters_reset()
    rng = np.random.default_rng(19)
    envs = [SR.Env(cps[e % 4].initial_state, 0, 0, 0) for e in range(B)]
    counts, draws, seen = SR.Counts(), 0, set()
    for t in range(T):
        frm, act, want = np.zeros((B, 2), np.int8), np.zeros(B, np.uint8), []
        for e in range(B):
            cp = cps[e % 4]
            reg = WR.region(cp, envs[e].state)
            rows = reg.pushes
            draws += 1
            if draws % 7 == 0 or not rows:  # a choice that is no push move: PUSH_NONE, a walk move or a cell outside the region
                kind = (draws // 7) % 3
                q = envs[e].state[0]
                choice = ((0, 0), PUSH_NONE) if kind == 0 else ((q, next((a for a in range(4) if not any(
                    pm.frm == q and pm.action == a for pm in rows)), 0)) if kind == 1 else ((cp.width - 1, cp.height - 1), 1))
            else:
                pm = rows[int(rng.integers(0, len(rows)))]
                choice = (pm.frm, pm.action)
            frm[e], act[e] = choice[0], choice[1]
            w = SR.macro_step(cp, envs[e], choice[0], choice[1], max_steps=MAX, autoreset=True, reg=reg)
            want.append(w)
            counts.add(w)
            seen.add(w.status)
            envs[e] = SR.Env(w.state, w.steps, w.terminated, w.truncated)
        out = vec.step_push(torch.as_tensor(frm, device=vec.device), torch.as_tensor(act, device=vec.device))
        _compare_vec(vec, cps, want, out)
    assert seen == {SR.REFUSED, SR.DONE, SR.CUT, SR.RESET}
    c = vec.counters()
    assert (c["env_steps"], c["episodes_ended"], c["episodes_solved"], c["bad_actions"]) == (counts.env_steps, counts.ended,
                                                                                          counts.solved, 0)
    assert counts.env_steps > B * T // 2 and counts.ended > B


def test_choice_and_mask_of_a_vector_environment():
    B = 64
    cps, vec = _level1_vec(B, max_steps=None)
    with pytest.raises(RuntimeError, match="reset"):
        vec.step_push(choice=torch.zeros(B, dtype=torch.int64, device=vec.device))
    vec.reset()
    gen = torch.Generator().manual_seed(3)
    for _ in range(6):
        vec.step(torch.randint(0, 4, (B,), generator=gen, dtype=torch.uint8).to(vec.device))
    pos = vec.states()
    mask = vec.push_mask()
    wide = vec.push_mask(expanded=True)
    H, W = max(cp.height for cp in cps), max(cp.width for cp in cps)
    assert mask.shape == (B, H, W) and mask.dtype == torch.uint8 and wide.shape == (B, 4, H, W) and wide.dtype == torch.bool
    regs = [WR.region(cps[e % 4], _live(vec, cps, pos, e)) for e in range(B)]
    want = np.zeros((B, 4, H, W), bool)
    for e, reg in enumerate(regs):
        for pm in reg.pushes:
            want[e, pm.action, pm.frm[1], pm.frm[0]] = True
    assert (wide.cpu().numpy() == want).all() and vec.num_pushes.cpu().tolist() == [len(r.pushes) for r in regs]
    # the last push move of every environment in the flat order of the expanded mask; an index outside the shape for some
    flat = want.reshape(B, -1)
    choice = np.asarray([np.flatnonzero(f)[-1] if f.any() else 0 for f in flat], np.int64)
    choice[5], choice[6] = -1, 4 * H * W
    steps0 = vec.steps.cpu().numpy()
    out = vec.step_push(choice=torch.as_tensor(choice, device=vec.device))
    results = []
    for e in range(B):
        c = int(choice[e])
        inside = 0 <= c < 4 * H * W
        frm, a = ((c % (H * W)) % W, (c % (H * W)) // W), c // (H * W)
        results.append(SR.macro_step(cps[e % 4], SR.Env(_live(vec, cps, pos, e), int(steps0[e]), 0, 0), frm if inside else (0, 0),
                                     a if inside else PUSH_NONE, reg=regs[e]))
    _compare_vec(vec, cps, results, out)
    assert results[5].status == results[6].status == SR.REFUSED and sum(r.status == SR.DONE for r in results) > B // 2


# ---- 5. overlapping states ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", shape_states.SMALL, ids=[str(c) for c in shape_states.SMALL])
def test_overlapping_states(case):
    cp = shape_states.puzzle(case)
    rig = Rig([shape_states.text(case)])
    rig.cps[0] = cp  # (the session's oracle: its step cache is shared with the other shape tests)
    assert rig.npad == shape_states.PADDING[case]
    ids, states, choices = [], [], []
    for listed in shape_states.states(case):
        reg = shape_states.region(case, listed.state)
        rig._regions[(0, tuple(map(tuple, listed.state)))] = reg
        for pm in reg.pushes:
            ids.append(0)
            states.append(listed.state)
            choices.append((pm.frm, pm.action))
    assert len(ids) > 50 and any(shape_states.overlapping(cp, s) for s in states)
    results = rig.run(ids, states, choices)
    assert all(r.status in (SR.DONE, SR.CUT) for r in results) and sum(r.status == SR.DONE for r in results) > 50


# ---- 6. states that are goal states already ----------------------------------------------------------------------------------------
def test_goal_states_on_entry():
    no_goal = "A . . M0 .\n. . . . .\n"
    rig = Rig([HAND, no_goal])
    hand, free = rig.cps
    assert free.num_goals == 0
    m0 = hand.py.names.index("m0")
    goal = tuple((2, 2) if k == 0 else ((4, 2) if k == m0 else xy) for k, xy in enumerate(hand.initial_state))
    assert hand.py.is_goal_state(goal)
    ids, states, choices = [], [], []
    for pid, s in ((0, goal), (1, free.initial_state)):
        for pm in rig.region(pid, s).pushes:
            ids.append(pid)
            states.append(s)
            choices.append((pm.frm, pm.action))
    results = rig.run(ids, states, choices)
    walked = [r for r, c, s in zip(results, choices, states) if tuple(c[0]) != tuple(s[0])]
    pushed = [r for r, c, s in zip(results, choices, states) if tuple(c[0]) == tuple(s[0])]
    assert walked and all((r.status, r.moves, r.reward, r.terminated) == (SR.CUT, 1, 10.0, 1) for r in walked)
    assert all(r.status == SR.DONE and r.moves == 1 for r in pushed)
    assert {ids[k] for k, c in enumerate(choices) if tuple(c[0]) != tuple(states[k][0])} == {0, 1}
    assert any(r.terminated == 0 and r.dgoals == -1 for r in pushed)  # M0 pushed off its goal: the episode goes on


# ---- 7. the push mask ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tables", TABLES)
def test_push_mask_of_a_mixed_batch(tables):
    b = _bench(tables)
    ids, states = _bench_states(b)
    n0 = len(ids)
    mask = [1] * n0
    for k in (3, n0 // 2):  # masked items
        mask[k] = 0
    for bad_id in (-1, len(BENCH), 1 << 20):  # ids outside the set
        ids.append(bad_id)
        states.append(states[0])
        mask.append(1)
    out = list(b.cps[0].initial_state)  # a movable outside its grid
    out[-1] = (b.cps[0].width, out[-1][1])
    ids.append(0)
    states.append(tuple(out))
    mask.append(1)
    n = len(ids)
    t_ids = torch.as_tensor(np.asarray(ids, np.int32), device=b.dev)
    t_pos = b.pos(states)
    t_mask = torch.as_tensor(np.asarray(mask, np.uint8), device=b.dev)
    reg = walk_regions(b.vec, t_ids, t_pos, t_mask)
    rows = reg.pushes()
    assert rows.num_rows > 100
    # the scatter of the rows
    cells = b.map_h * b.map_w
    flat = (rows.item.long() * b.map_h + rows.frm[:, 1].long()) * b.map_w + rows.frm[:, 0].long()
    want = torch.zeros(n * cells, dtype=torch.int32, device=b.dev)
    want.index_add_(0, flat, torch.bitwise_left_shift(torch.ones_like(flat, dtype=torch.int32), rows.action.to(torch.int32)))
    want = want.to(torch.uint8).view(n, b.map_h, b.map_w)
    got = torch.full((n, b.map_h, b.map_w), 0xAB, dtype=torch.uint8, device=b.dev)  # the fill is overwritten everywhere
    count = torch.full((n,), -7, dtype=torch.int32, device=b.dev)
    b.vec.engine.push_mask(t_ids, t_pos, t_mask, got, count)
    assert torch.equal(got, want)
    assert torch.equal(count.long(), reg.offset[1:] - reg.offset[:-1])
    skipped = [3, n0 // 2] + list(range(n0, n))
    assert bool((got[skipped] == 0).all()) and bool((count[skipped] == 0).all()) and int(count.sum()) == rows.num_rows
    # the wrapper; NULL pos is the initial states; num_pushes may be NULL
    got2, count2 = push_mask(b.vec, t_ids, t_pos, t_mask)
    assert torch.equal(got2, want) and torch.equal(count2, count)
    first = torch.arange(len(BENCH), dtype=torch.int32, device=b.dev)
    init, _ = push_mask(b.vec, first)
    again = torch.full_like(init, 0xAB)
    b.vec.engine.push_mask(first, b.pos([cp.initial_state for cp in b.cps]), None, again, None)
    assert torch.equal(init, again) and int(init.count_nonzero()) > 0


# ---- 8. the expert in pushes --------------------------------------------------------------------------------------------------------
def test_expert_in_pushes():
    pz = PushWorldPuzzle(text=deep_puzzles.big())
    with_table = SolutionTable(pz, max_states=1 << 16)
    states = np.ascontiguousarray(with_table.states().astype(np.int8))[::97]
    with_table.close()
    B = states.shape[0]
    assert B == 442
    vec = VecPushWorld([pz], B, observation=None, max_steps=None)
    vec.reset()
    vec.pos[:, :3].copy_(torch.as_tensor(states, device=vec.device))
    with vec.push_table(0) as tab:
        cost = vec.push_cost_to_go([tab]).cost.clone()
        start = vec.pos.clone()
        live = cost > 0
        assert int(live.sum()) > 100 and int((cost == -1).sum()) > 50 and int((cost == 0).sum()) > 0
        done_at = torch.full((B,), -1, dtype=torch.int32, device=vec.device)
        for t in range(1, int(cost.max()) + 1):
            q = vec.push_cost_to_go([tab])
            _, _, term, _, moves, status = vec.step_push(q.push_from, q.push_action)
            acting = live & (done_at < 0)
            assert bool((status[acting] == _capi.PUSH_DONE).all()) and bool((moves[acting] >= 1).all())
            assert bool((status[~acting] == _capi.PUSH_REFUSED).all()) and bool((moves[~acting] == 0).all())
            assert bool((term[acting] == (cost[acting] == t).to(torch.uint8)).all())  # terminated after exactly `cost` macro steps
            done_at = torch.where(acting & (term != 0), torch.full_like(done_at, t), done_at)
        assert bool((done_at[live] == cost[live]).all()) and bool((done_at[~live] == -1).all())
        assert bool((vec.pos[~live] == start[~live]).all()) and bool((vec.steps[~live] == 0).all())  # dead and goal ones never move
        q = vec.push_cost_to_go([tab])
        assert bool((q.push_action == PUSH_NONE).all())
        assert bool((vec.step_push(q.push_from, q.push_action)[5] == _capi.PUSH_REFUSED).all())


# ---- 9. capture ---------------------------------------------------------------------------------------------------------------------
def _first_rows(vec):
    """(push_from, push_action) of every environment's first push row, PUSH_NONE where it has none: device ops only."""
    reg = vec.walk_regions()
    rows = reg.pushes()
    has = reg.offset[1:] > reg.offset[:-1]
    at = reg.offset[:-1].clamp(max=max(rows.num_rows - 1, 0))
    frm = torch.where(has[:, None], rows.frm[at], torch.zeros_like(rows.frm[at]))
    act = torch.where(has, rows.action[at], torch.full_like(rows.action[at], PUSH_NONE))
    return frm.contiguous(), act.contiguous()


def test_captured_step_push_equals_eager():
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
    # warm-up on a side stream (the first call sizes the workspace), then the capture of one macro step
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        static_from.copy_(frm)
        static_act.copy_(act)
        graphed.step_push(static_from, static_act)
    torch.cuda.current_stream(dev).wait_stream(s)
    eager.step_push(frm, act)
    assert torch.equal(eager.pos, graphed.pos)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graphed.step_push(static_from, static_act)
    # (the captured call ran nothing: both stand where the warm-up left them)
    for r in range(2):
        frm, act = _first_rows(eager)
        static_from.copy_(frm)
        static_act.copy_(act)
        g.replay()
        out = eager.step_push(frm, act)
        assert torch.equal(eager.pos, graphed.pos) and torch.equal(eager.steps, graphed.steps), r
        assert torch.equal(eager.reward, graphed.reward) and torch.equal(eager.dgoals, graphed.dgoals), r
        assert torch.equal(eager.terminated, graphed.terminated) and torch.equal(eager.truncated, graphed.truncated), r
        assert torch.equal(out[4], graphed.push_moves_taken) and torch.equal(out[5], graphed.push_status), r
        assert int((out[5] == _capi.PUSH_DONE).sum()) > B // 2

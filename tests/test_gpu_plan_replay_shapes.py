"""Plan replay on the device (pw_plan_replay_check / pw_plan_replay_emit) on the puzzle sets, starts and plans of
tests/replay_cases.py: random shapes, overlapping starts, traces that leave the grid and return, every padding (N_pad 4 .. 32:
8-, 16- and 32-lane groups), every table form (kTab 0 / 1 / 2), plan lengths around the lane-group width and the plan_cap (37, no
multiple of any group width; rows filled with 0xEE beyond their length), one- and three-goal puzzles.  Verdicts, first goals,
final states, offsets and every field of every row are compared with the C oracle stepped along the same plans
(``COraclePuzzle.env_step``), rewards as float64 bits; tests/test_replay_shapes_host.py pins what the lists hold."""
import numpy as np
import pytest
import torch

import cells_restatement as CR
import replay_cases as RC
import shape_states as SS
from pushworld_amd.puzzle import PushWorldPuzzle
from pushworld_amd.search import REPLAY_EARLY, REPLAY_NONE, REPLAY_NOT_GOAL, REPLAY_VALID, replay_plans
from pushworld_amd.vec_env import VecPushWorld

pytestmark = pytest.mark.gpu

OPTIONS = [{}, {"step_tables": "none"}, {"step_tables": "big"}]
_VECS = {}
_TABLE_COUNTS = {}  # (npad, form) -> (puzzles with tables, puzzles of the set)


def _vec(npad, options, **kw):
    key = (npad, tuple(sorted(options.items())), tuple(sorted(kw.items())))
    if key not in _VECS:
        puzzles = [PushWorldPuzzle(text=RC.text(k)) for k in RC.SETS[npad]]
        _VECS[key] = VecPushWorld(puzzles, len(puzzles), max_steps=None, device=0, engine_options=options,
                                  **({"observation": None} if not kw else kw))
        assert _VECS[key].num_objects_padded == npad
    return _VECS[key]


def _verdict(goals):
    """puzzle.py:413-424 on the goal flags of the states a plan passes through."""
    if any(goals[:-1]):
        return REPLAY_EARLY  # is_valid_plan: False, "goal was achieved before the plan ended"
    return REPLAY_VALID if goals[-1] else REPLAY_NOT_GOAL


def _replay_and_check(vec, npad, items, include="replayed"):
    """One replay_plans call over `items` (plans allocated at exactly n x CAP bytes), everything compared with the oracle."""
    dev, n = vec.device, len(items)
    ids, pos, plans, lens = RC.packed(npad, items)
    assert plans.shape == (n, RC.CAP) and plans.nbytes == n * RC.CAP
    out = replay_plans(vec, torch.as_tensor(ids, device=dev), torch.as_tensor(plans, device=dev),
                       torch.as_tensor(lens, device=dev), pos=torch.as_tensor(pos, device=dev), include=include, next_pos=True)
    traces = [RC.item_trace(it) for it in items]
    want_verdict = np.array([_verdict(tr.goals) for tr in traces], np.int8)
    want_first = np.array([tr.goals.index(True) if True in tr.goals else -1 for tr in traces], np.int32)
    verdict, first, final, offset = (x.cpu().numpy() for x in (out.verdict, out.first_goal, out.final_pos, out.offset))
    bad = np.nonzero(verdict != want_verdict)[0]
    assert bad.size == 0, (bad[:8].tolist(), verdict[bad[:8]].tolist(), want_verdict[bad[:8]].tolist())
    assert (first == want_first).all()
    keep = (REPLAY_VALID,) if include == "valid" else (REPLAY_VALID, REPLAY_NOT_GOAL, REPLAY_EARLY)
    rows = np.where(np.isin(want_verdict, keep), lens.astype(np.int64), 0)
    want_off = np.concatenate([[0], np.cumsum(rows)])
    assert (offset == want_off).all() and out.num_rows == want_off[-1]
    item, t, rpid, rpos, act, rew, done, nxt = (x.cpu().numpy() for x in (out.item, out.t, out.puzzle_id, out.pos, out.action,
                                                                        out.reward, out.done, out.next_pos))
    assert (item == np.repeat(np.arange(n), rows)).all()  # exactly the expected row set, in order
    for i, (it, tr) in enumerate(zip(items, traces)):
        wp = np.stack([RC.padded(s, npad) for s in tr.states])
        assert (final[i] == wp[-1]).all(), (i, it)
        lo, hi = want_off[i], want_off[i + 1]
        if hi == lo:
            continue
        assert (t[lo:hi] == np.arange(hi - lo)).all() and (rpid[lo:hi] == it.pid).all()
        assert (act[lo:hi] == np.array(it.plan, np.uint8)).all(), (i, it)
        assert (rpos[lo:hi] == wp[:-1]).all() and (nxt[lo:hi] == wp[1:]).all(), (i, it)
        assert (rew[lo:hi].view(np.uint64) == np.array(tr.rewards, np.float64).view(np.uint64)).all(), (i, it, rew[lo:hi].tolist())
        assert (done[lo:hi] == np.array(tr.terms, np.uint8)).all(), (i, it)
    return out, want_verdict


@pytest.mark.parametrize("options", OPTIONS, ids=["auto", "none", "big"])
@pytest.mark.parametrize("npad", [4, 8, 16, 32])
def test_sets_against_the_oracle(npad, options):
    vec = _vec(npad, options)
    form = options.get("step_tables", "auto")
    _TABLE_COUNTS[(npad, form)] = (vec.engine.get_option("step_table_puzzles"), len(RC.SETS[npad]))
    items = RC.items(npad)
    _, want = _replay_and_check(vec, npad, items)
    if form == "auto":  # include="valid" gives exactly the VALID items' rows
        out, _ = _replay_and_check(vec, npad, items, include="valid")
        assert out.num_rows == sum(len(it.plan) for it, v in zip(items, want) if v == REPLAY_VALID) > 0


def test_every_table_form_ran():
    """How replay_launch picks kTab: no puzzle with tables (0), some (1), all (2) -- each occurs over the parametrisation."""
    if len(_TABLE_COUNTS) < 12:  # (run alone: build the engines the parametrisation would have built)
        for npad in (4, 8, 16, 32):
            for options in OPTIONS:
                vec = _vec(npad, options)
                _TABLE_COUNTS[(npad, options.get("step_tables", "auto"))] = (vec.engine.get_option("step_table_puzzles"),
                                                                          len(RC.SETS[npad]))
    counts = list(_TABLE_COUNTS.values())
    assert any(c == 0 for c, _ in counts) and any(c == total for c, total in counts) and any(0 < c < total for c, total in counts)
    assert all(c == 0 for (_, form), (c, _) in _TABLE_COUNTS.items() if form == "none")


@pytest.mark.parametrize("n", [1, 3, 64 // 8 + 1])
def test_small_launches(n):
    """Fewer items than the lane groups of one wavefront, and one more: the tail of the item list, whose last item ends with
    the last byte of the plan buffer."""
    vec = _vec(8, {})
    items = RC.items(8)
    full = next(i for i, it in enumerate(items) if len(it.plan) == RC.CAP and i + 1 >= n)  # len == plan_cap, at the buffer's end
    for tail in (items[-n:], items[full + 1 - n:full + 1]):
        assert len(tail) == n
        _replay_and_check(vec, 8, tail)


@pytest.mark.parametrize("npad", [4, 8, 16, 32])
def test_demonstrations_in_cells_mode(npad):
    """VecPushWorld.demonstrations from overlapping live states: the observation of a row is the restatement's of its pos."""
    keys = RC.SETS[npad]
    live = []
    for pid, key in enumerate(keys):
        cp = RC.puzzle(key)
        # (one push from the goal, so that the planner does solve some; then goal-near states, which it may not)
        picked = [s for s, _ in RC.finish_starts(key)] + [s for kind, s in RC.states(key) if kind == "goal_near"]
        live += [(pid, s) for s in picked if SS.overlapping(cp, s)][:2 if key == SS.CASES[5] else 6]
    assert len(live) >= 4
    puzzles = [PushWorldPuzzle(text=RC.text(k)) for k in keys]
    vec = VecPushWorld(puzzles, len(live), puzzle_ids=[p for p, _ in live], observation="cells", max_steps=None, device=0)
    vec.reset()
    vec.set_states(np.stack([RC.padded(s, npad) for _, s in live]))
    sp = vec.planner(heuristic="N+RGD", batch=8, max_states=1 << 14)
    try:
        demo = vec.demonstrations(sp, max_rounds=60, plan_cap=512)
        torch.cuda.synchronize()
    finally:
        sp.close()
    T = demo.num_rows
    verdict, offset = demo.verdict.cpu().numpy(), demo.offset.cpu().numpy()
    assert T > 0 and (verdict == REPLAY_VALID).any()
    rpos, rpid, item = (x.cpu().numpy() for x in (demo.pos, demo.puzzle_id, demo.item))
    first = [int(offset[i]) for i in range(len(live)) if offset[i + 1] > offset[i]]
    last = [int(offset[i + 1]) - 1 for i in range(len(live)) if offset[i + 1] > offset[i]]
    for r in first:  # a plan's first row is the live state
        assert (rpos[r] == RC.padded(live[item[r]][1], npad)).all() and rpid[r] == live[item[r]][0]
    sel = sorted(set(first + last + np.random.default_rng(2).choice(T, size=min(64, T), replace=False).tolist()))
    obs = demo.obs[torch.as_tensor(sel, device=vec.device)].cpu().numpy()
    frame = tuple(vec.engine.cells_shape()[1:])
    for k, r in enumerate(sel):
        cp = RC.puzzle(keys[rpid[r]])
        state = tuple((int(x), int(y)) for x, y in rpos[r][:cp.num_movables])
        assert (obs[k] == CR.cells(cp, state, frame)).all(), r


@pytest.mark.parametrize("options", OPTIONS, ids=["auto", "none", "big"])
@pytest.mark.parametrize("npad", [8, 32])
def test_pw_step_from_states_beyond_the_grid(npad, options):
    """``group_push_set`` equals ``pw_step``: the states of the items' traces that lie beyond the grid (inside the engine's
    domain), each with the action the trace plays there, through ``pw_step`` itself under the same table forms."""
    import walk_restatement as WR

    ids, states, actions, want = [], [], [], []
    for it in RC.items(npad):
        cp, tr = RC.puzzle(it.key), RC.item_trace(it)
        for t, a in enumerate(it.plan):
            if not WR.in_grid(cp, tr.states[t]):
                ids.append(it.pid)
                states.append(tr.states[t])
                actions.append(a)
                want.append((tr.states[t + 1], tr.rewards[t], tr.terms[t]))
    B = len(ids)
    assert B >= 50 and len(set(ids)) >= 2
    puzzles = [PushWorldPuzzle(text=RC.text(k)) for k in RC.SETS[npad]]
    vec = VecPushWorld(puzzles, B, puzzle_ids=ids, observation=None, max_steps=None, device=0, engine_options=options)
    vec.reset()
    vec.set_states(np.stack([RC.padded(s, npad) for s in states]))
    vec.step(torch.as_tensor(np.array(actions, np.uint8), device=vec.device))
    torch.cuda.synchronize()
    pos, reward, term = vec.pos.cpu().numpy(), vec.reward.cpu().numpy(), vec.terminated.cpu().numpy()
    for i, (nxt, r, done) in enumerate(want):
        assert (pos[i] == RC.padded(nxt, npad)).all(), (i, ids[i], states[i], actions[i])
        assert reward[i:i + 1].view(np.uint64)[0] == np.array([r]).view(np.uint64)[0] and term[i] == done, (i, r, reward[i])

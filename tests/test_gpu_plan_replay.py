"""Plan replay on the device (pw_plan_replay_check / pw_plan_replay_emit, search.replay_plans, PlanBatch.validate /
StatePlanner.validate, VecPushWorld.demonstrations) against the C oracle stepped along the same plans: verdicts are the
reference's is_valid_plan, rows are pw_step's (float64 reward bits included), offsets are the prefix sums of the plan lengths,
observations are those of the rows' states.  No time limits anywhere: every case is deterministic."""
import glob
import os

import numpy as np
import pytest
import torch

from oracle import c_oracle, pw_oracle
from pushworld_amd import _capi
from pushworld_amd.puzzle import PushWorldPuzzle
from pushworld_amd.search import (REPLAY_CUT, REPLAY_EARLY, REPLAY_NONE, REPLAY_NOT_GOAL, REPLAY_SKIPPED, REPLAY_VALID,
                                  PlanBatch, replay_plans)
from pushworld_amd.vec_env import VecPushWorld

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "pushworld_amd", "data")
REF_CPP = sorted(glob.glob(os.path.join(ROOT, "tests", "puzzles", "ref_cpp", "*.pwp")))
LEVEL = {k: sorted(glob.glob(os.path.join(DATA, "puzzles", f"level{k}", "*.pwp"))) for k in (1, 2, 3, 4)}
CLEAN_SWEEP = os.path.join(DATA, "puzzles", "level2", "Clean Sweep.pwp")  # 19 movables: NP = 32
HUMAN_TOTAL = 18143  # SURVEY: actions of the 223 human solutions


def _human():
    """(puzzle path, plan as a list of actions) of all Level 1-4 puzzles."""
    out = []
    for k in (1, 2, 3, 4):
        for p in LEVEL[k]:
            name = os.path.splitext(os.path.basename(p))[0]
            with open(os.path.join(DATA, "solutions", f"level{k}", name + ".yaml")) as f:
                plan = [ln.split(":", 1)[1].strip() for ln in f if ln.startswith("plan:")][0]
            out.append((p, ["LRUD".index(c) for c in plan]))
    return out


def _oracles(paths, order):
    return [c_oracle.COraclePuzzle(open(p).read(), order=order) for p in paths]


def _trace(cp, start, plan):
    """The oracle stepped along `plan`: states [len + 1], rewards, terminated flags, goal flag of every state."""
    states, rewards, terms = [tuple(map(tuple, start))], [], []
    for a in plan:
        nxt, r, term = cp.env_step(states[-1], a)
        states.append(nxt)
        rewards.append(r)
        terms.append(term)
    return states, rewards, terms, [cp.py.is_goal_state(s) for s in states]


def _verdict(goals):
    """puzzle.py:413-424 on the goal flags of the states a plan passes through."""
    if any(goals[:-1]):
        return REPLAY_EARLY  # is_valid_plan: False, "goal was achieved before the plan ended"
    return REPLAY_VALID if goals[-1] else REPLAY_NOT_GOAL


def _pack(plans, cap, device):
    arr = np.zeros((len(plans), cap), np.uint8)
    for i, p in enumerate(plans):
        arr[i, :min(len(p), cap)] = p[:cap]
    return torch.as_tensor(arr, device=device)


def _engine(paths, order):
    puzzles = [PushWorldPuzzle(p, order=order) for p in paths]
    vec = VecPushWorld(puzzles, len(paths), observation=None, max_steps=None)
    return vec


def _padded(state, npad):
    row = np.zeros((npad, 2), np.int8)
    row[:len(state)] = np.asarray(state, np.int8)
    return row


@pytest.mark.parametrize("order", ["python", "cpp"])
def test_human_solutions(order):
    human = _human()
    assert len(human) == 223
    paths, plans = [p for p, _ in human], [pl for _, pl in human]
    lens = np.array([len(p) for p in plans], np.int64)
    assert lens.sum() == HUMAN_TOTAL and lens.min() == 6 and lens.max() == 421
    vec = _engine(paths, order)
    dev, npad = vec.device, vec.num_objects_padded
    ids = torch.arange(len(paths), dtype=torch.int32, device=dev)
    out = replay_plans(vec, ids, _pack(plans, 512, dev), torch.as_tensor(lens.astype(np.int32), device=dev), next_pos=True)
    assert (out.verdict.cpu().numpy() == REPLAY_VALID).all()
    assert (out.first_goal.cpu().numpy() == lens).all()
    want_off = np.concatenate([[0], np.cumsum(lens)])
    assert (out.offset.cpu().numpy() == want_off).all() and out.num_rows == HUMAN_TOTAL
    item, t, rpid, pos, act, rew, done, nxt = (x.cpu().numpy() for x in (out.item, out.t, out.puzzle_id, out.pos, out.action,
                                                                        out.reward, out.done, out.next_pos))
    final = out.final_pos.cpu().numpy()
    for i, cp in enumerate(_oracles(paths, order)):
        states, rewards, terms, goals = _trace(cp, cp.initial_state, plans[i])
        lo, hi = want_off[i], want_off[i + 1]
        assert (item[lo:hi] == i).all() and (rpid[lo:hi] == i).all() and (t[lo:hi] == np.arange(hi - lo)).all()
        assert (act[lo:hi] == np.array(plans[i], np.uint8)).all()
        want_pos = np.stack([_padded(s, npad) for s in states])
        assert (pos[lo:hi] == want_pos[:-1]).all(), (i, paths[i])
        assert (nxt[lo:hi] == want_pos[1:]).all(), (i, paths[i])
        assert (final[i] == want_pos[-1]).all()
        assert (rew[lo:hi].view(np.uint64) == np.array(rewards, np.float64).view(np.uint64)).all(), (i, paths[i])
        assert (done[lo:hi] == np.array(terms, np.uint8)).all()
        assert rew[hi - 1] == 10.0 and done[hi - 1] == 1 and not done[lo:hi - 1].any()
        assert _verdict(goals) == REPLAY_VALID


def test_every_verdict_class():
    human = _human()[:40]
    paths = [p for p, _ in human]
    vec = _engine(paths, "python")
    dev, npad = vec.device, vec.num_objects_padded
    cps = _oracles(paths, "python")
    cap = 512
    # (kind, puzzle) items: the classes interleaved with valid neighbours
    kinds = ["valid", "early", "valid", "short", "none", "valid", "cut", "bad_id", "valid", "outside", "bad_byte", "masked",
             "valid", "empty", "big_id"]
    items = [(kinds[i % len(kinds)], i % len(paths)) for i in range(90)]
    plans, lens, pid, mask, pos, want, want_first = [], [], [], [], [], [], []
    py_oracles = {}
    for kind, k in items:
        plan = list(human[k][1])
        start = _padded(cps[k].initial_state, npad)
        m, p_id, ln = 1, k, None
        if kind == "early":
            plan = plan + [0]
        elif kind == "short":
            plan = plan[:-1]
        elif kind == "none":
            ln = -1
        elif kind == "cut":
            ln = cap + 1
        elif kind == "bad_id":
            p_id = -1
        elif kind == "big_id":
            p_id = len(paths)
        elif kind == "outside":
            start = start.copy()
            start[0] = (cps[k].width, 1)
        elif kind == "bad_byte":
            plan[len(plan) // 2] = 7
        elif kind == "masked":
            m = 0
        elif kind == "empty":
            plan = []
        plans.append(plan)
        lens.append(len(plan) if ln is None else ln)
        pid.append(p_id)
        mask.append(m)
        pos.append(start)
        if kind in ("valid", "early", "short", "empty"):  # where the oracle's is_valid_plan is defined
            goals = _trace(cps[k], cps[k].initial_state, plan)[3]
            want.append(_verdict(goals))
            if k < 6:  # the Python oracle's own is_valid_plan (its tables are slow to build: a few puzzles)
                if k not in py_oracles:
                    py_oracles[k] = pw_oracle.load(paths[k])
                assert py_oracles[k].is_valid_plan(plan) == (want[-1] == REPLAY_VALID)
            want_first.append(goals.index(True) if True in goals else -1)
        else:
            want.append({"none": REPLAY_NONE, "cut": REPLAY_CUT}.get(kind, REPLAY_SKIPPED))
            want_first.append(-1)
    want = np.array(want, np.int8)
    by_kind = {k: {int(want[i]) for i, (kk, _) in enumerate(items) if kk == k} for k in kinds}
    assert by_kind == {"valid": {REPLAY_VALID}, "early": {REPLAY_EARLY}, "short": {REPLAY_NOT_GOAL}, "none": {REPLAY_NONE},
                       "cut": {REPLAY_CUT}, "bad_id": {REPLAY_SKIPPED}, "big_id": {REPLAY_SKIPPED}, "outside": {REPLAY_SKIPPED},
                       "bad_byte": {REPLAY_SKIPPED}, "masked": {REPLAY_SKIPPED}, "empty": {REPLAY_NOT_GOAL}}
    t_pid = torch.as_tensor(np.array(pid, np.int32), device=dev)
    t_plans = _pack(plans, cap, dev)
    t_len = torch.as_tensor(np.array(lens, np.int32), device=dev)
    t_mask = torch.as_tensor(np.array(mask, np.uint8), device=dev)
    t_pos = torch.as_tensor(np.stack(pos), device=dev)
    lens = np.array(lens, np.int64)
    results = {}
    for include, keep in (("valid", (REPLAY_VALID,)), ("replayed", (REPLAY_VALID, REPLAY_NOT_GOAL, REPLAY_EARLY))):
        out = replay_plans(vec, t_pid, t_plans, t_len, pos=t_pos, mask=t_mask, include=include, next_pos=True)
        assert (out.verdict.cpu().numpy() == want).all(), include
        assert (out.first_goal.cpu().numpy() == np.array(want_first)).all()
        rows = np.where(np.isin(want, keep), lens, 0)
        want_off = np.concatenate([[0], np.cumsum(rows)])
        assert (out.offset.cpu().numpy() == want_off).all()
        assert out.num_rows == want_off[-1] > 0
        item, t, rpos, act, rew, done, nxt = (x.cpu().numpy() for x in (out.item, out.t, out.pos, out.action, out.reward,
                                                                       out.done, out.next_pos))
        assert (item == np.repeat(np.arange(len(items)), rows)).all()  # exactly the expected row set, in order
        for i, (kind, k) in enumerate(items):
            if rows[i] == 0:
                continue
            states, rewards, terms, _ = _trace(cps[k], cps[k].initial_state, plans[i])
            lo, hi = want_off[i], want_off[i + 1]
            wp = np.stack([_padded(s, npad) for s in states])
            assert (t[lo:hi] == np.arange(hi - lo)).all() and (act[lo:hi] == np.array(plans[i], np.uint8)).all()
            assert (rpos[lo:hi] == wp[:-1]).all() and (nxt[lo:hi] == wp[1:]).all(), (i, kind)
            assert (rew[lo:hi].view(np.uint64) == np.array(rewards, np.float64).view(np.uint64)).all(), (i, kind)
            assert (done[lo:hi] == np.array(terms, np.uint8)).all()
        results[include] = (out, want_off[-1])
    assert results["replayed"][1] > results["valid"][1]

    # a row buffer smaller than the total: rows < cap are right, the rest is counted, nothing behind cap is written
    out, total = results["replayed"]
    cap_rows, guard = int(total) // 2, 64
    eng = vec.engine
    r_pos = torch.full((cap_rows + guard, npad, 2), 0x55, dtype=torch.int8, device=dev)
    r_act = torch.full((cap_rows + guard,), 0x55, dtype=torch.uint8, device=dev)
    r_rew = torch.full((cap_rows + guard,), -7.0, dtype=torch.float64, device=dev)
    r_done = torch.full((cap_rows + guard,), 0x55, dtype=torch.uint8, device=dev)
    r_item = torch.full((cap_rows + guard,), -7, dtype=torch.int32, device=dev)
    dropped = torch.full((1,), -1, dtype=torch.int64, device=dev)
    eng.plan_replay_emit(t_pid, t_pos, t_plans, t_len, t_mask, _capi.REPLAY_INCLUDE_REPLAYED, out.verdict, out.offset, cap_rows,
                         item=r_item, row_pos=r_pos, action=r_act, reward=r_rew, done=r_done, dropped=dropped)
    assert int(dropped.item()) == total - cap_rows
    assert torch.equal(r_pos[:cap_rows], out.pos[:cap_rows]) and torch.equal(r_act[:cap_rows], out.action[:cap_rows])
    assert torch.equal(r_rew[:cap_rows], out.reward[:cap_rows]) and torch.equal(r_done[:cap_rows], out.done[:cap_rows])
    assert torch.equal(r_item[:cap_rows], out.item[:cap_rows])
    assert (r_pos[cap_rows:] == 0x55).all() and (r_act[cap_rows:] == 0x55).all() and (r_done[cap_rows:] == 0x55).all()
    assert (r_rew[cap_rows:] == -7.0).all() and (r_item[cap_rows:] == -7).all()

    # npad below the set's largest number of movables is refused before any launch
    n_max = max(p.num_movables for p in vec.puzzles)
    assert n_max > 4
    rc = _capi.lib.pw_plan_replay_check(eng.handle, _capi._ptr(t_pid), None, 4, _capi._ptr(t_plans), _capi._ptr(t_len), cap,
                                        None, len(items), 0, _capi._ptr(out.verdict), None, None, _capi._ptr(out.offset), None)
    assert rc == _capi.PW_EINVAL and "npad" in _capi.last_error()


def test_goal_start_and_empty_plan():
    # puzzle.py:413-424: from a start that is a goal the empty plan is valid, any longer one reaches the goal early
    path, plan = _human()[0]
    vec = _engine([path], "python")
    dev, npad = vec.device, vec.num_objects_padded
    cp = _oracles([path], "python")[0]
    goal_state = _trace(cp, cp.initial_state, plan)[0][-1]
    assert cp.py.is_goal_state(goal_state)
    pos = torch.as_tensor(np.stack([_padded(goal_state, npad)] * 2 + [_padded(cp.initial_state, npad)]), device=dev)
    out = replay_plans(vec, torch.zeros(3, dtype=torch.int32, device=dev), _pack([[], [0, 1], []], 4, dev),
                       torch.as_tensor(np.array([0, 2, 0], np.int32), device=dev), pos=pos, include="replayed")
    assert out.verdict.tolist() == [REPLAY_VALID, REPLAY_EARLY, REPLAY_NOT_GOAL]
    assert out.first_goal.tolist() == [0, 0, -1]
    assert out.offset.tolist() == [0, 0, 2, 2] and out.num_rows == 2


def _random_vec(paths, per, order, seed, max_steps=30, observation=None, **kw):
    """`per` environments per puzzle, each left at the state after its own number (0 .. max_steps) of seeded random steps."""
    puzzles = [PushWorldPuzzle(p, order=order) for p in paths]
    ids = np.repeat(np.arange(len(paths)), per)
    vec = VecPushWorld(puzzles, len(ids), puzzle_ids=ids, observation=observation, max_steps=None, **kw)
    vec.reset()
    rng = np.random.default_rng(seed)
    stop = rng.integers(0, max_steps + 1, size=len(ids))
    chosen = vec.states().copy()
    for t in range(1, max_steps + 1):
        vec.step(torch.as_tensor(rng.integers(0, 4, size=len(ids)).astype(np.uint8), device=vec.device))
        now = vec.states()
        chosen[stop == t] = now[stop == t]
    vec.set_states(chosen)
    torch.cuda.synchronize()
    return vec, paths, ids


@pytest.mark.parametrize("big", [False, True])
def test_given_start_states(big):
    small = [p for p in LEVEL[1] if PushWorldPuzzle(p).num_movables <= 8][:6]
    paths = (REF_CPP[:5] + [CLEAN_SWEEP] + LEVEL[1][:4]) if big else (REF_CPP + small)
    vec, paths, ids = _random_vec(paths, 4, "cpp", seed=5 if big else 3)
    assert vec.num_objects_padded == (32 if big else 8)
    cps = _oracles(paths, "cpp")
    sp = vec.planner(heuristic="N+RGD", batch=8, max_states=1 << 14)
    try:
        info, plans, plan_len, _ = sp.plan(vec.puzzle_id, vec.pos, max_rounds=40, plan_cap=512)
        verdict = sp.validate().cpu().numpy()
        out = replay_plans(vec, vec.puzzle_id, plans, plan_len, pos=vec.pos)
        info, plans, plan_len = (x.cpu().numpy() for x in (info, plans, plan_len))
    finally:
        sp.close()
    assert (out.verdict.cpu().numpy() == verdict).all()
    final, start = out.final_pos.cpu().numpy(), vec.states()
    solved = info[:, 0] == 1
    assert solved.any() and (~solved).any()
    for i in range(len(ids)):
        cp = cps[ids[i]]
        if solved[i]:
            assert verdict[i] == REPLAY_VALID, i
            states, _, _, goals = _trace(cp, start[i][:cp.num_movables].tolist(), plans[i, :plan_len[i]].tolist())
            assert goals[-1] and cp.py.is_goal_state(tuple(map(tuple, final[i][:cp.num_movables].tolist())))
            assert (final[i] == _padded(states[-1], vec.num_objects_padded)).all()
        else:
            assert verdict[i] == REPLAY_NONE and plan_len[i] == -1, i
    assert out.num_rows == int(plan_len[solved].sum())


@pytest.mark.parametrize("observation", ["cells", "uint8"])
def test_demonstration_observations(observation):
    small = [p for p in LEVEL[1] if PushWorldPuzzle(p).num_movables <= 8][:6]
    vec, paths, ids = _random_vec(REF_CPP + small, 8, "python", seed=9, observation=observation, pixels_per_cell=3,
                                  border_width=1)
    sp = vec.planner(heuristic="N+RGD", batch=8, max_states=1 << 14)
    try:
        # behind a step on the same stream, with no synchronisation in between
        rng = np.random.default_rng(1)
        vec.step(torch.as_tensor(rng.integers(0, 4, size=len(ids)).astype(np.uint8), device=vec.device))
        pos0, obs0, steps0 = vec.pos.clone(), vec.obs.clone(), vec.steps.clone()  # (device copies: no wait)
        demo = vec.demonstrations(sp, max_rounds=100, plan_cap=512)
        torch.cuda.synchronize()
        plan_len = sp._out[2].cpu().numpy()
        plans = sp._out[1].cpu().numpy()
    finally:
        sp.close()
    T = demo.num_rows
    assert T >= 64 and demo.obs.shape[0] == T
    verdict, offset = demo.verdict.cpu().numpy(), demo.offset.cpu().numpy()
    assert (verdict == REPLAY_VALID).any() and (verdict == REPLAY_NONE).any()
    rpos, rpid, item, act = (x.cpu().numpy() for x in (demo.pos, demo.puzzle_id, demo.item, demo.action))
    starts = vec.states()
    first_rows = [int(offset[i]) for i in range(len(ids)) if offset[i + 1] > offset[i]]
    last_rows = [int(offset[i + 1]) - 1 for i in range(len(ids)) if offset[i + 1] > offset[i]]
    for i in range(len(ids)):
        if offset[i + 1] > offset[i]:
            assert (rpos[offset[i]] == starts[i]).all() and (rpid[offset[i]:offset[i + 1]] == ids[i]).all()
            assert (act[offset[i]:offset[i + 1]] == plans[i, :plan_len[i]]).all()
    sel = sorted(set(first_rows + last_rows + np.random.default_rng(2).choice(T, size=64, replace=False).tolist()))
    obs = demo.obs[torch.as_tensor(sel, device=vec.device)].cpu().numpy()
    if observation == "cells":
        _, hc, wc = vec.engine.cells_shape()
        for k, r in enumerate(sel):
            pz = vec.puzzles[rpid[r]]
            state = [(int(x), int(y)) for x, y in rpos[r][:pz.num_movables]]
            assert (obs[k] == pz.cells(state, frame=(hc, wc))).all(), r
    else:
        h, w, _ = vec.engine.obs_shape
        want = c_oracle.observe_batch(_oracles(paths, "python"), rpid, rpos, sel, h // 3, w // 3, 3, 1)
        assert obs.dtype == np.uint8 and (obs == want).all()
    # the environment itself is where the step left it
    assert torch.equal(vec.pos, pos0) and torch.equal(vec.obs, obs0) and torch.equal(vec.steps, steps0)


def test_plan_batch_validate_and_benchmark_rgd(tmp_path):
    from pushworld_amd.benchmark_rgd import PLANNER_NAMES, benchmark_rgd_planner, planning_result, yaml_dump

    paths = REF_CPP[:4]
    puzzles = [PushWorldPuzzle(p, order="cpp") for p in paths]
    pb = PlanBatch(puzzles, heuristic="N+RGD", batch=1, max_states=1 << 14)
    try:
        pb.run(max_rounds=200)
        verdict = pb.validate().cpu().numpy()
        res = pb.results()
    finally:
        pb.close()
    assert any(plan is not None for plan, _, _ in res)
    for (plan, pi, _), v, p in zip(res, verdict, paths):
        if plan is None:
            assert v == REPLAY_NONE
        else:
            assert (v == REPLAY_VALID) == PushWorldPuzzle(p).is_valid_plan(plan) and v == REPLAY_VALID

    # benchmark_rgd validates with one PlanBatch.validate(): its files are what one PushWorldPuzzle per plan gives
    src = tmp_path / "puzzles"
    src.mkdir()
    for p in paths:
        (src / os.path.basename(p)).write_text(open(p).read())
    got = benchmark_rgd_planner(str(tmp_path / "results"), str(src), heuristic="N+RGD", time_limit=None, max_states=1 << 14)
    assert len(got) == len(paths)
    for dst, result in got.items():
        name = os.path.splitext(os.path.basename(dst))[0]
        plan = result.get("plan")
        valid = True if plan is None else PushWorldPuzzle(str(src / (name + ".pwp"))).is_valid_plan(["LRUD".index(c) for c in plan])
        status = "solved" if plan is not None else {"no solution exists": "exhausted", "memory error": "limit"}.get(
            result.get("failure_reason"), "unknown")
        want = planning_result(PLANNER_NAMES["N+RGD"], name, status, plan, result["planning_time"], None, valid)
        assert open(dst).read() == yaml_dump(want)
    assert any(r.get("plan") for r in got.values())

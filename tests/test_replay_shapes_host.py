"""The inputs of tests/test_gpu_plan_replay_shapes.py pinned on the CPU before a device sees them: the puzzle sets, starts and
plans of tests/replay_cases.py.  Everything is asserted from the C oracle's traces alone: every set holds the verdict classes,
the plan lengths around the lane-group width and the plan_cap, the reward values, the traces that leave the grid and return and
the overlapping starts that the kernel has never been given."""
import numpy as np
import pytest

import replay_cases as RC
import shape_states as SS
import walk_restatement as WR

VALID, NOT_GOAL, EARLY = "valid", "not_goal", "early"
MULTI_GOAL = (8, 16)  # the sets with three-goal puzzles


def _verdict(goals):
    """puzzle.py:413-424 on the goal flags of the states a plan passes through."""
    if any(goals[:-1]):
        return EARLY
    return VALID if goals[-1] else NOT_GOAL


def test_sets_and_three_goal_variants():
    assert {n: [k[:3] for k in keys] for n, keys in RC.SETS.items()} == {
        4: [(3, 12, 9)], 8: [(3, 12, 9), (5, 30, 1), (8, 16, 2), (5, 30, 1), (8, 16, 2)],
        16: [(12, 30, 4), (12, 30, 4), (5, 30, 1)], 32: [(18, 30, 6), (32, 62, 5), (8, 16, 2)]}
    for npad, keys in RC.SETS.items():
        assert min(p for p in (4, 8, 16, 32) if p >= max(RC.puzzle(k).num_movables for k in keys)) == npad
    for key in RC.THREE:
        base, cp = SS.puzzle(key[:3]), RC.puzzle(key)
        a, b = SS.text(key[:3]).split(), RC.text(key).split()
        changed = [(x, y) for x, y in zip(a, b) if x != y]
        assert sorted(changed) == [(".", "G1"), (".", "G2")]  # two free cells turned into goals, nothing else
        assert cp.num_goals == 3 and cp.py.names[:4] == ["a", "m2", "m1", "m0"] and cp.num_movables == base.num_movables
        assert (cp.width, cp.height) == (base.width, base.height) and cp.py.wall_cells == base.py.wall_cells
        listed = RC.states(key)
        assert [k for k, _ in listed] == ["initial"] + ["near"] * 6 + ["far"] * 10 + ["goal_near"] * 6
        assert all(WR.in_grid(cp, s) for _, s in listed)
        finish = RC.finish_starts(key)
        assert len(finish) >= 3
        for start, action in finish:  # every goal movable on its goal but one, which the oracle's step pushes home
            off = [g for g in range(3) if start[1 + g] != cp.py.goal_state[g]]
            assert len(off) == 1 and WR.in_grid(cp, start) and not cp.py.is_goal_state(start)
            nxt, reward, term = cp.env_step(start, action)
            assert term and reward == 10.0 and cp.py.is_goal_state(nxt)


@pytest.mark.parametrize("npad", [4, 8, 16, 32])
def test_items(npad):
    items = RC.items(npad)
    ids, pos, plans, lens = RC.packed(npad)
    assert plans.shape == (len(items), RC.CAP) and RC.CAP % RC.gs(npad) != 0
    verdicts = {VALID: 0, NOT_GOAL: 0, EARLY: 0}
    rewards, leave, overlapping, off_and_back = set(), 0, 0, 0
    for i, it in enumerate(items):
        cp = RC.puzzle(it.key)
        assert it.key == RC.SETS[npad][it.pid] and WR.in_grid(cp, it.start)  # (the check kernel skips other starts)
        tr = RC.item_trace(it)
        assert all(RC.in_domain(cp, s) for s in tr.states) and len(it.plan) <= RC.CAP
        assert (plans[i, :lens[i]] == np.array(it.plan, np.uint8)).all() and (plans[i, lens[i]:] == RC.FILL).all()
        v = _verdict(tr.goals)
        verdicts[v] += 1
        if it.kind in ("valid", "early"):
            assert v == it.kind, (i, it)
        rewards |= set(tr.rewards)
        leave += RC.leaves_and_returns(cp, tr.states)
        overlapping += SS.overlapping(cp, it.start)
        r = tr.rewards
        off_and_back += bool(r) and r[-1] == 10.0 and 0.99 in r[:-1] and -1.01 in r[:-1]
        if it.kind == "off_and_back":
            assert v == VALID and 0.99 in r[:-1] and -1.01 in r[:-1]
    assert min(verdicts.values()) >= 8, verdicts
    assert set(RC.lengths(npad)) <= set(lens.tolist())  # 0, 1, GS - 1, GS, GS + 1, 2 GS, 2 GS + 1, CAP - 1, CAP
    assert int(lens.max()) == RC.CAP  # len == plan_cap; the last item of the buffer is checked by the launch shapes
    assert rewards >= ({10.0, 0.99, -1.01, -0.01} if npad in MULTI_GOAL else {10.0, -0.01}), rewards
    assert leave >= 10, leave
    assert 2 * overlapping >= len(items)
    if npad in MULTI_GOAL:  # (a one-goal puzzle never pays 0.99)
        assert off_and_back >= 1
    # every start of every puzzle of the set is there
    assert {(it.pid, it.start) for it in items} >= {(pid, s) for pid, key in enumerate(RC.SETS[npad]) for s in RC.starts(key)}

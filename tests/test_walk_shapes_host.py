"""The inputs of tests/test_gpu_walk_shapes.py and tests/test_gpu_push_search_shapes.py, pinned on the CPU before a device sees
them: the state lists of tests/shape_states.py (random-shape puzzles, states with overlaps).
  * the two restatements of the step function (the compiled C oracle, ``oracle.pw_oracle.OraclePuzzle``'s table lookups) agree
    on every (q, a) that the walk restatement evaluates on these states;
  * coverage conditions, asserted from the restatement alone: the lists do hold the rows that only states with overlaps give
    (successors outside the grid, goal rows among them), long push chains, moved bits >= 16, the largest board;
  * a board worked out by hand on which a push move leaves the grid."""
import pytest

import push_search_restatement as PR
import shape_states as SS
import walk_restatement as WR
from oracle import c_oracle, pw_oracle

_STATS = {}


def _stats(case):
    """Per listed state of the case: (region, rows outside the grid, goal rows, goal rows outside the grid)."""
    if case not in _STATS:
        cp = SS.puzzle(case)
        out = []
        for _, s in SS.states(case):
            r = SS.region(case, s)
            outside = [pm for pm in r.pushes if not WR.in_grid(cp, pm.next_state)]
            goal = [pm for pm in r.pushes if pm.goal]
            out.append((r, outside, goal, [pm for pm in goal if not WR.in_grid(cp, pm.next_state)]))
        _STATS[case] = out
    return _STATS[case]


@pytest.mark.parametrize("case", SS.CASES)
def test_puzzles_and_lists(case):
    n, size, _ = case
    cp = SS.puzzle(case)
    assert (cp.width, cp.height) == (SS.FRAME[case],) * 2 == (size + 2,) * 2 and cp.num_movables == n
    assert cp.py.sizes[0] == SS.AGENT[case] and cp.num_goals == 1
    assert min(p for p in (4, 8, 16, 32) if p >= n) == SS.PADDING[case]
    listed = SS.states(case)
    near, far, goal_near = SS.COUNTS[case]
    assert [k for k, _ in listed] == ["initial"] + ["near"] * near + ["far"] * far + ["goal_near"] * goal_near
    assert len(listed) == (8 if size == 62 else 31) and listed[0].state == cp.initial_state
    assert all(WR.in_grid(cp, s) and len(s) == n for _, s in listed)  # the starts are inside; their successors need not be
    assert not SS.overlapping(cp, cp.initial_state)
    for kind, s in listed:
        if kind == "goal_near":  # the goal movable is one cell from its goal
            (gx, gy), (x, y) = cp.py.goal_state[0], s[1]
            assert abs(gx - x) + abs(gy - y) == 1


@pytest.mark.parametrize("case", SS.CASES)
def test_two_oracles_agree(case):
    """Every (q, a) the restatement evaluated on the listed states (its step cache holds them), C oracle against the Python
    oracle's table lookups."""
    cp = SS.puzzle(case)
    tables = pw_oracle.OraclePuzzle(SS.text(case))
    assert tables.initial_state == cp.initial_state and tables.sizes == cp.py.sizes
    checked = 0
    for _, s in SS.states(case):
        r = SS.region(case, s)
        steps = WR._steps(cp, tuple(s[1:]))
        assert all((q, a) in steps for q in r.dist for a in range(4))
        for q in r.dist:
            placed = (q,) + tuple(s[1:])
            for a in range(4):
                assert steps[(q, a)] == tables.get_next_state_moved(placed, a), (case, placed, a)
                checked += 1
    assert checked >= 4 * len(SS.states(case))


@pytest.mark.parametrize("case", SS.CASES)
def test_coverage(case):
    cp = SS.puzzle(case)
    listed, stats = SS.states(case), _stats(case)
    # at least one third of the listed states have somewhere to walk and something to push
    assert 3 * sum(1 for r, *_ in stats if len(r.dist) >= 2 and len(r.pushes) >= 1) >= len(listed)
    assert sum(len(outside) for _, outside, _, _ in stats) >= 1  # a successor outside its grid
    assert any(bin(pm.moved).count("1") >= 3 for r, *_ in stats for pm in r.pushes)  # the agent and two more in one push
    assert any(SS.overlapping(cp, s) and SS.agent_overlaps(cp, s) for _, s in listed)
    assert all(pm.moved & 1 and len(pm.next_state) == cp.num_movables for r, *_ in stats for pm in r.pushes)
    if SS.PADDING[case] == 32:
        assert any(pm.moved >> 16 for r, *_ in stats for pm in r.pushes)
    if case == SS.CASES[5]:
        assert cp.num_movables == 32 and all(len(s) == 32 for _, s in listed)
        assert max(max(r.dist.values()) for r, *_ in stats) > 100
        assert any(q[1] == 62 for r, *_ in stats for q in r.dist)
        assert any(pm.moved >> 31 for r, *_ in stats for pm in r.pushes)  # the last lane of the 32-lane group


def test_goal_rows():
    assert sum(len(goal) for case in SS.CASES for *_, goal, _ in _stats(case)) >= 5
    case = SS.CASES[2]
    cp = SS.puzzle(case)
    stats = _stats(case)
    for k in SS.GOAL_OUTSIDE_LISTED:  # a goal row whose successor is outside its grid, and the first goal row of its state
        r, _, goal, goal_outside = stats[k]
        assert goal_outside and goal[0] is goal_outside[0]
        st = SS.store(case, SS.states(case)[k].state)
        assert st.pushes == 1 and st.goal_index == st.num_states - 1 >= 2 and st.canons[-1] == (0, 0)
        assert st.states[-1] == goal[0].next_state and not WR.in_grid(cp, st.states[-1])
    for start in SS.GOAL_OUTSIDE_STARTS:  # the same in the third layer of a search
        assert WR.in_grid(cp, start) and SS.overlapping(cp, start)
        st = SS.store(case, start)
        assert st.pushes == 3 and st.goal_index == st.num_states - 1 >= 30
        assert st.links[-1].goal and not WR.in_grid(cp, st.states[-1]) and st.canons[-1] == (0, 0)
        assert all(WR.in_grid(cp, s) for s in st.states[:-1]) and not any(ln.goal for ln in st.links[:-1])
        # the search by walk_restatement.push_search does not count the successor it cannot close
        want = WR.push_search(cp, start=start)
        assert want.num_states == st.num_states - 1 and want.plan == PR.plan_of(cp, st, st.goal_index)


@pytest.mark.parametrize("case", SS.SMALL)
def test_search_starts(case):
    cp = SS.puzzle(case)
    starts = SS.search_starts(case)
    assert len(starts) == len(set(starts)) == 4
    for start in starts:
        assert WR.in_grid(cp, start) and SS.overlapping(cp, start)
        st = SS.store(case, start, stop_at_goal=False, max_pushes=3)
        assert 20 <= st.num_states <= 400 and len(st.layer_states) == 3 and st.goal_index == -1
        expanded = st.states[:st.layers[3][0]] if len(st.layers) == 4 else st.states
        assert any(not WR.in_grid(cp, pm.next_state) for s in expanded for pm in WR.region(cp, s).pushes)
        assert all(WR.in_grid(cp, s) for s in st.states)  # and none of them is in the store
    goals = [SS.store(case, s, max_pushes=3) for s in SS.goal_starts(case)]
    assert sum(1 for st in goals if st.pushes == 1) >= 2 and sum(1 for st in goals if (st.pushes or 0) >= 2) >= 1
    for start in SS.DEEP_GOAL_STARTS[case]:
        assert SS.overlapping(cp, start)


# A board of 6 x 4 cells with its border.  The start state below puts the bar M1 (two cells) on the right border column:
#      x 0 1 2 3 4 5
#  y 0   W W W W W W
#  y 1   W A . . M1M1      (M1 at (4, 1): its second cell lies on the border wall (5, 1))
#  y 2   W M0. . G0W
#  y 3   W W W W W W
BORDER = "A . M1 M1\nM0 . . G0\n"


def test_hand_worked_push_out_of_the_grid():
    p = c_oracle.COraclePuzzle(BORDER)
    assert (p.width, p.height, p.num_movables, p.py.names) == (6, 4, 3, ["a", "m0", "m1"])
    assert p.py.sizes == [(1, 1), (1, 1), (2, 1)] and p.initial_state == ((1, 1), (1, 2), (3, 1))
    start = ((1, 1), (1, 2), (4, 1))
    assert WR.in_grid(p, start) and SS.overlapping(p, start) and not SS.agent_overlaps(p, start)
    reg = WR.region(p, start)
    # M0 cannot be pushed (DOWN from (1, 1) and LEFT from (2, 2) end at the border).  M1 overlaps a wall already, so no wall
    # stops it: RIGHT from (3, 1) pushes it to (5, 1), out of the grid; UP from (4, 2) pushes it onto the top border, inside.
    assert reg.dist == {(1, 1): 0, (2, 1): 1, (3, 1): 2, (2, 2): 2, (3, 2): 3, (4, 2): 4}
    assert reg.parent == {(2, 1): 1, (3, 1): 1, (2, 2): 3, (3, 2): 1, (4, 2): 1}  # (3, 2): RIGHT from (2, 2) before DOWN from (3, 1)
    assert reg.canon == (1, 1)
    out_of_grid = ((4, 1), (1, 2), (5, 1))
    onto_border = ((4, 1), (1, 2), (4, 0))
    assert reg.pushes == [
        WR.Push((3, 1), 1, 2, 0b101, False, out_of_grid),
        WR.Push((4, 2), 2, 4, 0b101, False, onto_border),
    ]
    assert not WR.in_grid(p, out_of_grid) and WR.in_grid(p, onto_border)
    # after the push UP the agent stands where the bar was; the bar lies on the top border and nothing can be pushed any more
    after = WR.region(p, onto_border)
    assert sorted(after.dist) == [(1, 1), (2, 1), (2, 2), (3, 1), (3, 2), (4, 1), (4, 2)] and after.pushes == [] and after.canon == (1, 1)
    st = PR.search_store(p, start=start, max_pushes=2)
    assert st.states == [start, onto_border] and out_of_grid not in st.states
    assert st.canons == [(1, 1), (1, 1)]
    assert st.links == [PR.Link(-1, (0, 0), PR.ROOT_ACTION, 0, False), PR.Link(0, (4, 2), 2, 4, False)]
    assert st.layers == [(0, 1), (1, 1)] and st.layer_states == [1, 0]
    assert (st.num_states, st.goal_index, st.pushes, st.push_rows, st.largest_region) == (2, -1, None, 2, 7)
    assert PR.plan_of(p, st, 1) == [1, 3, 1, 1, 2]
    want = WR.push_search(p, start=start, max_pushes=2)
    assert (want.plan, want.layer_states, want.num_states, want.push_rows, want.largest_region) == (None, [1, 0], 2, 2, 7)

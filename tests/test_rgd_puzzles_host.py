"""The constructed RGD puzzles of tests/rgd_puzzles.py, pinned with the plain-Python restatement so that the inputs of
tests/test_gpu_rgd_deep.py cannot drift: each ladder's cost and recursion calls, its first finite pushing depth, how many walk
states the restatement gives up on, and ``pw_puzzle_movement_graph`` against ``R.movement_graphs``.  No GPU."""
import math
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deep_puzzles  # noqa: E402
import rgd_puzzles as P  # noqa: E402
import rgd_restatement as R  # noqa: E402
from oracle import pw_oracle  # noqa: E402
from pushworld_amd import _capi  # noqa: E402
from pushworld_amd.puzzle import PushWorldPuzzle, masks_to_graph  # noqa: E402

# (k, gap) -> calls of the initial state at full depth, with fewest_tools (None: more than 300 000, never evaluated)
INITIAL_CALLS = {
    (2, 0): (2, 3), (3, 0): (3, 6), (16, 0): (16, 136), (17, 0): (17, 153), (31, 0): (31, 496),
    (2, 1): (4, 6), (3, 1): (10, 18), (12, 1): (208, 1242), (16, 1): (415, 4552), (17, 1): (574, 8810),
    (20, 1): (1072, 33909), (28, 1): (4694, None), (12, 3): (474, 2521),
}


def test_shapes():
    def dims(text):
        pz = PushWorldPuzzle(text=text)
        return tuple(pz.dimensions), pz.num_movables

    assert dims(P.ladder(31, 0)) == ((37, 33), 32)   # PW_MAX_OBJECTS movables, levels = 30
    assert dims(P.ladder(28, 1)) == ((61, 30), 29)
    assert dims(P.ladder(12, 3)) == ((51, 14), 13)
    assert dims(P.room(62, 62)) == ((64, 64), 2)     # PW_MAX_DIM
    assert sorted(INITIAL_CALLS) == sorted(P.LADDERS)
    for bad in ((31, 1), (30, 1), (15, 3)):
        with pytest.raises(AssertionError):
            P.ladder(*bad)


@pytest.mark.parametrize("k,gap", P.LADDERS)
def test_ladder_cost_calls_and_first_finite_depth(k, gap):
    oz = pw_oracle.OraclePuzzle(P.ladder(k, gap))
    assert oz.num_movables == k + 1 and oz.names[:3] == ["a", "m1", "m2"] and oz.names[-1] == "m%d" % k
    s0, goal = oz.initial_state, oz.goal_state[0]
    full = R.RecursiveGraphDistance(oz, fewest_tools=False)
    assert full.estimate(s0) == P.ladder_cost(k, gap)
    assert full.calls == INITIAL_CALLS[(k, gap)][0]
    # the first finite pushing depth is exactly k - 1 = N - 2
    assert full.goal_cost(s0, 1, goal, k - 1) == P.ladder_cost(k, gap)
    if INITIAL_CALLS[(k, gap)][1] is not None and INITIAL_CALLS[(k, gap)][1] < 10000:
        assert math.isinf(full.goal_cost(s0, 1, goal, k - 2))
        few = R.RecursiveGraphDistance(oz, fewest_tools=True, graphs=full.graphs)
        assert few.estimate(s0) == P.ladder_cost(k, gap)
        assert few.calls == INITIAL_CALLS[(k, gap)][1]
    else:  # depth k - 2 takes tens of thousands of calls: one depth short of each of the two halves is as telling
        assert math.isinf(full.goal_cost(s0, 1, goal, min(k - 2, 10)))


@pytest.mark.parametrize("k,gap,fewest", [m for m in P.MODES if P.max_calls(*m) <= 9000])
def test_walk_states_the_restatement_gives_up_on(k, gap, fewest):
    """The skipped-state caps of the GPU test hold for the restatement alone.  ((31, 0) with fewest_tools, 5 s on the host,
    is left to the GPU test: 61 states, none skipped at 140 000 calls, the largest 132 230.)"""
    text, states, costs, calls = P.ladder_reference(k, gap, fewest)
    skipped = costs.count(None)
    assert costs[0] == P.ladder_cost(k, gap)
    assert len(states) == P.WALK_STEPS + 1  # measured: no walk had to be shortened
    if (k, gap) in P.NEVER_SKIPPED:
        assert skipped == 0
    assert skipped <= P.SKIP_CAP * len(states)  # (measured: 0 everywhere; 12, 3 is the one case outside NEVER_SKIPPED)
    assert len(set(costs)) >= 2 and len(set(states)) >= 5


CONSTRUCTED = [("ladder %d %d" % kg, lambda kg=kg: P.ladder(*kg)) for kg in P.LADDERS] + [
    ("room 62x62", lambda: P.room(62, 62)),
    ("room 5x4", lambda: P.room(5, 4)),
    ("serpentine 62x61", lambda: deep_puzzles.serpentine(62, 61)),
    ("serpentine 14x13 overshoot", lambda: deep_puzzles.serpentine(14, 13, True)),
]


@pytest.mark.parametrize("name,make", CONSTRUCTED, ids=[c[0] for c in CONSTRUCTED])
def test_movement_graph_equals_the_restatement(name, make):
    text = make()
    oz = pw_oracle.OraclePuzzle(text, "python")
    want = dict(zip(oz.names, R.movement_graphs(oz)))
    for order in (_capi.ORDER_PYTHON, _capi.ORDER_CPP):
        pp = _capi.ParsedPuzzle(text, order)
        assert len(pp.names) == len(want)
        for j, nm in enumerate(pp.names):
            assert masks_to_graph(pp.movement_graph_masks(j)) == want[nm], (name, order, nm)


def test_room_and_serpentine_graphs():
    room = R.movement_graphs(pw_oracle.OraclePuzzle(P.room(62, 62)))
    assert [len(g) for g in room] == [3844, 3844]
    assert (62, 62) in room[1] and room[1][(62, 62)] == set()  # the box never leaves the corner
    oz = pw_oracle.OraclePuzzle(deep_puzzles.serpentine(62, 61))
    g = R.movement_graphs(oz)
    path = [(x + 1, y + 1) for x, y in deep_puzzles.serpentine_path(62, 61)]
    assert sorted(g[0]) == sorted(path) and len(path) == 1952
    # the box: the last row, pushed both ways (the agent's graph ignores the box) into the two end cells it never leaves
    assert sorted(g[1]) == [(x, 61) for x in range(1, 63)] and g[1][(1, 61)] == g[1][(62, 61)] == set()
    box = R.PathDistances(g[1])
    assert box.get(path[-3], path[-1]) == 2 and math.isinf(box.get(path[-1], path[-3]))
    assert R.PathDistances(g[0]).get(path[0], path[-1]) == len(path) - 1

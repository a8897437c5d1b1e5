"""The inputs of tests/test_gpu_push_plan_batch_limits.py, pinned on the CPU before a device sees them: the runs of
tests/push_plan_limit_cases.py restated by tests/push_planner_restatement.py (K17's semantics, which K24 must reproduce).
  * the ten info words of every run, as literals: after its last round, and for the runs that the device also stops earlier
    (the states form of part 1, the shapes at K = 8) after four rounds;
  * what each case was chosen for, asserted from the restatement alone, so that a change of a generator cannot quietly empty a
    case: 6, 7 and 8 movables and a board 16 cells high among items of 3 movables, 16 x 16 frames with movables at x = 15 and
    y = 15 and queues of NaN and +inf keys only, RGD budgets that overrun beside finite keys, a goal state outside its grid
    through movable 7, plans of more than one push for ``push_cap``, the round in which `Seeing Red` first pushes a key of 25.

One figure differs from the issue that asked for these cases: of the 48 listed shape starts at K = 8, nine (not "at least ten")
are still running with 40 or more states after four rounds -- (8, 3) start 12 has 39.  Ten are asserted where the device runs
them, over the eight-round runs at K = 8 (twelve are), and the nine after four rounds are pinned as they are.
The restatements take about 25 s of CPU in all; the longest, `Shape Of You` at K = 64, about 6 s."""
import pytest

import push_plan_limit_cases as C
import push_planner_restatement as PP
import shape_states as SS
from test_push_planner_host import check_store_invariants

R, E, S = "running", "exhausted", "solved"

# status, rounds, expanded, states, open, goal index, RGD overruns, push rows, largest region, largest key
PINNED_LEVEL1 = {
    ("Shape Of You", 1): (R, 8, 8, 98, 90, -1, 0, 178, 40, 14),
    ("Shape Of You", 8): (R, 8, 57, 686, 629, -1, 0, 1346, 45, 17),
    ("Shape Of You", 64): (S, 8, 390, 3020, 2624, 3019, 0, 8675, 45, 18),
    ("Seeing Red", 1): (R, 8, 8, 97, 89, -1, 0, 158, 45, 24),
    ("Seeing Red", 8): (S, 5, 33, 278, 238, 277, 0, 669, 45, 25),
    ("Seeing Red", 64): (S, 5, 207, 1044, 835, 1043, 0, 4036, 45, 27),
    ("Victory Road", 1): (S, 6, 6, 22, 15, 21, 0, 26, 26, 11),
    ("Victory Road", 8): (S, 6, 31, 91, 59, 90, 0, 135, 26, 11),
    ("Victory Road", 64): (S, 6, 105, 120, 14, 119, 0, 390, 26, 11),
    ("Pick A Tool", 1): (S, 5, 5, 8, 2, 7, 0, 7, 26, 10),
    ("Pick A Tool", 8): (S, 3, 7, 8, 0, 7, 0, 9, 26, 10),
    ("Pick A Tool", 64): (S, 3, 7, 8, 0, 7, 0, 9, 26, 10),
    ("Swiss Army Knife", 1): (R, 8, 8, 15, 7, -1, 0, 44, 77, 19),
    ("Swiss Army Knife", 8): (R, 8, 46, 147, 101, -1, 0, 421, 82, 19),
    ("Swiss Army Knife", 64): (R, 8, 206, 600, 394, -1, 0, 2388, 83, 20),
    ("Two Goals", 1): (S, 4, 4, 17, 12, 16, 0, 36, 68, 15),
    ("Two Goals", 8): (S, 4, 23, 45, 21, 44, 0, 208, 68, 17),
    ("Two Goals", 64): (S, 4, 51, 52, 0, 51, 0, 434, 68, 17),
    ("Single Obstacle", 1): (S, 4, 4, 8, 3, 7, 0, 8, 30, 4),
    ("Single Obstacle", 8): (S, 3, 8, 9, 0, 8, 0, 12, 30, 4),
    ("Single Obstacle", 64): (S, 3, 8, 9, 0, 8, 0, 12, 30, 4),
}
# the states form: K = 8 after four rounds
PINNED_LIVE = {
    "Shape Of You": (R, 4, 25, 249, 224, -1, 0, 555, 40, 17),
    "Seeing Red": (R, 4, 25, 271, 246, -1, 0, 531, 45, 25),
    "Victory Road": (R, 4, 15, 38, 23, -1, 0, 37, 26, 11),
    "Pick A Tool": PINNED_LEVEL1["Pick A Tool", 8],
    "Swiss Army Knife": (R, 4, 14, 29, 15, -1, 0, 90, 82, 19),
    "Two Goals": PINNED_LEVEL1["Two Goals", 8],
    "Single Obstacle": PINNED_LEVEL1["Single Obstacle", 8],
}

_E2, _E83, _E61, _E75 = (E, 2, 2, 2, 0, -1, 0, 2, 1, -1), (E, 2, 2, 2, 0, -1, 0, 1, 4, -1), (E, 3, 3, 3, 0, -1, 0, 4, 32, -1), \
    (E, 1, 1, 1, 0, -1, 0, 0, 2, -1)
# per K: the 13 starts of (8, 2), of (8, 3), of (6, 1) and of (7, 5) after at most eight rounds
PINNED_SHAPES = {
    1: [
        _E2, (R, 8, 8, 14, 6, -1, 0, 19, 13, -1), _E2, _E2, _E2, (E, 6, 6, 6, 0, -1, 0, 25, 6, -1),
        (R, 8, 8, 29, 21, -1, 0, 37, 23, -1), (R, 8, 8, 17, 9, -1, 0, 31, 20, -1), (R, 8, 8, 31, 23, -1, 0, 33, 15, -1),
        (R, 8, 8, 26, 18, -1, 0, 38, 28, -1), (R, 8, 8, 23, 15, -1, 0, 40, 6, -1), (R, 8, 8, 21, 13, -1, 0, 28, 23, -1),
        (R, 8, 8, 28, 20, -1, 0, 42, 20, -1),
        _E83, (E, 1, 1, 1, 0, -1, 0, 0, 4, -1), _E83, _E83, _E83, (R, 8, 8, 9, 1, -1, 0, 11, 25, -1), _E83,
        (E, 2, 2, 2, 0, -1, 0, 1, 3, -1), (E, 3, 3, 3, 0, -1, 0, 11, 12, -1), (E, 7, 7, 7, 0, -1, 0, 11, 10, -1),
        (R, 8, 8, 15, 7, -1, 0, 23, 47, -1), (R, 8, 8, 11, 3, -1, 0, 16, 13, -1), (R, 8, 8, 21, 13, -1, 0, 29, 28, -1),
        _E61, (R, 8, 8, 9, 1, -1, 0, 17, 32, -1), _E61, _E61, (E, 4, 4, 4, 0, -1, 0, 6, 33, -1), (E, 6, 6, 6, 0, -1, 0, 25, 51, -1),
        _E61, (R, 8, 8, 34, 26, -1, 0, 85, 38, -1), (R, 8, 8, 14, 6, -1, 0, 26, 14, -1), (R, 8, 8, 18, 10, -1, 0, 37, 44, -1),
        (R, 8, 8, 19, 11, -1, 0, 77, 52, -1), (R, 8, 8, 12, 4, -1, 0, 28, 27, -1), (E, 2, 2, 2, 0, -1, 0, 6, 29, -1),
        _E75, (R, 8, 8, 12, 4, -1, 0, 20, 26, -1), _E75, (E, 1, 1, 1, 0, -1, 0, 0, 3, -1), (E, 3, 3, 3, 0, -1, 0, 2, 3, -1), _E75,
        _E75, (R, 8, 8, 11, 3, -1, 0, 12, 14, -1), (E, 1, 1, 1, 0, -1, 0, 0, 11, -1), (E, 6, 6, 6, 0, -1, 0, 10, 28, -1),
        (R, 8, 8, 9, 1, -1, 0, 20, 4, -1), (E, 1, 1, 1, 0, -1, 0, 2, 5, -1), (R, 8, 8, 17, 9, -1, 0, 24, 9, -1),
    ],
    8: [
        _E2, (R, 8, 55, 63, 8, -1, 0, 121, 13, -1), _E2, _E2, _E2, (E, 3, 6, 6, 0, -1, 0, 25, 6, -1),
        (R, 8, 57, 85, 28, -1, 0, 169, 23, -1), (R, 8, 55, 98, 43, -1, 0, 182, 20, -1), (R, 8, 57, 81, 24, -1, 0, 181, 25, -1),
        (R, 8, 57, 102, 45, -1, 0, 194, 28, -1), (R, 8, 51, 89, 38, -1, 0, 252, 6, -1), (R, 8, 55, 96, 41, -1, 0, 195, 23, -1),
        (R, 8, 57, 98, 41, -1, 0, 156, 20, -1),
        _E83, (E, 1, 1, 1, 0, -1, 0, 0, 4, -1), _E83, _E83, _E83, (E, 4, 12, 12, 0, -1, 0, 14, 25, -1), _E83,
        (E, 2, 2, 2, 0, -1, 0, 1, 3, -1), (E, 2, 3, 3, 0, -1, 0, 11, 12, -1), (E, 4, 7, 7, 0, -1, 0, 11, 10, -1),
        (R, 8, 57, 106, 49, -1, 0, 237, 47, -1), (E, 7, 12, 12, 0, -1, 0, 23, 13, -1), (R, 8, 57, 65, 8, -1, 0, 111, 28, -1),
        _E61, (R, 8, 20, 26, 6, -1, 0, 47, 34, -1), _E61, _E61, (E, 3, 4, 4, 0, -1, 0, 6, 33, -1), (E, 4, 6, 6, 0, -1, 0, 25, 51, -1),
        _E61, (R, 8, 57, 128, 71, -1, 0, 506, 47, -1), (R, 8, 49, 73, 24, -1, 0, 150, 43, -1), (R, 8, 20, 23, 3, -1, 0, 95, 45, -1),
        (S, 4, 25, 50, 18, 49, 0, 142, 52, -1), (R, 8, 23, 24, 1, -1, 0, 69, 29, -1), (E, 2, 2, 2, 0, -1, 0, 6, 29, -1),
        _E75, (E, 4, 14, 14, 0, -1, 0, 32, 26, -1), _E75, (E, 1, 1, 1, 0, -1, 0, 0, 3, -1), (E, 3, 3, 3, 0, -1, 0, 2, 3, -1), _E75,
        _E75, (E, 4, 12, 12, 0, -1, 0, 22, 14, -1), (E, 1, 1, 1, 0, -1, 0, 0, 11, -1), (E, 3, 6, 6, 0, -1, 0, 10, 28, -1),
        (E, 6, 12, 12, 0, -1, 0, 31, 4, -1), (E, 1, 1, 1, 0, -1, 0, 2, 5, -1), (E, 7, 36, 36, 0, -1, 0, 82, 9, -1),
    ],
    64: [
        _E2, (R, 8, 61, 66, 5, -1, 0, 130, 13, -1), _E2, _E2, _E2, (E, 3, 6, 6, 0, -1, 0, 25, 6, -1),
        (R, 8, 219, 361, 142, -1, 0, 634, 23, -1), (R, 8, 262, 476, 214, -1, 0, 1307, 20, -1),
        (R, 8, 350, 514, 164, -1, 0, 973, 25, -1), (R, 8, 322, 552, 230, -1, 0, 932, 28, -1),
        (R, 8, 138, 157, 19, -1, 0, 679, 6, -1), (R, 8, 283, 518, 235, -1, 0, 925, 23, -1),
        (R, 8, 386, 726, 340, -1, 0, 1255, 20, -1),
        _E83, (E, 1, 1, 1, 0, -1, 0, 0, 4, -1), _E83, _E83, _E83, (E, 4, 12, 12, 0, -1, 0, 14, 25, -1), _E83,
        (E, 2, 2, 2, 0, -1, 0, 1, 3, -1), (E, 2, 3, 3, 0, -1, 0, 11, 12, -1), (E, 4, 7, 7, 0, -1, 0, 11, 10, -1),
        (R, 8, 358, 518, 160, -1, 0, 1675, 47, -1), (E, 7, 12, 12, 0, -1, 0, 23, 13, -1), (R, 8, 93, 112, 19, -1, 0, 191, 28, -1),
        _E61, (R, 8, 20, 26, 6, -1, 0, 47, 34, -1), _E61, _E61, (E, 3, 4, 4, 0, -1, 0, 6, 33, -1), (E, 4, 6, 6, 0, -1, 0, 25, 51, -1),
        _E61, (R, 8, 315, 532, 217, -1, 0, 2900, 56, -1), (R, 8, 84, 101, 17, -1, 0, 237, 43, -1),
        (R, 8, 20, 23, 3, -1, 0, 95, 45, -1), (S, 3, 29, 51, 0, 50, 0, 187, 52, -1), (R, 8, 23, 24, 1, -1, 0, 69, 29, -1),
        (E, 2, 2, 2, 0, -1, 0, 6, 29, -1),
        _E75, (E, 4, 14, 14, 0, -1, 0, 32, 26, -1), _E75, (E, 1, 1, 1, 0, -1, 0, 0, 3, -1), (E, 3, 3, 3, 0, -1, 0, 2, 3, -1), _E75,
        _E75, (E, 4, 12, 12, 0, -1, 0, 22, 14, -1), (E, 1, 1, 1, 0, -1, 0, 0, 11, -1), (E, 3, 6, 6, 0, -1, 0, 10, 28, -1),
        (E, 6, 12, 12, 0, -1, 0, 31, 4, -1), (E, 1, 1, 1, 0, -1, 0, 2, 5, -1), (E, 7, 36, 36, 0, -1, 0, 82, 9, -1),
    ],
}
# K = 8 after four rounds, the runs the issue's coverage figures were taken from
PINNED_SHAPES_COVER = [
    _E2, (R, 4, 23, 34, 11, -1, 0, 57, 13, -1), _E2, _E2, _E2, (E, 3, 6, 6, 0, -1, 0, 25, 6, -1),
    (R, 4, 25, 45, 20, -1, 0, 85, 23, -1), (R, 4, 23, 45, 22, -1, 0, 89, 20, -1), (R, 4, 25, 51, 26, -1, 0, 92, 25, -1),
    (R, 4, 25, 54, 29, -1, 0, 94, 28, -1), (R, 4, 19, 43, 24, -1, 0, 93, 6, -1), (R, 4, 23, 49, 26, -1, 0, 82, 23, -1),
    (R, 4, 25, 62, 37, -1, 0, 89, 20, -1),
    _E83, (E, 1, 1, 1, 0, -1, 0, 0, 4, -1), _E83, _E83, _E83, (R, 4, 12, 12, 0, -1, 0, 14, 25, -1), _E83,
    (E, 2, 2, 2, 0, -1, 0, 1, 3, -1), (E, 2, 3, 3, 0, -1, 0, 11, 12, -1), (R, 4, 7, 7, 0, -1, 0, 11, 10, -1),
    (R, 4, 25, 65, 40, -1, 0, 122, 47, -1), (R, 4, 8, 10, 2, -1, 0, 16, 13, -1), (R, 4, 25, 39, 14, -1, 0, 62, 28, -1),
    _E61, (R, 4, 9, 12, 3, -1, 0, 21, 32, -1), _E61, _E61, (E, 3, 4, 4, 0, -1, 0, 6, 33, -1), (R, 4, 6, 6, 0, -1, 0, 25, 51, -1),
    _E61, (R, 4, 25, 68, 43, -1, 0, 231, 40, -1), (R, 4, 17, 32, 15, -1, 0, 66, 14, -1), (R, 4, 7, 9, 2, -1, 0, 14, 45, -1),
    (S, 4, 25, 50, 18, 49, 0, 142, 52, -1), (R, 4, 8, 12, 4, -1, 0, 41, 25, -1), (E, 2, 2, 2, 0, -1, 0, 6, 29, -1),
    _E75, (R, 4, 14, 14, 0, -1, 0, 32, 26, -1), _E75, (E, 1, 1, 1, 0, -1, 0, 0, 3, -1), (E, 3, 3, 3, 0, -1, 0, 2, 3, -1), _E75,
    _E75, (R, 4, 12, 12, 0, -1, 0, 22, 14, -1), (E, 1, 1, 1, 0, -1, 0, 0, 11, -1), (E, 3, 6, 6, 0, -1, 0, 10, 28, -1),
    (R, 4, 9, 11, 2, -1, 0, 24, 4, -1), (E, 1, 1, 1, 0, -1, 0, 2, 5, -1), (R, 4, 18, 26, 8, -1, 0, 42, 9, -1),
]
# K = 8, at most ten rounds, in the order of BUDGETS
PINNED_BUDGET = [
    (S, 5, 33, 248, 207, 247, 228, 596, 45, 9),
    (S, 5, 33, 252, 217, 251, 138, 661, 45, 20),
    (S, 5, 33, 266, 231, 265, 96, 661, 45, 22),
    (S, 5, 33, 283, 242, 282, 37, 665, 45, 25),
    (R, 10, 73, 749, 676, -1, 54, 1719, 41, -1),
    (R, 10, 73, 771, 698, -1, 65, 1571, 39, 18),
    (S, 8, 57, 589, 531, 588, 35, 1368, 45, 17),
    (S, 6, 31, 62, 30, 61, 52, 88, 26, 3),
    (S, 6, 31, 62, 30, 61, 47, 94, 26, 5),
    (S, 3, 7, 8, 0, 7, 6, 9, 26, 2),
]
PINNED_OUTSIDE8 = (S, 1, 1, 4, 0, 3, 0, 6, 17, -1)
PINNED_OUTSIDE8_INSIDE = (S, 3, 5, 9, 2, 8, 0, 15, 16, 4)  # from the initial state: solved by a goal row inside the grid
# `Seeing Red` at K = 8 after begin and after every round
PINNED_RANGE = [
    (R, 0, 0, 1, 1, -1, 0, 0, 43, 19),
    (R, 1, 1, 15, 14, -1, 0, 22, 44, 24),
    (R, 2, 9, 95, 86, -1, 0, 195, 45, 25),
    (R, 3, 17, 188, 171, -1, 0, 362, 45, 25),
    (R, 4, 25, 271, 246, -1, 0, 531, 45, 25),
    PINNED_LEVEL1["Seeing Red", 8],
]


def _final(run):
    return tuple(C.restated(run).infos[-1])


def test_cases_and_pins_line_up():
    assert set(PINNED_LEVEL1) == {(r.puzzle, r.k) for r in C.LEVEL1_RUNS} and set(PINNED_LIVE) == set(C.LEVEL1)
    assert all(len(PINNED_SHAPES[k]) == len(C.shape_runs(k)) == 52 for k in C.KS) and len(PINNED_SHAPES_COVER) == 52
    assert len(PINNED_BUDGET) == len(C.BUDGET_RUNS) == 10
    assert set(C.ORDERS[0]) == set(C.LEVEL1) and C.ORDERS[1] == C.ORDERS[0][::-1]
    for name, dims in C.LEVEL1.items():
        cp, _ = C.oracles_of(name)
        assert (cp.num_movables, cp.width, cp.height) == dims, name
    sizes = [C.LEVEL1[n][0] for n in C.ORDERS[0]]
    assert sizes == sorted(sizes, reverse=True) and sizes[0] == 8 and sizes[-1] == 3  # the largest N first, then last
    assert sorted(set(sizes)) == [3, 4, 6, 7, 8]
    assert max(d[2] for d in C.LEVEL1.values()) == 16 and C.LEVEL1["Swiss Army Knife"][2] == 16


@pytest.mark.parametrize("run", C.LEVEL1_RUNS, ids=C.run_id)
def test_level1_pinned(run):
    cp, _ = C.oracles_of(run.puzzle)
    got = C.restated(run)
    print(C.run_id(run), "%.1f s" % got.seconds, tuple(got.infos[-1]))
    assert tuple(got.infos[-1]) == PINNED_LEVEL1[run.puzzle, run.k]
    assert got.seconds < 30  # (about 6 s for the longest where the cases were chosen)
    check_store_invariants(cp, got.ref)
    if run.k == C.LIVE_K:
        assert tuple(C.after(run, C.LIVE_ROUNDS)) == PINNED_LIVE[run.puzzle]
    # every key is finite and no budget overruns: the finite buckets at N = 6 .. 8
    assert got.ref.rgd_exceeded == 0 and got.ref.largest_key >= 4
    assert all(i.rounds == min(r, got.infos[-1].rounds) for r, i in enumerate(got.infos))
    assert all(a.states <= b.states for a, b in zip(got.infos, got.infos[1:]))


def test_level1_coverage():
    finals = {(r.puzzle, r.k): C.restated(r) for r in C.LEVEL1_RUNS}
    # each of 6, 7 and 8 movables both solved and still running, with a store that uses every byte of the key
    for name, byte in (("Victory Road", 5), ("Pick A Tool", 5), ("Seeing Red", 6), ("Shape Of You", 7)):
        states = finals[name, 64].ref.states
        assert len(states[0]) == byte + 1 and len({s[byte] for s in states}) > 1, name  # the last movable moves
    assert {finals["Shape Of You", k].ref.status for k in C.KS} == {R, S}
    assert {finals["Seeing Red", k].ref.status for k in C.KS} == {R, S}
    # the board 16 cells high: a movable reaches the last row a movable can stand in, and the search is still running
    cp, _ = C.oracles_of("Swiss Army Knife")
    reached = [max(y + h for (x, y), (w, h) in zip(s, cp.py.sizes)) for s in finals["Swiss Army Knife", 64].ref.states]
    assert cp.height == 16 and max(reached) >= 15 and finals["Swiss Army Knife", 64].ref.status == R
    # the states form stops `Shape Of You`, `Seeing Red`, `Victory Road` and `Swiss Army Knife` while they run
    assert sum(PINNED_LIVE[n][0] == R for n in C.LEVEL1) == 4 and sum(PINNED_LIVE[n][0] == S for n in C.LEVEL1) == 3
    assert C.LIVE_ITEMS % len(C.LEVEL1) != 0 and C.LIVE_ITEMS > 1024  # more items than a device has workgroups


@pytest.mark.parametrize("k", C.KS)
def test_shapes_pinned(k):
    for run, want in zip(C.shape_runs(k), PINNED_SHAPES[k]):
        cp, _ = C.oracles_of(run.puzzle)
        got = C.restated(run)
        assert tuple(got.infos[-1]) == want, C.run_id(run)
        assert got.seconds < 10
        check_store_invariants(cp, got.ref)
        assert C.in_grid(run.puzzle, C.start_of(run)) and got.ref.states[0] == tuple(C.start_of(run))
    if k == C.SHAPE_COVER_K:
        assert [tuple(C.after(run, C.SHAPE_COVER_ROUNDS)) for run in C.shape_runs(k)] == PINNED_SHAPES_COVER


def test_shapes_coverage():
    sizes = []
    for case in C.SHAPES:
        cp, _ = C.oracles_of(case)
        assert (cp.width, cp.height) == (16, 16) and cp.num_movables == case[0]
        sizes.append(cp.num_movables)
    assert sizes == [8, 8, 6, 7]
    runs = C.shape_runs(C.SHAPE_COVER_K)
    listed = [r for r in runs if r.start != 0]
    assert len(runs) == 52 and len(listed) == 48
    assert sum(SS.overlapping(C.oracles_of(r.puzzle)[0], C.start_of(r)) for r in listed) >= 40
    assert max(x for x, _ in C.shape_starts((8, 2))[2]) == 15 and max(y for _, y in C.shape_starts((8, 2))[2]) == 15
    assert max(x for x, _ in C.shape_starts((8, 2))[7]) == 15
    assert any(x == 15 for r in listed for x, _ in C.start_of(r)) and any(y == 15 for r in listed for _, y in C.start_of(r))
    finals = [C.restated(r).infos[-1] for r in runs]
    assert sum(i.status == R and i.states >= 40 for i in finals) >= 10
    assert sum(i.status == E for i in finals) >= 10
    assert sum(i.status == S for i in finals) >= 1
    cover = [C.after(r, C.SHAPE_COVER_ROUNDS) for r in runs]
    assert sum(i.status == R and i.states >= 40 for i in cover) == 9  # (the issue's sketch said ten; see the module's docstring)
    assert tuple(cover[2 * 13 + 10]) == (S, 4, 25, 50, 18, 49, 0, 142, 52, -1)  # (6, 1), the fourth far state
    assert cover[12].states == 62 and cover[13 + 10].states == 65
    assert sum(i.status == E for i in cover) >= 10
    # every key of these puzzles is +inf or NaN, at every K: the queues without a finite bucket at N = 6 .. 8
    for k in C.KS:
        for r in C.shape_runs(k):
            got = C.restated(r)
            assert got.ref.largest_key == -1 and got.ref.rgd_exceeded == 0
    # the largest stores, for the closed set and the rows of 64 parents
    assert max(C.restated(r).infos[-1].states for r in C.shape_runs(64)) == 726
    assert max(C.restated(r).infos[-1].push_rows for r in C.shape_runs(64)) == 2900


def test_starts_outside_their_grid():
    moved = []
    for case in C.SHAPES:
        cp, _ = C.oracles_of(case)
        state = C.outside_start(case)
        assert not C.in_grid(case, state) and all(-128 <= v <= 127 for xy in state for v in xy)
        changed = [j for j, (a, b) in enumerate(zip(state, cp.initial_state)) if tuple(a) != tuple(b)]
        assert changed == [cp.num_movables - 1]  # one movable, the last: field word 2 (N = 6) or 3 (N = 7, 8)
        moved.append(tuple(a - b for a, b in zip(state[changed[0]], cp.initial_state[changed[0]])))
        graphs = C.restated(C.Run(case, 0, 1, C.SHAPE_ROUNDS, None)).ref.rgd.graphs
        ref = PP.PushPlannerRestatement(cp, C.oracles_of(case)[1], batch=1, graphs=graphs)
        with pytest.raises(ValueError, match="outside the grid"):
            ref.begin(state)
    # right and down by the least that leaves the frame (the value still fits a nibble where the movable is wider than a cell), and -1
    assert moved[0][1] == 0 and moved[0][0] > 0 and moved[1][0] == 0 and moved[1][1] > 0
    assert C.outside_start(C.SHAPES[2])[-1][0] == -1 and C.outside_start(C.SHAPES[3])[-1][1] == -1
    assert C.outside_start(C.SHAPES[1])[-1][1] == 15


@pytest.mark.parametrize("run, want", list(zip(C.BUDGET_RUNS, PINNED_BUDGET)), ids=[C.run_id(r) for r in C.BUDGET_RUNS])
def test_budget_pinned(run, want):
    cp, _ = C.oracles_of(run.puzzle)
    got = C.restated(run)
    assert tuple(got.infos[-1]) == want and got.seconds < 10
    check_store_invariants(cp, got.ref)
    assert got.ref.rgd_exceeded > 0


def test_budget_coverage():
    refs = [C.restated(r).ref for r in C.BUDGET_RUNS]
    assert all(ref.rgd_exceeded > 0 for ref in refs)
    # finite and NaN keys in one queue: a finite key was pushed and a budget overran, and entries of both kinds are still open
    mixed = [ref for ref in refs if ref.largest_key >= 0 and ref.rgd_exceeded > 0]
    assert len(mixed) >= 9
    assert sum(any(b[0] == 0 for b in ref.buckets) and any(b[0] == 2 for b in ref.buckets) for ref in mixed) >= 5
    assert refs[4].largest_key == -1 and refs[4].status == R  # `Shape Of You` with one call: no finite key at all
    assert {ref.status for ref in refs} == {R, S}
    assert [C.oracles_of(r.puzzle)[0].num_movables for r in C.BUDGET_RUNS] == [7, 7, 7, 7, 8, 8, 8, 6, 6, 6]


def test_goal_state_outside_its_grid_through_movable_7():
    cp, _ = C.oracles_of("outside8")
    assert cp.py.names == C.OUTSIDE8_ORDER and cp.num_movables == 8 and (cp.width, cp.height) == (8, 6)
    ref = C.restated(C.OUTSIDE8_RUN).ref
    assert tuple(ref.info()) == PINNED_OUTSIDE8
    assert ref.states[-1] == ((4, 3), (5, 3), (1, 1), (2, 1), (3, 1), (4, 1), (5, 1), (6, 3)) and ref.canons[-1] == (0, 0)
    assert not C.in_grid("outside8", ref.states[-1]) and all(C.in_grid("outside8", s) for s in ref.states[:-1])
    assert [j for j, (a, b) in enumerate(zip(ref.states[-1], ref.states[0])) if a != b] == [0, 1, 7]
    x, _ = ref.states[-1][7]
    assert x + cp.py.sizes[7][0] == cp.width + 1  # movable 7, the high half of the fourth field word, is the one outside
    assert C.pushes_of(ref) == [((3, 3), 1)] and check_store_invariants(cp, ref) == 1
    inside = C.restated(C.OUTSIDE8_INSIDE_RUN).ref
    assert tuple(inside.info()) == PINNED_OUTSIDE8_INSIDE and all(C.in_grid("outside8", s) for s in inside.states)
    assert inside.canons[-1] != (0, 0) and check_store_invariants(cp, inside) == 3


def test_plans_for_push_cap():
    """The two items of the ``push_cap`` test: plans of more than one push and of different lengths, N = 8 and N = 3."""
    long_, short = (C.restated(C.Run(n, None, 64, C.ROUNDS, None)).ref for n in ("Shape Of You", "Two Goals"))
    assert long_.status == short.status == S
    assert (len(C.pushes_of(long_)), len(C.pushes_of(short))) == (8, 4)
    assert len(long_.states[0]) == 8 and len(short.states[0]) == 3


def test_range_run():
    got = C.restated(C.RANGE_RUN)
    assert [tuple(i) for i in got.infos] == PINNED_RANGE
    assert got.ref.largest_key == C.RANGE_SHORT == 25 and min(C.RANGE_SAME) == 26
    first = min(r for r, i in enumerate(got.infos) if i.largest_key >= C.RANGE_SHORT)
    assert first == 2 < got.ref.rounds
    # the +inf bucket, number cost_range, on either side of the first word boundary of each level of the bucket bitmap
    assert [c >> 6 for c in C.RANGE_SAME] == [0, 1, 1, 64, 64] and [c >> 12 for c in C.RANGE_SAME] == [0, 0, 0, 1, 1]


def test_time_limit_items():
    """Every puzzle of part 1 runs at least one round at K = 8 and none is solved at its start: a time limit that ends the
    searches after fewer rounds than the unlimited run shows in the round count."""
    for name in C.LEVEL1:
        got = C.restated(C.Run(name, None, 8, C.ROUNDS, None))
        assert got.infos[0].status == R and got.infos[-1].rounds >= 3

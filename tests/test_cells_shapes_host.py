"""The inputs of tests/test_gpu_cells_shapes.py pinned on the CPU before a device sees them: on every listed state of the random-
shape puzzles of tests/replay_cases.py (the six cases of tests/shape_states.py and the three-goal variants) the host definition
``PushWorldPuzzle.cells`` equals the restatement of tests/cells_restatement.py, built from the oracle's sets alone; and the
lists do hold what the kernel has to be careful with -- cells hidden under a higher movable, three movables on one cell, a hidden
cell in the second trip of the lane loop, goal shapes that run into the border wall."""
import pytest

import cells_restatement as CR
import replay_cases as RC
import shape_states as SS
from pushworld_amd.puzzle import PushWorldPuzzle


def _odd(cp):
    return (cp.height + 3, cp.width + 5)


@pytest.mark.parametrize("key", RC.KEYS)
def test_host_definition_equals_restatement(key):
    cp = RC.puzzle(key)
    pz = PushWorldPuzzle(text=RC.text(key))
    assert pz.dimensions == (cp.width, cp.height) and pz.initial_state == cp.initial_state
    assert len(pz.goal_state) == cp.num_goals == (3 if RC.is_three(key) else 1)
    for frame in (None, _odd(cp)):
        for kind, s in RC.states(key):
            assert (pz.cells(s, frame=frame) == CR.cells(cp, s, frame)).all(), (key, frame, kind, s)
    odd = CR.cells(cp, cp.initial_state, _odd(cp))
    assert (odd[:, 1:1 + cp.height, 2:2 + cp.width] == CR.cells(cp, cp.initial_state)).all()  # margins 1 | 2 and 2 | 3
    assert odd.sum() == CR.cells(cp, cp.initial_state).sum()


@pytest.mark.parametrize("key", RC.KEYS)
def test_every_case_hides_cells(key):
    cp = RC.puzzle(key)
    hiding = [s for _, s in RC.states(key) if CR.hidden(cp, s)]
    assert len(hiding) >= 6, len(hiding)
    for s in hiding:  # the hidden cell shows the higher index, in the restatement as in the definition of DESIGN K10
        k, index, top = CR.hidden(cp, s)[0]
        w = cp.py.sizes[k][0]
        x, y = s[k][0] + index % w, s[k][1] + index // w
        assert k < top and CR.cells(cp, s)[1, y, x] == 1 + top


def test_coverage_over_all_cases():
    depth, late, clipped = 0, 0, []
    for key in RC.KEYS:
        cp = RC.puzzle(key)
        for _, s in RC.states(key):
            depth = max(depth, CR.cover_depth(cp, s))
            late += any(index >= 64 for _, index, _ in CR.hidden(cp, s))
        if CR.goal_clipped(cp):
            clipped.append(key)
    assert depth >= 3  # a cell covered by three movables
    assert late >= 1  # a hidden cell beyond the first 64 of its bounding box: the second trip of the kernel's lane loop
    assert len(clipped) >= 2, clipped  # a goal shape (plane 2) that reaches into the border wall or past the frame


def test_states_are_the_overlapping_ones():
    for key in RC.KEYS:
        cp = RC.puzzle(key)
        listed = RC.states(key)
        assert 2 * sum(SS.overlapping(cp, s) for _, s in listed) >= len(listed), key

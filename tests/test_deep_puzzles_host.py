"""The deep and large puzzles of tests/deep_puzzles.py against the host reference (the reverse breadth-first search of
tests/test_gpu_solution_table.py::HostTable over the compiled C oracle): the recorded figures, so that the inputs of the GPU
tests cannot drift.  No GPU."""
import numpy as np
import pytest

import deep_puzzles
from pushworld_amd.puzzle import PushWorldPuzzle


@pytest.mark.parametrize("name", list(deep_puzzles.EXPECT))
def test_recorded_figures(name):
    """(states, goal states, dead ends, largest finite cost, cost of the start) of every puzzle but the million-row room."""
    assert deep_puzzles.host_table(name).summary == deep_puzzles.EXPECT[name]


def test_the_scan_boundaries():
    """The two started serpentines give cost_start tables of exactly 256 and 257 words, the largest board 1952."""
    words = {name: deep_puzzles.EXPECT[name][3] + 3 for name in deep_puzzles.EXPECT}
    assert words[deep_puzzles.M256[0]] == 256 and words[deep_puzzles.M257[0]] == 257
    assert words["serpentine 62x61"] == 1953 and words["serpentine 62x61 overshoot"] == 1952
    assert [deep_puzzles.EXPECT["corridor %d" % L][3] for L in deep_puzzles.CORRIDORS] == [15, 16, 17, 31, 32, 33]


def test_shapes():
    """The boards are the sizes the tests rely on: 16 x 16 with the border for the batch builder, 64 x 63 the largest; the
    pockets puzzle has 17 movables; the three-box room is the 6 x 6 room."""
    def dims(text):
        pz = PushWorldPuzzle(text=text)
        return tuple(pz.dimensions), pz.num_movables

    assert dims(deep_puzzles.serpentine(14, 14)) == ((16, 16), 2)
    assert dims(deep_puzzles.serpentine(14, 13, True)) == ((16, 15), 2)
    assert dims(deep_puzzles.serpentine(62, 61, True)) == ((64, 63), 2)
    assert dims(deep_puzzles.pockets())[1] == 2 + deep_puzzles.POCKETS_EXTRA == 17
    assert dims(deep_puzzles.room3()) == ((8, 8), 4)
    assert dims(deep_puzzles.corridor(35)) == ((37, 3), 2)


def test_every_bucket_of_a_serpentine_is_small_until_the_overshoot():
    """Without dead ends a path puzzle has at most three rows per cost; with overshoot the dead-end bucket is a third of the
    table, after a run of 1950 small buckets."""
    t = deep_puzzles.host_table("serpentine 62x61 overshoot")
    finite = t.cost[t.cost != 0xFFFF]
    assert np.bincount(finite).max() == 1950 and np.bincount(finite)[1:].max() <= 3 and (t.cost == 0xFFFF).sum() == 1951

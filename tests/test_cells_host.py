"""Host side of the cell-grid observations: the numpy definition ``PushWorldPuzzle.cells`` against
hand-written arrays, against the reference's own renders, and its invariants over every Level 1-4 puzzle; the argument
checks of the C calls that return before any launch and of ``VecPushWorld(observation=...)``."""
import ctypes
import glob
import os

import numpy as np
import pytest

from pushworld_amd import _capi
from pushworld_amd.puzzle import Colors, PushWorldPuzzle
from pushworld_amd.vec_env import VecPushWorld

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_PY = os.path.join(ROOT, "tests", "puzzles", "ref_python")
PUZZLES = os.path.join(ROOT, "pushworld_amd", "data", "puzzles")
P = ctypes.c_void_p(4096)  # stand-in for a device pointer: every check below returns before anything is read through it


def _grid(text):
    return np.array([[int(c) for c in row.split()] for row in text.strip().splitlines()], np.uint8)


def _border(h, w, inner=1):
    g = np.full((h, w), 3, np.uint8)
    g[1:-1, 1:-1] = inner
    return g


def test_multiple_goals_both_orders():
    # A at (5, 2), M1 at (3, 2) with goal G1 at (2, 2), M2 at (7, 2) with goal G2 at (8, 2) (border walls included)
    for order, ids in (("python", {"A": 1, "M2": 2, "M1": 3}), ("cpp", {"A": 1, "M1": 2, "M2": 3})):
        pz = PushWorldPuzzle(os.path.join(REF_PY, "multiple_goals.pwp"), order=order)
        c = pz.cells(pz.initial_state)
        assert c.shape == (3, 5, 11) and c.dtype == np.uint8
        assert (c[0] == _border(5, 11)).all()
        occ = np.zeros((5, 11), np.uint8)
        occ[2, 5], occ[2, 3], occ[2, 7] = ids["A"], ids["M1"], ids["M2"]
        assert (c[1] == occ).all(), order
        goal = np.zeros((5, 11), np.uint8)
        goal[2, 2], goal[2, 8] = ids["M1"], ids["M2"]
        assert (c[2] == goal).all(), order


FILE_PARSING_STATIC = """
3 3 3 3 3 3 3 3 3 3 3 3
3 1 1 1 1 1 1 1 1 3 3 3
3 1 1 1 1 1 1 1 1 3 3 3
3 1 1 1 1 1 1 1 1 3 3 3
3 1 1 1 1 1 1 1 1 3 3 3
3 1 1 1 1 1 1 1 1 3 3 3
3 1 1 1 1 1 1 1 1 1 1 3
3 1 1 1 1 1 1 1 1 1 1 3
3 1 1 1 1 1 1 1 2 1 1 3
3 1 1 1 1 1 1 1 2 1 1 3
3 1 1 1 1 1 1 1 1 1 1 3
3 1 1 1 1 1 1 1 1 3 3 3
3 1 1 1 1 1 1 1 1 3 3 3
3 1 1 1 1 1 1 1 1 3 3 3
3 1 1 1 1 1 1 1 1 3 3 3
3 1 1 1 1 1 1 1 1 3 3 3
3 1 1 1 1 1 1 1 1 3 3 3
3 3 3 3 3 3 3 3 3 3 3 3
"""

# objects by name: A (agent), M0 (two diagonal cells), M1, M2 (a ring around M3), M3, M4 (diagonal); goals G1, G4
FILE_PARSING_OCC = """
0 0 0 0 0 M0 0 0 0 0 0 0
0 0 0 0 M0 0 0 0 0 0 0 0
0 M1 0 0 0 0 0 0 0 0 0 0
0 0 0 0 0 0 0 0 0 0 0 0
0 0 0 0 0 0 0 0 0 0 0 0
0 0 0 0 0 0 0 0 0 0 0 0
0 0 M2 M2 M2 0 0 0 0 0 0 0
0 0 M2 M3 M2 0 0 0 0 0 0 0
0 0 M2 M2 M2 0 0 0 0 0 0 0
0 0 0 0 0 0 0 0 0 0 0 0
0 0 0 0 0 0 0 0 0 0 0 0
0 A A A 0 0 0 0 0 0 0 0
0 0 0 A 0 0 0 0 0 0 0 0
0 0 0 A 0 0 M4 0 0 0 0 0
0 0 0 0 0 0 0 M4 0 0 0 0
0 0 0 0 0 0 0 0 0 0 0 0
"""

FILE_PARSING_GOAL = """
0 0 0 0 0 0 0 0 0 0 0 0
0 0 0 0 0 0 0 0 0 0 0 0
0 0 0 M1 0 0 0 0 0 0 0 0
0 0 0 0 0 0 M4 0 0 0 0 0
0 0 0 0 0 0 0 M4 0 0 0 0
"""


def _named(text, ids, h, w, row0):
    out = np.zeros((h, w), np.uint8)
    for y, row in enumerate(text.strip().splitlines()):
        for x, tok in enumerate(row.split()):
            if tok != "0":
                out[row0 + y, x] = ids[tok]
    return out


def test_file_parsing_both_orders():
    # python order: agent, goal objects descending (M4, M1), the rest in file order (M0, M2, M3); cpp: M1, M4, M0, M2, M3
    for order, names in (("python", ["A", "M4", "M1", "M0", "M2", "M3"]), ("cpp", ["A", "M1", "M4", "M0", "M2", "M3"])):
        pz = PushWorldPuzzle(os.path.join(REF_PY, "file_parsing.pwp"), order=order)
        ids = {n: k + 1 for k, n in enumerate(names)}
        c = pz.cells(pz.initial_state)
        assert c.shape == (3, 18, 12)
        assert (c[0] == _grid(FILE_PARSING_STATIC)).all()
        assert (c[1] == _named(FILE_PARSING_OCC, ids, 18, 12, 1)).all(), order
        assert (c[2] == _named(FILE_PARSING_GOAL, ids, 18, 12, 2)).all(), order
        # the goal codes are the plane-1 codes of the objects that belong there
        assert set(np.unique(c[2])) == {0, ids["M1"], ids["M4"]}


def test_frame_offsets_and_errors():
    pz = PushWorldPuzzle(os.path.join(REF_PY, "multiple_goals.pwp"))
    own = pz.cells(pz.initial_state)
    big = pz.cells(pz.initial_state, frame=(10, 16))
    oy, ox = (10 - 5) // 2, (16 - 11) // 2
    assert (big[:, oy : oy + 5, ox : ox + 11] == own).all()
    big[:, oy : oy + 5, ox : ox + 11] = 0
    assert not big.any()
    with pytest.raises(ValueError, match="smaller"):
        pz.cells(pz.initial_state, frame=(4, 11))
    with pytest.raises(ValueError, match="movables"):
        pz.cells(pz.initial_state[:2])
    # cells outside the frame are dropped, the largest index wins where objects overlap
    c = pz.cells(((-3, 2), (5, 2), (5, 2)))
    assert c[1, 2, 5] == 3 and (c[1] > 0).sum() == 1


_FILL = {Colors.WALL: ("static", 3), Colors.AGENT_WALL: ("static", 2), (255, 255, 255): ("static", 1),
         Colors.AGENT: ("agent", None), Colors.GOAL_OBJECT: ("goalobj", None), Colors.MOVABLE: ("movable", None)}


def test_against_reference_renders(golden):
    keys = [k for k in golden.images.files if "|init|" in k]
    assert len(keys) >= 12
    for key in keys:
        pkey, _, ppc, _bw = key.split("|")
        ppc = int(ppc)
        pz = PushWorldPuzzle(text=golden.text(pkey))
        img = golden.images[key]
        W, H = pz.dimensions
        assert img.shape == (H * ppc, W * ppc, 3)
        c = pz.cells(pz.initial_state)
        G = len(pz.goal_state)
        for y in range(H):
            for x in range(W):
                kind, code = _FILL[tuple(int(v) for v in img[y * ppc + ppc // 2, x * ppc + ppc // 2])]
                occ = int(c[1, y, x])
                if kind == "static":
                    assert occ == 0 and c[0, y, x] == code, (key, x, y)
                elif kind == "agent":
                    assert occ == 1, (key, x, y)
                elif kind == "goalobj":
                    assert 2 <= occ <= G + 1, (key, x, y)
                else:
                    assert occ > G + 1, (key, x, y)


def _level_puzzles():
    for lvl in ("level1", "level2", "level3", "level4"):
        yield from sorted(glob.glob(os.path.join(PUZZLES, lvl, "*.pwp")))


@pytest.mark.parametrize("order", ["python", "cpp"])
def test_invariants_every_level_puzzle(order):
    paths = list(_level_puzzles())
    assert len(paths) > 100
    for path in paths:
        pz = PushWorldPuzzle(path, order=order)
        W, H = pz.dimensions
        frame = (H + 3, W + 4)
        c = pz.cells(pz.initial_state, frame=frame)
        oy, ox = 1, 2
        inner = np.zeros(frame, bool)
        inner[oy : oy + H, ox : ox + W] = True
        assert not c[:, ~inner].any(), path  # padding: zero in every plane
        assert (c[0][inner] > 0).all()
        assert (c[0] == 3).sum() == len(pz.wall_positions)
        assert (c[0] == 2).sum() == len(pz.agent_wall_positions - pz.wall_positions)
        for k, m in enumerate(pz.movable_objects):  # initial states do not overlap: every shape cell is reported
            assert (c[1] == k + 1).sum() == len(m.cells), (path, k)
        for g in range(len(pz.goal_state)):
            assert (c[2] == g + 2).sum() == len(pz.movable_objects[g + 1].cells), (path, g)
        assert c[2].max() <= len(pz.goal_state) + 1


def test_c_calls_without_an_engine():
    lib = _capi.lib
    h = ctypes.c_int()
    assert lib.pw_engine_cells_shape(None, ctypes.byref(h), ctypes.byref(h)) == _capi.PW_EINVAL
    assert "null engine" in _capi.last_error()
    assert lib.pw_render_cells(None, P, P, P, 4096, 8, None) == _capi.PW_EINVAL
    assert "null engine" in _capi.last_error()
    assert lib.pw_step_cells(None, P, P, P, P, P, P, P, P, P, 4096, 8, 0, None) == _capi.PW_EINVAL
    assert "null engine" in _capi.last_error()
    assert _capi.OPTIONS["cells_base_bytes"] == 51


def test_vec_observation_arguments():
    path = os.path.join(REF_PY, "multiple_goals.pwp")
    with pytest.raises(ValueError, match="cells"):
        VecPushWorld([path], 4, observation="grid")
    for kw in (dict(incremental=True), dict(tune=True), dict(tune_allocations=4)):
        with pytest.raises(ValueError, match="observation='cells'"):
            VecPushWorld([path], 4, observation="cells", **kw)

"""The cell-grid observation restated from the oracle's own sets, in plain Python + numpy: what
``pw_render_cells`` / ``pw_step_cells`` and the host definition ``PushWorldPuzzle.cells`` are compared with on random shapes,
overlapping states and states at the edge of the engine's domain.  A helper, not a test; nothing of the package is imported.

``cells(cp, state, frame)`` for an ``oracle.c_oracle.COraclePuzzle`` reads only ``cp.py.shapes``, ``wall_cells``,
``agent_wall_cells``, ``goal_state``, ``cp.width`` and ``cp.height``, and follows K10's words:
  frame    (Hc, Wc) cells, the puzzle at row offset (Hc - H) // 2 and column offset (Wc - W) // 2
  plane 0  0 outside the puzzle, 1 floor, 2 agent wall, 3 wall; a wall is never an agent wall
  plane 1  1 + k on the cells movable k covers, k ascending, so the largest k wins where movables overlap
  plane 2  1 + k on movable k's shape at the goal position of k (goal g belongs to movable g + 1), the largest k wins
  every cell outside the frame is dropped"""
import numpy as np


def offsets(cp, frame=None):
    """(Hc, Wc, oy, ox) of the frame (default: the puzzle's own H x W)."""
    hc, wc = (cp.height, cp.width) if frame is None else (int(frame[0]), int(frame[1]))
    assert hc >= cp.height and wc >= cp.width, (frame, cp.height, cp.width)
    return hc, wc, (hc - cp.height) // 2, (wc - cp.width) // 2


def covered(cp, k, origin):
    """The puzzle-frame cells (x, y) of movable k with its bounding box at `origin`."""
    return [(int(origin[0]) + cx, int(origin[1]) + cy) for cx, cy in cp.py.shapes[k]]


def cells(cp, state, frame=None):
    hc, wc, oy, ox = offsets(cp, frame)
    out = np.zeros((3, hc, wc), np.uint8)

    def put(plane, x, y, value):
        fx, fy = x + ox, y + oy
        if 0 <= fx < wc and 0 <= fy < hc:
            out[plane, fy, fx] = value

    for y in range(cp.height):
        for x in range(cp.width):
            kind = 3 if (x, y) in cp.py.wall_cells else (2 if (x, y) in cp.py.agent_wall_cells else 1)
            put(0, x, y, kind)
    assert len(state) == cp.num_movables
    for k in range(cp.num_movables):
        for x, y in covered(cp, k, state[k]):
            put(1, x, y, 1 + k)
    for g, origin in enumerate(cp.py.goal_state):
        for x, y in covered(cp, g + 1, origin):
            put(2, x, y, 1 + (g + 1))
    return out


def hidden(cp, state):
    """[(k, index, top)]: shape cells of movable k lying under a higher-indexed movable `top` (the highest); `index` is the
    cell's row-major index inside k's bounding box, the lane-loop index of the kernel."""
    owner = {}
    for k in range(cp.num_movables):
        for c in covered(cp, k, state[k]):
            owner.setdefault(c, []).append(k)
    out = []
    for (x, y), ks in owner.items():
        for k in ks[:-1]:
            w = cp.py.sizes[k][0]
            out.append((k, (y - state[k][1]) * w + (x - state[k][0]), ks[-1]))
    return out


def cover_depth(cp, state):
    """The largest number of movables that share one cell."""
    count = {}
    for k in range(cp.num_movables):
        for c in covered(cp, k, state[k]):
            count[c] = count.get(c, 0) + 1
    return max(count.values())


def goal_clipped(cp, frame=None):
    """True when some goal shape of plane 2 reaches into the border wall or past the frame."""
    hc, wc, oy, ox = offsets(cp, frame)
    for g, origin in enumerate(cp.py.goal_state):
        for x, y in covered(cp, g + 1, origin):
            if not (0 <= x + ox < wc and 0 <= y + oy < hc):
                return True
            if x in (0, cp.width - 1) or y in (0, cp.height - 1):
                return True
    return False

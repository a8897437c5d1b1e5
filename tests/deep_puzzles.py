"""Tiny hand-built puzzles whose exhausted spaces are DEEP (a largest cost-to-go in the hundreds and thousands) or LARGE (tens of
thousands to millions of rows): inputs of the cost-to-go table tests.  The figures in EXPECT were
computed with the reverse breadth-first search of tests/test_gpu_solution_table.py::HostTable over the compiled C oracle;
tests/test_deep_puzzles_host.py pins them without a GPU.

A puzzle whose cells form ONE path of P cells that ends in a box, a free cell and the goal (`M0 . G0`) has 3 P - 6 states: the
box on one of its three cells and the agent anywhere behind it.  P - 1 of them are goal states, none is a dead end, and the
largest cost is the start's: P - 4 steps up to the box and two pushes, P - 2.  With the goal and the free cell swapped
(`M0 G0 .`) the box can be pushed past its goal: the P - 1 states with the box on the last cell are dead ends, P - 2 are goal
states, and the largest cost is P - 3."""


def _grid(rows):
    return "\n".join(" ".join(r) for r in rows) + "\n"


def serpentine_path(W, H):
    """The cells (x, y) of the path through a W x H interior: the even rows, left to right and right to left in turn, joined
    at alternating ends by one cell of the odd row between them."""
    path = []
    for y in range(0, H, 2):
        xs = range(W) if (y // 2) % 2 == 0 else range(W - 1, -1, -1)
        path += [(x, y) for x in xs]
        if y + 2 < H:
            path.append((path[-1][0], y + 1))
    return path


def serpentine(W, H, overshoot=False, start=0):
    """A W x H interior that is all wall but the serpentine path.  The path begins at its `start`-th cell, where the agent
    stands (the cells before it stay wall: every cell less makes the largest cost one less), and ends in `M0 . G0`, or in
    `M0 G0 .` with `overshoot`."""
    path = serpentine_path(W, H)
    assert 0 <= start <= len(path) - 4
    g = [["W"] * W for _ in range(H)]
    for x, y in path[start:]:
        g[y][x] = "."
    tail = ("M0", "G0", ".") if overshoot else ("M0", ".", "G0")
    for (x, y), cell in zip(path[-3:], tail):
        g[y][x] = cell
    x, y = path[start]
    g[y][x] = "A"
    return _grid(g)


def serpentine_with_max_cost(W, H, max_cost):
    """serpentine(W, H) without overshoot, started so far along the path that the largest cost is exactly `max_cost`."""
    return serpentine(W, H, start=len(serpentine_path(W, H)) - 2 - max_cost)


def corridor(L):
    """One row of L cells: the agent, L - 4 free cells, then `M0 . G0`.  The largest cost is L - 2."""
    assert L >= 4
    return _grid([["A"] + ["."] * (L - 4) + ["M0", ".", "G0"]])


def big():
    """The open 6 x 6 room with two boxes (tests/test_gpu_table_sample.py `big`)."""
    g = [["."] * 6 for _ in range(6)]
    g[0][0], g[2][2], g[3][3], g[5][5] = "A", "M0", "M1", "G0"
    return _grid(g)


def room3():
    """`big` with a third box: the exhausted space has more than 2^20 states."""
    g = [["."] * 6 for _ in range(6)]
    g[0][0], g[2][2], g[3][3], g[1][4], g[5][5] = "A", "M0", "M1", "M2", "G0"
    return _grid(g)


POCKETS_EXTRA = 15


def pockets(extra=POCKETS_EXTRA):
    """corridor(7) plus `extra` more movables, each sealed alone in a single cell between walls: 2 + extra movables, and the
    state space of the corridor (the sealed ones never move)."""
    width = max(7, 2 * extra - 1)
    top = ["A", ".", ".", ".", "M0", ".", "G0"] + ["W"] * (width - 7)
    cells = ["W"] * width
    for k in range(extra):
        cells[2 * k] = "M%d" % (k + 1)
    return _grid([top, ["W"] * width, cells])


M256 = ("serpentine 30x29 max 253", lambda: serpentine_with_max_cost(30, 29, 253))   # m = max_cost + 3 = 256
M257 = ("serpentine 30x29 max 254", lambda: serpentine_with_max_cost(30, 29, 254))   # m = 257
CORRIDORS = [17, 18, 19, 33, 34, 35]

# name -> (the puzzle's text, (states, goal states, dead ends, largest finite cost, cost of the start))
_CASES = [
    ("serpentine 14x14", lambda: serpentine(14, 14), (306, 103, 0, 102, 102)),
    ("serpentine 30x29", lambda: serpentine(30, 29), (1386, 463, 0, 462, 462)),
    ("serpentine 62x17", lambda: serpentine(62, 17), (1692, 565, 0, 564, 564)),
    ("serpentine 62x61", lambda: serpentine(62, 61), (5850, 1951, 0, 1950, 1950)),
    ("serpentine 14x13 overshoot", lambda: serpentine(14, 13, True), (306, 102, 103, 101, 101)),
    ("serpentine 30x29 overshoot", lambda: serpentine(30, 29, True), (1386, 462, 463, 461, 461)),
    ("serpentine 62x61 overshoot", lambda: serpentine(62, 61, True), (5850, 1950, 1951, 1949, 1949)),
    # the path of 255 / 256 cells: 3 P - 6 states, P - 1 goal states, largest cost P - 2 (the host reference agrees)
    M256 + ((759, 254, 0, 253, 253),),
    M257 + ((762, 255, 0, 254, 254),),
    ("big", big, (42832, 1190, 14444, 19, 11)),
    ("pockets", pockets, (15, 6, 0, 5, 5)),
] + [("corridor %d" % L, (lambda L=L: corridor(L)), (3 * (L - 2), L - 1, 0, L - 2, L - 2)) for L in CORRIDORS]

TEXT = {name: make for name, make, _ in _CASES}
EXPECT = {name: want for name, _, want in _CASES}

_HOST = {}


def text(name):
    return TEXT[name]()


def host_table(name):
    """The reference table of a case (test_gpu_solution_table.HostTable); computed once per session and never changed."""
    from test_gpu_solution_table import HostTable

    if name not in _HOST:
        _HOST[name] = HostTable(text(name))
    return _HOST[name]


# one set for the batch builder: both 14-wide serpentines (16 x 16 with the border, its limit), the 42 832 rows of `big`, and
# three of the tiny cases of tests/test_gpu_solution_table.py
BATCH_DEEP = ["serpentine 14x14", "serpentine 14x13 overshoot", "big"]
BATCH_TINY = ["pytest:trivial.pwp", "pytest:trivial_tool.pwp", "pytest:transitive_pushing.pwp"]
BATCH_CAP = 50000  # max_states_each: above the 42 832 states of `big`


def batch_set(golden):
    """(names, texts, host tables) of the set above, in set order."""
    import test_gpu_solution_table as k12

    names = BATCH_DEEP + BATCH_TINY
    texts = [text(k) for k in BATCH_DEEP] + [golden.text(k) for k in BATCH_TINY]
    hosts = [host_table(k) for k in BATCH_DEEP] + [k12.host_table(golden, k) for k in BATCH_TINY]
    return names, texts, hosts

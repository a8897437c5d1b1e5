"""Seeded random puzzles for the expansion tests (a helper module, imported by test files that put tests/ on sys.path)."""


def many_movables_text(rng, n_mov, cols=20, rows=14, cells=(1, 3), goal_p=0.35, big=(), x_min=0):
    """A puzzle with n_mov movables (agent included) of ``cells`` (lo, hi) cells each, goals for a fraction ``goal_p`` of them,
    some walls.  ``big``: (w, h) bounding boxes of L-shaped movables (a row of w cells over a column of h) placed first, as
    movables 1, 2, ... -- what makes the pair tables large without filling the grid; ``x_min``: the other movables start at
    columns from there on (movables near the right edge of a wide grid)."""
    grid = [[[] for _ in range(cols)] for _ in range(rows)]

    def blob(n):
        cells_ = [(int(rng.integers(x_min, cols)), int(rng.integers(0, rows)))]
        for _ in range(n - 1):
            bx, by = cells_[int(rng.integers(0, len(cells_)))]
            dx, dy = [(1, 0), (-1, 0), (0, 1), (0, -1)][int(rng.integers(0, 4))]
            if 0 <= bx + dx < cols and 0 <= by + dy < rows and (bx + dx, by + dy) not in cells_:
                cells_.append((bx + dx, by + dy))
        return cells_

    for _ in range(int(rng.integers(4, 14))):
        grid[int(rng.integers(0, rows))][int(rng.integers(0, cols))].append("W")
    names = ["A"] + [f"M{k}" for k in range(1, n_mov)]
    for i, name in enumerate(names):
        while True:
            if 1 <= i <= len(big):
                w, h = big[i - 1]
                x0, y0 = int(rng.integers(0, cols - w + 1)), int(rng.integers(0, rows - h + 1))
                shape = [(x0 + dx, y0) for dx in range(w)] + [(x0, y0 + dy) for dy in range(1, h)]
            else:
                shape = blob(int(rng.integers(cells[0], cells[1] + 1)))
            if all(not grid[y][x] for x, y in shape):
                for x, y in shape:
                    grid[y][x].append(name)
                break
    for k in range(1, n_mov):
        if rng.random() < goal_p:
            x, y = int(rng.integers(0, cols)), int(rng.integers(0, rows))
            if not any(t.startswith("G") or t == "W" for t in grid[y][x]):
                grid[y][x].append(f"G{k}")
    if not any(t.startswith("G") for row in grid for c in row for t in c):
        grid[0][0] = [t for t in grid[0][0] if t != "W"] + ["G1"]
    return "\n".join(" ".join("+".join(c) if c else "." for c in row) for row in grid) + "\n"

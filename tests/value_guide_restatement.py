"""``pw_guide_step`` (include/pushworld_amd.h) restated in plain numpy and Python floats: one function, one
environment at a time, nothing shared with the library.  The lookup is a callable ``look(i, p, row) -> (cost, acts)``:
``HostLookup`` answers it from ``HostTable``s (tests/test_gpu_solution_batch.py: a forward plus reverse breadth-first search
with the C oracle), ``ArrayLookup`` from arrays that some query wrote (the applied form)."""
import numpy as np

AUTORESET, END_DEAD, REFRESH = 1, 2, 4
GUIDED, OPTIMAL, DEAD_ENTERED, UNKNOWN = 0, 1, 2, 3
INF = 0xFFFF


class HostLookup:
    """``tables``: {puzzle id: (HostTable, W, H)}.  The answer for (p, row) is the host table's cost (-1 at a dead end) and
    action bits of the state made of the row's first N movables; -2 / 0 for a puzzle without a table, an id outside the set,
    a coordinate outside 0 .. 15 or outside the W x H grid, N beyond the row, and a state the start does not reach."""

    def __init__(self, tables):
        self.tables = dict(tables)

    def __call__(self, i, p, row):
        if p not in self.tables:
            return -2, 0
        host, W, H = self.tables[p]
        N = len(host.states[0])
        if N > len(row):
            return -2, 0
        s = tuple((int(x), int(y)) for x, y in row[:N])
        if any(not (0 <= x < min(W, 16) and 0 <= y < min(H, 16)) for x, y in s):
            return -2, 0
        j = host.index.get(s)
        if j is None:
            return -2, 0
        c = int(host.cost[j])
        return (-1 if c == INF else c), int(host.acts[j])


class ArrayLookup:
    """The applied form: ``(cost_in[i], acts_in[i] or 0)``."""

    def __init__(self, cost_in, acts_in=None):
        self.cost_in, self.acts_in = np.asarray(cost_in), None if acts_in is None else np.asarray(acts_in)

    def __call__(self, i, p, row):
        return int(self.cost_in[i]), 0 if self.acts_in is None else int(self.acts_in[i])


def guide_step(look, puzzle_id, pos, reward, terminated, truncated, cost, acts, seen, dead, dead_cost, gamma, scale, flags,
               counts=None, mask=None, shaped=None):
    """One ``pw_guide_step`` call.  Nothing given is changed; returns a dict of new arrays ``cost``, ``acts``, ``seen``,
    ``dead``, ``truncated``, ``shaped`` (float64; the given ``shaped`` where nothing is written, zeros without one), ``counts``
    (int64 [P, 4]) and the ints ``ended`` (what ``episodes_ended`` of ``pw_counters`` advances by) and, per branch of the
    rule, how many environments took it (``branches``)."""
    P = len(dead_cost)
    n = len(puzzle_id)
    out = dict(cost=np.array(cost, dtype=np.int32), acts=np.array(acts, dtype=np.uint8), seen=np.array(seen, dtype=np.uint8),
               dead=np.array(dead, dtype=np.uint8), truncated=np.array(truncated, dtype=np.uint8),
               shaped=np.zeros(n, dtype=np.float64) if shaped is None else np.array(shaped, dtype=np.float64),
               counts=np.zeros((P, 4), dtype=np.int64) if counts is None else np.array(counts, dtype=np.int64), ended=0)
    br = dict(masked=0, refresh=0, fresh=0, refused=0, cut=0, guided=0, optimal=0, dead_entered=0, unknown=0, shaped_nonzero=0)
    gamma, scale = float(gamma), float(scale)
    for i in range(n):
        if mask is not None and mask[i] == 0:
            br["masked"] += 1
            continue
        p = int(puzzle_id[i])
        c, a = look(i, p, pos[i])
        t, u = int(terminated[i]), int(truncated[i])
        if flags & REFRESH:
            br["refresh"] += 1
            out["cost"][i], out["acts"][i], out["dead"][i] = c, a, int(c == -1)
            out["seen"][i] = int((t | u) != 0)
            continue
        fresh = bool(flags & AUTORESET) and seen[i] != 0
        refused = t == 0xFF
        c_prev = int(cost[i])
        br["fresh"] += fresh
        br["refused"] += refused
        if (flags & END_DEAD) and c == -1 and t == 0 and u == 0 and not fresh:
            out["truncated"][i] = u = 1
            out["ended"] += 1
            br["cut"] += 1
        f = 0.0
        if not (fresh or refused or c == -2 or c_prev == -2):
            dc = int(dead_cost[p]) if 0 <= p < P else 0
            phi = -(scale * float(dc if c == -1 else c))
            phi_prev = -(scale * float(dc if c_prev == -1 else c_prev))
            f = gamma * phi - phi_prev  # (two roundings: Python floats are never fused)
            br["shaped_nonzero"] += f != 0.0
        out["shaped"][i] = float(reward[i]) + f
        if 0 <= p < P and not fresh and not refused:
            guided = c != -2 and c_prev != -2
            if guided:
                out["counts"][p, GUIDED] += 1
                br["guided"] += 1
                if c_prev > 0 and c == c_prev - 1:
                    out["counts"][p, OPTIMAL] += 1
                    br["optimal"] += 1
                if c == -1 and c_prev >= 0:
                    out["counts"][p, DEAD_ENTERED] += 1
                    br["dead_entered"] += 1
            if c == -2:
                out["counts"][p, UNKNOWN] += 1
                br["unknown"] += 1
        out["cost"][i], out["acts"][i], out["dead"][i] = c, a, int(c == -1)
        out["seen"][i] = int((t | u) != 0)
    out["branches"] = br
    return out

"""Walk regions and push moves on the device (pw_walk_regions / pw_walk_pushes) on the random-shape puzzles and
the state lists of tests/shape_states.py: states with overlaps, whose push moves leave the grid, on every padding (4 .. 32), with
agents and movables beyond 8 x 8 cells, 32 movables and the 64 x 64 frame.  Every field of every item is compared with the
restatement of tests/walk_restatement.py by ``test_gpu_walk.Batch.check``; tests/test_walk_shapes_host.py pins what the lists
hold.  Successors outside their grid go back in as items and must come back skipped."""
import numpy as np
import pytest
import torch

import shape_states as SS
import walk_restatement as WR
from oracle import c_oracle
from pushworld_amd.search import walk_regions
from test_gpu_walk import TABLES, Batch
from test_walk_host import HAND

pytestmark = pytest.mark.gpu

# Inside successors that the second generation restates per case (None: all of them); every successor outside its grid goes in
# whatever their number.  A successor's region shares no step with its parent's, and the restatement takes 0.01 s (5, 30, 1)
# to 0.3 .. 0.75 s (32, 62, 5) per state: the rows of the larger cases are sampled, seeded, in row order.
GEN2_INSIDE = {SS.CASES[0]: None, SS.CASES[1]: 150, SS.CASES[2]: None, SS.CASES[3]: 40, SS.CASES[4]: 60, SS.CASES[5]: 6}


class ShapeBatch(Batch):
    """``test_gpu_walk.Batch`` over cases of shape_states: its oracle puzzles and its regions are the session's."""

    def __init__(self, cases, tables="all", extra=()):
        super().__init__([SS.text(c) for c in cases] + list(extra), tables)
        self.cases = list(cases)
        self.cps[:len(self.cases)] = [SS.puzzle(c) for c in self.cases]

    def region(self, pid, state):
        return SS.region(self.cases[pid], state) if pid < len(self.cases) else super().region(pid, state)


_BATCHES = {}


def _batch(cases, tables, extra=()):
    key = (tuple(cases), tables, tuple(extra))
    if key not in _BATCHES:
        _BATCHES[key] = ShapeBatch(cases, tables, extra)
    return _BATCHES[key]


def _mixed(tables):
    """All six puzzles in one set, and HAND.  Every one of the six has a movable beyond 8 x 8 cells and HAND has none, so
    step_tables="big" leaves HAND without tables; the 64 x 64 board gets none under any form (they end at 62 columns): the set
    runs the kernels' "tables for some puzzles" form under "all" too."""
    return _batch(SS.CASES, tables, [HAND])


def _check_tables(b, tables):
    """The engine built the tables the form asks for: for every puzzle of at most 62 columns ("all"), for those of them with a
    movable beyond 8 x 8 cells ("big"), for none."""
    with_tables, count = b.vec.engine.get_option("step_table_puzzles"), len(b.cps)
    fits = [cp for cp in b.cps if cp.width <= 62]
    if tables == "big":
        assert with_tables == sum(any(w > 8 or h > 8 for w, h in cp.py.sizes) for cp in fits)
        if count > 1:
            assert 0 < with_tables < count
    else:
        assert with_tables == (len(fits) if tables == "all" else 0)


@pytest.mark.parametrize("tables", TABLES)
@pytest.mark.parametrize("case", SS.CASES)
def test_listed_states(case, tables):
    b = _batch([case], tables)
    assert b.npad == SS.PADDING[case] and (b.map_h, b.map_w) == (SS.FRAME[case],) * 2
    _check_tables(b, tables)
    states = [s for _, s in SS.states(case)]
    reg, rows, want = b.check([0] * len(states), states)
    assert rows.num_rows == sum(len(w) for w in want) > 0
    if case == SS.CASES[5]:  # bit 31 of the moved mask: a negative int32
        assert bool((rows.moved < 0).any())


def _second_generation(case, want):
    """(states, skipped): the successors of the rows of `want` that go back in -- every one outside its grid, and the inside
    ones (all, or GEN2_INSIDE[case] of them drawn with a seed), in row order."""
    cp = SS.puzzle(case)
    succ = [pm.next_state for w in want for pm in w]
    inside = [k for k, s in enumerate(succ) if WR.in_grid(cp, s)]
    keep = set(k for k in range(len(succ)) if k not in set(inside))
    cap = GEN2_INSIDE[case]
    if cap is None or cap >= len(inside):
        keep.update(inside)
    else:
        keep.update(np.random.default_rng(7).choice(inside, size=cap, replace=False).tolist())
    picked = sorted(keep)
    states = [succ[k] for k in picked]
    return states, {i for i, s in enumerate(states) if not WR.in_grid(cp, s)}


@pytest.mark.parametrize("case", SS.CASES)
def test_second_generation(case):
    tables = TABLES[SS.CASES.index(case) % 3]
    b = _batch([case], tables)
    first = [s for _, s in SS.states(case)]
    want = [b.region(0, s).pushes for s in first]
    states, skipped = _second_generation(case, want)
    assert skipped and len(skipped) < len(states)
    if GEN2_INSIDE[case] is None:
        assert len(states) == sum(len(w) for w in want)
    # the ones outside their grid come back skipped (region_size -1, zero canon, a map of WALK_OUTSIDE, no rows), the others
    # are compared in full
    _, rows, want2 = b.check([0] * len(states), states, skipped=skipped)
    assert rows.num_rows > 0 and all(want2[i] == [] for i in skipped)


def _mixed_items():
    """(ids, states, mask, skipped) of the mixed set: the listed states of all six puzzles interleaved by puzzle, a state of the
    64 x 64 board first and last, two masked items, the ids -1 and `count`, an item with a movable at x = W, and HAND's
    initial state."""
    order = [5, 0, 1, 2, 3, 4]
    lists = {p: [s for _, s in SS.states(SS.CASES[p])] for p in order}
    ids, states = [], []
    for k in range(max(len(v) for v in lists.values())):
        for p in order:
            if k < len(lists[p]):
                ids.append(p)
                states.append(lists[p][k])
    assert ids[0] == 5
    mask = [1] * len(ids)
    skipped = set()
    for k in (4, len(ids) // 2):  # masked items
        mask[k] = 0
        skipped.add(k)
    ids.append(len(SS.CASES))
    states.append(c_oracle.COraclePuzzle(HAND).initial_state)
    mask.append(1)
    for bad_id in (-1, len(SS.CASES) + 1):  # ids outside the set: -1 and `count`
        ids.append(bad_id)
        states.append(lists[0][0])
        mask.append(1)
        skipped.add(len(ids) - 1)
    cp = SS.puzzle(SS.CASES[4])  # the last movable of (18, 30, 6) one column beyond the border
    out = list(cp.initial_state)
    out[-1] = (cp.width, out[-1][1])
    ids.append(4)
    states.append(tuple(out))
    mask.append(1)
    skipped.add(len(ids) - 1)
    ids.append(5)
    states.append(lists[5][-1])
    mask.append(1)
    return ids, states, mask, skipped


@pytest.mark.parametrize("tables", TABLES)
def test_mixed_set(tables):
    b = _mixed(tables)
    assert b.npad == 32 and (b.map_h, b.map_w) == (64, 64)  # 64 LDS rows per board for every item, 5 to 64 of them used
    assert sorted(cp.height for cp in b.cps) == [5, 14, 18, 32, 32, 32, 64]
    _check_tables(b, tables)
    ids, states, mask, skipped = _mixed_items()
    assert ids[0] == ids[-1] == 5 and len(skipped) == 5
    _, rows, want = b.check(ids, states, mask, skipped)
    assert rows.num_rows > 5000 and all(want[i] == [] for i in skipped)


def test_pushes_with_cap_on_the_mixed_set():
    b = _mixed("all")
    ids, states, mask, skipped = _mixed_items()
    t_ids = torch.as_tensor(np.asarray(ids, np.int32), device=b.dev)
    t_pos = b.pos(states)
    t_mask = torch.as_tensor(np.asarray(mask, np.uint8), device=b.dev)
    reg = walk_regions(b.vec, t_ids, t_pos, t_mask)
    counts = [0 if i in skipped else len(b.region(p, s).pushes) for i, (p, s) in enumerate(zip(ids, states))]
    total = sum(counts)
    assert reg.num_pushes == total and total > 5000
    assert (reg.offset.cpu().numpy() == np.concatenate([[0], np.cumsum(counts)])).all()
    full = reg.pushes()
    assert int(full.dropped.item()) == 0
    cap = total // 2
    # sentinels behind the buffers: nothing at or beyond `cap` is written
    item = torch.full((total,), -7, dtype=torch.int32, device=b.dev)
    frm = torch.full((total, 2), -7, dtype=torch.int8, device=b.dev)
    act = torch.full((total,), 77, dtype=torch.uint8, device=b.dev)
    walk = torch.full((total,), -7, dtype=torch.int32, device=b.dev)
    moved = torch.full((total,), -7, dtype=torch.int32, device=b.dev)
    goal = torch.full((total,), 77, dtype=torch.uint8, device=b.dev)
    nxt = torch.full((total, b.npad, 2), -7, dtype=torch.int8, device=b.dev)
    dropped = torch.full((1,), -1, dtype=torch.int64, device=b.dev)
    b.vec.engine.walk_pushes(t_ids, t_pos, t_mask, reg.offset, cap, item, frm, act, walk, moved, goal, nxt, dropped)
    assert int(dropped.item()) == total - cap
    for got, want, fill in ((item, full.item, -7), (frm, full.frm, -7), (act, full.action, 77), (walk, full.walk, -7),
                            (moved, full.moved, -7), (goal, full.goal, 77), (nxt, full.next_pos, -7)):
        assert torch.equal(got[:cap], want[:cap]) and bool((got[cap:] == fill).all())
    # the full rows are the restatement's (every field of them: test_mixed_set)
    at = 0
    fi, fa, fw = full.item.cpu().numpy(), full.action.cpu().numpy(), full.walk.cpu().numpy()
    for i, (pid, s) in enumerate(zip(ids, states)):
        if i in skipped:
            continue
        for pm in b.region(pid, s).pushes:
            assert (fi[at], fa[at], fw[at]) == (i, pm.action, pm.walk)
            at += 1
    assert at == total


def test_paths_from_overlapping_starts():
    """WalkRegions.path to the three farthest positions of four start states in which the agent itself overlaps something."""
    b = _mixed("all")
    eng = b.vec.engine
    ids, states = [], []
    for pid in (1, 2, 4, 5):  # agents of 9 x 8, 8 x 7, 1 x 7 and 4 x 1 cells
        cp = b.cps[pid]
        s = max((s for _, s in SS.states(SS.CASES[pid]) if SS.overlapping(cp, s) and SS.agent_overlaps(cp, s)),
                key=lambda s: len(b.region(pid, s).dist))
        ids.append(pid)
        states.append(s)
    reg = walk_regions(b.vec, torch.as_tensor(np.asarray(ids, np.int32), device=b.dev), b.pos(states), maps=True)
    for i, (pid, s) in enumerate(zip(ids, states)):
        r = b.region(pid, s)
        assert len(r.dist) >= 4
        start = np.ascontiguousarray(np.asarray(s, np.int8))
        for q in sorted(r.dist, key=lambda q: (-r.dist[q], q))[:3]:
            acts = reg.path(i, q)
            assert len(acts) == r.dist[q] > 0 and acts == WR.path(r, q)
            got, _ = eng.plan_states(pid, bytes(acts), start=start)
            assert tuple(got[-1, 0]) == q and (got[:, 1:] == start[None, 1:]).all()  # nothing else moved on the way

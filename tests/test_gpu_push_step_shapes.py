"""Stepping by pushes on the device (pw_step_push / pw_push_mask) on the random-shape puzzles and the state
lists of tests/shape_states.py: overlapping states on every padding -- the GS = 8, 16 and 32 instances of the kernel -- with cuts
that read the path ancestor through the parent bits, column 63 of the 64 x 64 board, and one set of all six puzzles whose lane
groups take items of boards of 14, 18, 32 and 64 rows one after another.  Every output of every item is compared field by field
with tests/push_step_restatement.py by ``test_gpu_push_step.Rig.run``; the regions are the session's (``shape_states.region``)."""
import numpy as np
import pytest
import torch

import push_step_restatement as SR
import shape_states as SS
from pushworld_amd.search import PUSH_NONE
from test_gpu_push_step import Rig
from test_gpu_walk import TABLES

pytestmark = pytest.mark.gpu

IDS = [str(c) for c in SS.CASES]
# max_steps of the cut runs, chosen on the CPU: with 0, 1, 2 steps on entry in turn, at least 20 rows per case (5 of the 64 x 64
# board's) end CUT after two or more moves -- the ancestor of `from` is read through the parent bits -- and 20 end DONE
CUT_MAX_STEPS = {SS.CASES[0]: 5, SS.CASES[1]: 16, SS.CASES[2]: 5, SS.CASES[3]: 20, SS.CASES[4]: 16, SS.CASES[5]: 30}
# (rows, rows DONE, the most moves of a row, rows DONE under the cut, rows CUT after two or more moves) per case, from the
# restatement; no listed state is a goal state, so without max_steps every row is DONE
PINNED = {
    SS.CASES[0]: (141, 141, 24, 46, 95),
    SS.CASES[1]: (1239, 1239, 56, 622, 617),
    SS.CASES[2]: (374, 374, 19, 215, 159),
    SS.CASES[3]: (4232, 4232, 61, 1630, 2602),
    SS.CASES[4]: (1358, 1358, 85, 622, 736),
    SS.CASES[5]: (3284, 3284, 116, 721, 2563),
}
# the mixed set also under two limits: cuts among boards of four heights.  Per max_steps: (rows DONE per puzzle, rows CUT after
# two or more moves) of the mixed batch, from the restatement
MIXED_MAX_STEPS = {"all": None, "big": 30, "none": 9}
MIXED_PINNED = {None: ([61, 76, 93, 93, 93, 24], 0), 30: ([61, 66, 93, 51, 75, 9], 85), 9: ([43, 24, 85, 4, 19, 1], 264)}
MIXED_ROWS = 3  # push rows per listed state in the mixed batch: the first, the middle and the last one


class ShapeRig(Rig):
    """``test_gpu_push_step.Rig`` over cases of shape_states: its oracle puzzles and its regions are the session's."""

    def __init__(self, cases, tables="all", max_steps=None):
        super().__init__([SS.text(c) for c in cases], tables, max_steps)
        self.cases = list(cases)
        self.cps = [SS.puzzle(c) for c in self.cases]

    def region(self, pid, state):
        return SS.region(self.cases[pid], state)


def case_items(case, pid=0):
    """(ids, states, choices): every push row of every listed state of the case, in list and row order."""
    ids, states, choices = [], [], []
    for listed in SS.states(case):
        for pm in SS.region(case, listed.state).pushes:
            ids.append(pid)
            states.append(listed.state)
            choices.append((pm.frm, pm.action))
    return ids, states, choices


def entry_steps(n):
    return [i % 3 for i in range(n)]


def _summary(results):
    return (len(results), sum(r.status == SR.DONE for r in results), max(r.moves for r in results))


@pytest.mark.parametrize("case", SS.CASES, ids=IDS)
def test_every_push_row_of_every_listed_state(case):
    cp = SS.puzzle(case)
    rig = ShapeRig([case])
    assert rig.npad == SS.PADDING[case]
    ids, states, choices = case_items(case)
    assert any(SS.overlapping(cp, s) for s in states)
    results = rig.run(ids, states, choices, pad=-7)
    assert all(r.status in (SR.DONE, SR.CUT) for r in results)
    print(case, _summary(results))
    assert _summary(results) == PINNED[case][:3]
    assert sum(r.status == SR.DONE for r in results) > 50 and max(r.moves for r in results) > 3
    if case == SS.CASES[5]:  # column 63 of the board (bit 63 of a row): a movable has a cell there after the push
        assert any(any(xy[0] + w == 64 for xy, (w, _) in zip(r.state, cp.py.sizes)) for r in results if r.status == SR.DONE)


@pytest.mark.parametrize("case", SS.CASES, ids=IDS)
def test_cuts(case):
    rig = ShapeRig([case], max_steps=CUT_MAX_STEPS[case])
    ids, states, choices = case_items(case)
    results = rig.run(ids, states, choices, steps=entry_steps(len(ids)), pad=-7)
    done = sum(r.status == SR.DONE for r in results)
    cut = [r for r, s, c in zip(results, states, choices) if r.status == SR.CUT and r.moves >= 2]
    print(case, done, len(cut))
    assert (done, len(cut)) == PINNED[case][3:]
    assert done >= 20 and len(cut) >= (5 if case == SS.CASES[5] else 20)
    # a cut row's agent stands on the path: the ancestor of `from`, `moves` layers from the start
    for r, s, c in zip(results, states, choices):
        if r.status == SR.CUT and r.moves >= 2:
            reg = SS.region(case, s)
            assert reg.dist[r.state[0]] == r.moves < reg.dist[tuple(c[0])] + 1 and r.state[1:] == tuple(s[1:]) and r.truncated


def mixed_items():
    """(ids, states, choices, refused) of the set of all six puzzles: of every listed state MIXED_ROWS push rows, and for the
    first two states of every puzzle three choices that are no push moves -- a `from` outside the region, a walk move and
    PUSH_NONE -- interleaved so that consecutive items come from different puzzles."""
    per = []
    for pid, case in enumerate(SS.CASES):
        cp, items = SS.puzzle(case), []
        aw, ah = cp.py.sizes[0]
        for k, listed in enumerate(SS.states(case)):
            reg = SS.region(case, listed.state)
            rows = reg.pushes
            picked = sorted({0, len(rows) // 2, len(rows) - 1}) if rows else []
            items += [(pid, listed.state, (rows[j].frm, rows[j].action), False) for j in picked[:MIXED_ROWS]]
            if k < 2:
                outside = next((x, y) for y in range(cp.height - ah + 1) for x in range(cp.width - aw + 1) if (x, y) not in reg.dist)
                walk = next((q, a) for q in sorted(reg.dist, key=lambda q: (q[1], q[0])) for a in range(4)
                            if len(cp.get_next_state_moved((q,) + tuple(listed.state[1:]), a)[1]) == 1)
                items += [(pid, listed.state, (outside, 1), True), (pid, listed.state, walk, True),
                          (pid, listed.state, ((0, 0), PUSH_NONE), True)]
        per.append(items)
    out = []
    for k in range(max(len(v) for v in per)):
        for pid in (5, 0, 3, 2, 1, 4):  # heights 64, 14, 32, 18, 32, 32
            if k < len(per[pid]):
                out.append(per[pid][k])
    return [it[0] for it in out], [it[1] for it in out], [it[2] for it in out], [it[3] for it in out]


@pytest.mark.parametrize("tables", TABLES)
def test_mixed_set(tables):
    rig = ShapeRig(SS.CASES, tables, max_steps=MIXED_MAX_STEPS[tables])
    assert rig.npad == 32 and sorted({cp.height for cp in rig.cps}) == [14, 18, 32, 64]
    ids, states, choices, refused = mixed_items()
    n = len(ids)
    assert all(a != b for a, b in zip(ids[:12], ids[1:13])) and set(ids) == set(range(6)) and sum(refused) == 36
    results = rig.run(ids, states, choices, steps=[i % 4 for i in range(n)], term=[9] * n, trunc=[5] * n, pad=-7)
    # (Rig.run has compared every field, and the whole row of a refused item -- sentinels included -- with what went in)
    assert [r.status == SR.REFUSED for r in results] == refused
    assert all((r.steps, r.terminated, r.truncated) == (i % 4, 9, 5) for i, r in enumerate(results) if r.status == SR.REFUSED)
    done = [sum(r.status == SR.DONE for r, p in zip(results, ids) if p == pid) for pid in range(6)]
    cut = sum(r.status == SR.CUT and r.moves >= 2 for r in results)
    print(tables, done, cut)
    assert (done, cut) == MIXED_PINNED[MIXED_MAX_STEPS[tables]] and n == 476
    assert min(done) >= 1 and sum(r.status == SR.CUT for r in results) == cut
    assert cut >= 50 or MIXED_MAX_STEPS[tables] is None


@pytest.mark.parametrize("tables", TABLES)
def test_push_mask_of_the_mixed_set(tables):
    rig = ShapeRig(SS.CASES, tables)
    ids, states, _, _ = mixed_items()
    n = len(ids)
    pos = np.zeros((n, rig.npad, 2), np.int8)
    want = np.zeros((n, 64, 64), np.uint8)
    counts = []
    for i, (pid, s) in enumerate(zip(ids, states)):
        pos[i, :len(s)] = np.asarray(s, np.int8)
        rows = rig.region(pid, s).pushes
        counts.append(len(rows))
        for pm in rows:
            assert not want[i, pm.frm[1], pm.frm[0]] >> pm.action & 1
            want[i, pm.frm[1], pm.frm[0]] |= 1 << pm.action
    mask = [0 if i in (3, n // 2) else 1 for i in range(n)]  # two masked items
    for i in (3, n // 2):
        want[i], counts[i] = 0, 0
    t_ids = torch.as_tensor(np.asarray(ids, np.int32), device=rig.dev)
    got = torch.full((n, 64, 64), 0xAB, dtype=torch.uint8, device=rig.dev)  # the fill is overwritten everywhere
    count = torch.full((n,), -7, dtype=torch.int32, device=rig.dev)
    rig.vec.engine.push_mask(t_ids, torch.as_tensor(pos, device=rig.dev), torch.as_tensor(np.asarray(mask, np.uint8), device=rig.dev),
                             got, count)
    assert (got.cpu().numpy() == want).all() and count.cpu().tolist() == counts
    assert sum(counts) > 30000 and any(want[i, 32:].any() for i in range(n) if ids[i] == 5)  # rows no other board has

"""A thin helper over ``push_table_restatement`` (``build``, ``query``, ``_key``) for the batched cost-to-go tables over pushes
(``pw_push_solve_batch_*``): the packed key of a canonical state, tables as plain arrays, and the comparison of
two tables BY STATE -- the batched kernel numbers the states of a layer as its schedule has it, so a device state is mapped to
the reference's state by (canon, boxes) and everything else is compared through that map.  Not a test."""
from collections import namedtuple

import numpy as np

import push_table_restatement as PT

Arrays = namedtuple("Arrays", "keys row_off cost best succ frm action flags")


def pack_key(canon, state):
    """The 64-bit key of the canonical state (canon, boxes of ``state``): movable j at bits 8 j, x in the low nibble, y in the
    high one; ``state`` holds the puzzle's movables and nothing else, so the bits beyond them are zero."""
    key = 0
    for j, (x, y) in enumerate(PT._key(canon, state)):
        assert j < 8 and 0 <= x < 16 and 0 <= y < 16
        key |= (x | (y << 4)) << (8 * j)
    return key


def keys_of(positions):
    """uint64 [S] keys of an integer array [S, N, 2] of positions (the agent already at canon)."""
    p = np.asarray(positions).astype(np.uint64)
    shifts = (np.arange(p.shape[1], dtype=np.uint64) * np.uint64(8))[None, :]
    return ((p[:, :, 0] | (p[:, :, 1] << np.uint64(4))) << shifts).sum(axis=1).astype(np.uint64)


def of_restated(t):
    """``Arrays`` of a ``push_table_restatement.Table``."""
    keys = np.array([pack_key(c, s) for s, c in zip(t.store.states, t.store.canons)], dtype=np.uint64)
    return Arrays(keys, np.asarray(t.row_off, np.int64), np.asarray(t.cost, np.int64), np.asarray(t.best, np.int64),
                  np.asarray(t.succ, np.int64), np.asarray(t.frm, np.int64).reshape(-1, 2), np.asarray(t.action, np.int64),
                  np.asarray(t.flags, np.int64))


def of_table(tab, n_mov):
    """``Arrays`` of a ``search.PushSolutionTable`` of a puzzle with ``n_mov`` movables."""
    pos, canon = (x.cpu().numpy().astype(np.int64) for x in tab.states())
    at = pos[:, :n_mov].copy()
    at[:, 0] = canon
    succ, frm, action, flags = (x.cpu().numpy().astype(np.int64) for x in tab.rows())
    return Arrays(keys_of(at), tab.offsets().cpu().numpy().astype(np.int64), tab.costs().cpu().numpy().astype(np.int64),
                  tab.best().cpu().numpy().astype(np.int64), succ, frm.reshape(-1, 2), action, flags)


def of_batch(batch, item):
    """``Arrays`` of item ``item`` of a ``search.PushSolutionTableBatch``; its keys are checked against its ``states``."""
    keys = batch.keys(item).cpu().numpy().astype(np.uint64)
    assert (keys_of(batch.states(item)) == keys).all()
    succ, frm, action, flags = (x.cpu().numpy().astype(np.int64) for x in batch.rows(item))
    return Arrays(keys, batch.offsets(item).cpu().numpy().astype(np.int64), batch.costs(item).cpu().numpy().astype(np.int64),
                  batch.best(item).cpu().numpy().astype(np.int64), succ, frm.reshape(-1, 2), action, flags)


def state_map(got, want):
    """int64 [S]: the state of ``want`` that state i of ``got`` is; asserts a bijection that keeps state 0."""
    S = len(want.keys)
    assert len(got.keys) == S
    order = np.argsort(want.keys, kind="stable")
    sorted_keys = want.keys[order]
    assert (sorted_keys[1:] != sorted_keys[:-1]).all()
    at = np.searchsorted(sorted_keys, got.keys)
    assert (at < S).all() and (sorted_keys[np.minimum(at, S - 1)] == got.keys).all()
    m = order[at].astype(np.int64)
    assert len(np.unique(m)) == S and m[0] == 0
    return m


def compare(got, want):
    """Every state and row of ``got`` against ``want`` by state: S, R, per state the cost, best and the row count, per row (in the
    state's own order) from, action and flags, and succ by state identity.  Returns the state map."""
    m = state_map(got, want)
    S, R = len(want.keys), len(want.succ)
    assert got.row_off.shape == (S + 1,) and got.row_off[0] == 0 and got.row_off[-1] == R == len(got.succ)
    counts = np.diff(got.row_off)
    assert (counts >= 0).all() and (counts == np.diff(want.row_off)[m]).all()
    assert (got.cost == want.cost[m]).all()
    assert (got.best == want.best[m]).all()
    state_of_row = np.repeat(np.arange(S), counts)
    k = np.arange(R) - got.row_off[state_of_row]
    r = want.row_off[m[state_of_row]] + k  # the same row of the same state over there
    assert (got.frm == want.frm[r]).all()
    assert (got.action == want.action[r]).all()
    assert (got.flags == want.flags[r]).all()
    inside = got.succ >= 0
    assert (inside == (want.succ[r] >= 0)).all() and (got.succ[~inside] == -1).all() and (got.succ < S).all()
    assert (m[got.succ[inside]] == want.succ[r][inside]).all()
    return m


def summary_of(a):
    """(states, rows, rows out of grid, of them goal rows, goal states, dead ends, largest cost, cost of the start): the tuple of
    ``push_table_restatement.EXPECT`` from a table's arrays."""
    out = a.succ < 0
    return (len(a.keys), len(a.succ), int(out.sum()), int((out & ((a.flags & 1) != 0)).sum()), int((a.cost == 0).sum()),
            int((a.cost == -1).sum()), int(a.cost.max()), int(a.cost[0]))

"""The cost index, the draws and the plans of csrc/pw_table_sample.inc on DEEP and LARGE tables: the puzzles of
tests/deep_puzzles.py.  tests/test_gpu_table_sample.py covers every case of the interface on tables of at most 500 rows and a
largest cost of 15; the paths it cannot reach are

  * the scan's carry over rounds of 256 words: cost_start tables of m = 256 (one full round), 257 (a second round of one word)
    and 1952 words (seven full rounds and a partial one);
  * chunks > 1 in the count and scatter launches: 6 workgroups over the 5 850 rows of the largest serpentine, 42 over the
    42 832 rows of `big`, and the batch handle where tables of 306 rows share those 42 workgroups per table with `big` (41 of
    their chunks hold no row);
  * plans of 1 949 actions in a plan_cap of 2 048, bands hundreds of buckets wide, cost_start reads far from word 0;
  * npad == 32: the fourth uint4 store and the half-word mask in word 8 of a 17-movable state;
  * a table above 2^20 rows (chunks = 1 024).

Reference: the numpy restatement (tests/table_sample_restatement.py) fed with the tables as read back; the tables themselves
are compared with the host reference over the C oracle (tests/deep_puzzles.py), or -- the table above 2^20 rows -- with their
own defining equations.  Every result is an integer: equality is exact.  The host loop of table_index_launch that halves
`chunks` needs more than 2^20 tables in one handle, one of them above 2^20 rows: it stays unexercised."""
import numpy as np
import pytest
import torch

import deep_puzzles
from table_sample_restatement import INF, draw_row, walk_plan
from test_gpu_table_sample import Table, assert_index

pytestmark = pytest.mark.gpu

OVER = "serpentine 62x61 overshoot"                          # m = 1952, chunks = 6, a dead-end bucket of 1 951 rows
M256, M257 = deep_puzzles.M256[0], deep_puzzles.M257[0]      # m = 256 / 257, chunks = 1
SINGLES = [M256, M257, OVER, "big"]                          # `big`: chunks = 42, buckets of thousands of rows
WORDS = {M256: 256, M257: 257, OVER: 1952, "big": 22}
B = 1000                                                     # environments per sample: not a multiple of 256
BIG = (1 << 31) - 1


class Single:
    """A per-puzzle table (K12) on an engine of its own, and its rows and cost index as read back."""

    def __init__(self, text, max_states=60000):
        from pushworld_amd.puzzle import PushWorldPuzzle
        from pushworld_amd.search import SolutionTable

        self.pz = PushWorldPuzzle(text=text)
        self.eng = self.pz._engine()
        self.tab = SolutionTable(self.pz, max_states=max_states)
        self.dev, self.npad, self.n_mov = self.tab.device, self.tab.npad, self.pz.num_movables
        tab = self.tab
        self.t = Table(self.n_mov, tab.states(), tab.successors(), tab.costs(), tab.actions(), tab.cost_index())

    def close(self):
        self.tab.close()


@pytest.fixture(scope="module")
def singles():
    s = {name: Single(deep_puzzles.text(name)) for name in SINGLES}
    yield s
    for x in s.values():
        x.close()


class Batch:
    """The batch handle (K13) over the set of deep_puzzles.batch_set: six tables of 19 .. 42 832 rows from one launch."""

    def __init__(self, golden):
        from pushworld_amd import _capi
        from pushworld_amd.search import SolutionTableBatch

        self.names, texts, self.hosts = deep_puzzles.batch_set(golden)
        self.parsed = [_capi.ParsedPuzzle(t) for t in texts]
        self.pset = _capi.PuzzleSet(self.parsed, 0)
        self.eng = _capi.Engine(self.pset, None, 3, 1, _capi.OBS_U8)
        self.b = b = SolutionTableBatch(self.eng, max_states_each=deep_puzzles.BATCH_CAP)
        self.dev, self.npad = b.device, b.npad
        assert b.status.cpu().tolist() == [0] * len(self.names)
        self.n_mov = [len(h.states[0]) for h in self.hosts]
        self.t = [Table(self.n_mov[i], b.states(i), b.successors(i), b.costs(i), b.actions(i), b.cost_index(i))
                  for i in range(len(self.names))]

    def close(self):
        self.b.close()


@pytest.fixture(scope="module")
def batch(golden):
    w = Batch(golden)
    yield w
    w.close()


# ---- index ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SINGLES)
def test_index_of_a_deep_table(singles, name):
    s = singles[name]
    want = deep_puzzles.host_table(name)
    assert (s.t.cost == want.cost).all() and (s.t.succ == want.succ).all()  # (the table itself: the FIFO numbering is the host's)
    assert len(s.t.cost_start) == WORDS[name] == s.tab.max_cost + 3
    assert_index(s.t, name)
    again = s.tab.cost_index()  # built once: a second read returns the same arrays
    assert (again[0].cpu().numpy() == s.t.rows_by_cost).all()
    assert (again[1].view(torch.int32).cpu().numpy() == s.t.cost_start).all()


def test_index_of_a_batch_with_a_large_and_small_tables(batch):
    """One three-launch index over tables of 42 832, 538, 306, 306, 150 and 19 rows: 42 workgroups per table."""
    rows = [len(t.cost) for t in batch.t]
    assert max(rows) == 42832 and rows.count(306) == 2 and min(rows) < 256
    for i, t in enumerate(batch.t):
        host = batch.hosts[i]
        assert sorted(t.cost.tolist()) == sorted(host.cost.tolist()), batch.names[i]
        assert_index(t, batch.names[i])
    # a cost_index call on one item leaves the cost_start of every table as it was
    n = len(batch.t)
    for j in reversed(range(n)):
        batch.b.cost_index(j)
        for i in range(n):
            rows_i, start_i = batch.b.cost_index(i)
            assert (start_i.view(torch.int32).cpu().numpy() == batch.t[i].cost_start).all(), (j, i)
            assert (rows_i.cpu().numpy() == batch.t[i].rows_by_cost).all(), (j, i)


# ---- sample --------------------------------------------------------------------------------------------------------------------
BANDS = ["default", "round_boundary", "max_cost", "per_env"]


def _band(band, max_cost, rng, dev):
    """(the `cost` argument, lo [B], hi [B])."""
    if band == "default":
        return (1, None), np.full(B, 1), np.full(B, BIG)
    if band == "round_boundary":  # straddles word 256 of cost_start
        return (250, 260), np.full(B, 250), np.full(B, 260)
    if band == "max_cost":
        return (max_cost, max_cost), np.full(B, max_cost), np.full(B, max_cost)
    lo = rng.integers(-5, max_cost + 51, size=B).astype(np.int32)
    hi = rng.integers(-5, max_cost + 51, size=B).astype(np.int32)
    assert (hi < lo).any() and (lo > max_cost).any() and (lo < 0).any()
    return (torch.as_tensor(lo).to(dev), torch.as_tensor(hi).to(dev)), lo, hi


def _sentinels(n, npad, rng, dev):
    """Random bytes in every slot of pos, sentinels in everything else."""
    host = dict(pos=rng.integers(-128, 128, size=(n, npad, 2)).astype(np.int8), steps=np.full(n, 77, np.int32),
                term=np.full(n, 3, np.uint8), trunc=np.full(n, 5, np.uint8), row=np.full(n, -77, np.int32),
                cost=np.full(n, -99, np.int32), counter=rng.integers(0, 1000, size=n).astype(np.int32))
    return host, {k: torch.as_tensor(v).to(dev) for k, v in host.items()}


def _expected(before, table_of, mask, seed, lo, hi):
    """What one sample launch leaves, from the restatement; table_of[e]: the Table of environment e, None: not this handle's."""
    exp = {k: v.copy() for k, v in before.items()}
    n = len(mask)
    drawn = np.zeros(n, dtype=bool)
    for e in range(n):
        t = table_of[e]
        if t is None or not mask[e]:
            continue  # untouched: the sentinels, the counter included
        ctr = int(before["counter"][e]) + 1
        row = draw_row(seed, e, ctr, int(lo[e]), int(hi[e]), t.rows_by_cost, t.cost_start)
        exp["counter"][e], exp["row"][e], exp["cost"][e] = ctr, row, t.cost[row]
        exp["pos"][e] = 0
        exp["pos"][e, :t.n_mov] = t.states[row]
        exp["steps"][e] = exp["term"][e] = exp["trunc"][e] = 0
        drawn[e] = True
    return exp, drawn


def _check_sample(table, eng, ids, table_of, band, max_cost, rng, seed, npad, dev, with_ids=True):
    before, d = _sentinels(B, npad, rng, dev)
    mask = (rng.integers(0, 4, size=B) > 0).astype(np.uint8)
    mask_d, ids_d = torch.as_tensor(mask).to(dev), torch.as_tensor(ids).to(dev)
    cost, lo, hi = _band(band, max_cost, rng, dev)
    got = table.sample(ids_d if with_ids else None, d["pos"], d["steps"], d["term"], d["trunc"], cost=cost, mask=mask_d, seed=seed,
                       counter=d["counter"], out=(d["row"], d["cost"]))
    assert got[0] is d["row"] and got[1] is d["cost"]
    exp, drawn = _expected(before, table_of, mask, seed, lo, hi)
    got = {k: v.cpu().numpy() for k, v in d.items()}
    assert drawn.sum() > B // 2 and (~drawn).sum() > B // 8
    for k in exp:  # drawn environments as restated; every other one bit-identical to what it held
        assert (got[k] == exp[k]).all(), (k, np.flatnonzero((got[k] != exp[k]).reshape(B, -1).any(1))[:5])
    mc = np.array([t.max_cost if t is not None else 0 for t in table_of])
    clo = np.minimum(np.maximum(lo, 0), mc)
    chi = np.minimum(np.maximum(np.maximum(hi, lo), 0), mc)
    assert ((got["cost"] >= clo) & (got["cost"] <= chi))[drawn].all()
    # the drawn states satisfy what the step and render kernels rely on
    sel = torch.as_tensor(np.flatnonzero(drawn)).to(dev)
    eng.validate(ids_d[sel].contiguous(), d["pos"][sel].contiguous())
    # round trip: the query maps every drawn state back to its row and cost
    index = torch.full((B,), -5, dtype=torch.int32, device=dev)
    qcost, qacts = torch.full_like(index, -5), torch.zeros((B,), dtype=torch.uint8, device=dev)
    table.query(ids_d if with_ids else None, d["pos"], mask=torch.as_tensor(drawn).to(dev), out=(index, qcost, qacts))
    assert (index.cpu().numpy()[drawn] == got["row"][drawn]).all() and (qcost.cpu().numpy()[drawn] == got["cost"][drawn]).all()
    return got, drawn


@pytest.mark.parametrize("band", BANDS)
@pytest.mark.parametrize("name", SINGLES)
def test_sample_from_a_deep_table(singles, name, band):
    """1 000 environments, every seventh of another puzzle (untouched), a quarter masked; the bands of the module's list."""
    s = singles[name]
    rng = np.random.default_rng(SINGLES.index(name) * 10 + BANDS.index(band))
    ids = np.where(np.arange(B) % 7 == 3, 5, 0).astype(np.int32)
    table_of = [s.t if p == 0 else None for p in ids]
    got, drawn = _check_sample(s.tab, s.eng, ids, table_of, band, s.t.max_cost, rng, 0xDEE9_0000 + BANDS.index(band), s.npad, s.dev)
    if band == "round_boundary" and s.t.max_cost >= 260:
        assert set(got["cost"][drawn].tolist()) == set(range(250, 261))  # both sides of the boundary are drawn
    if band == "max_cost":
        assert (got["cost"][drawn] == s.t.max_cost).all()


@pytest.mark.parametrize("band", BANDS)
def test_sample_from_the_batch(batch, band):
    """1 000 environments over the six tables of the handle, and one puzzle id outside the set."""
    rng = np.random.default_rng(50 + BANDS.index(band))
    n = len(batch.t)
    ids = (np.arange(B) * 5 % (n + 1)).astype(np.int32)  # n: no such puzzle in the set (untouched)
    table_of = [batch.t[p] if p < n else None for p in ids]
    _check_sample(batch.b, batch.eng, ids, table_of, band, 102, rng, 0xBA7C_0000 + BANDS.index(band), batch.npad, batch.dev)


@pytest.mark.parametrize("with_ids", [True, False])
def test_sample_with_17_movables(with_ids):
    """The pockets puzzle: 17 movables (the per-puzzle search takes them), an NP 32 engine -- all four uint4 stores of an
    environment, and the half-word mask in word 8 of the 9-word state.  The slots hold random bytes before the draw; after
    it the first 17 pairs are the row's state and the 15 trailing pairs are zero."""
    s = Single(deep_puzzles.text("pockets"))
    try:
        assert s.npad == 32 and s.n_mov == 17 and len(s.t.cost) == 15 and s.t.max_cost == 5
        want = deep_puzzles.host_table("pockets")
        assert (s.t.cost == want.cost).all() and (s.t.states == np.array(want.states).reshape(s.t.states.shape)).all()
        assert_index(s.t)
        rng = np.random.default_rng(32 + with_ids)
        ids = np.where(np.arange(B) % 7 == 3, 5, 0).astype(np.int32) if with_ids else np.zeros(B, np.int32)
        table_of = [s.t if p == 0 else None for p in ids]
        before, d = _sentinels(B, 32, rng, s.dev)
        mask = (rng.integers(0, 4, size=B) > 0).astype(np.uint8)
        ids_d = torch.as_tensor(ids).to(s.dev) if with_ids else None
        s.tab.sample(ids_d, d["pos"], d["steps"], d["term"], d["trunc"], cost=(0, None), mask=torch.as_tensor(mask).to(s.dev),
                     seed=17, counter=d["counter"], out=(d["row"], d["cost"]))
        exp, drawn = _expected(before, table_of, mask, 17, np.zeros(B, np.int64), np.full(B, BIG))
        got = {k: v.cpu().numpy() for k, v in d.items()}
        assert drawn.sum() > B // 2
        for k in exp:
            assert (got[k] == exp[k]).all(), k
        assert (got["pos"][drawn, 17:] == 0).all() and (before["pos"][drawn, 17:] != 0).any()
        assert (got["pos"][drawn, :17] == s.t.states[got["row"][drawn]]).all()
        assert (got["pos"][drawn, 16] != 0).any()  # (the seventeenth movable is not at the origin: the half word is kept)
        assert (got["pos"][~drawn] == before["pos"][~drawn]).all()
        assert set(got["row"][drawn].tolist()) == set(range(15))
        sel = torch.as_tensor(np.flatnonzero(drawn)).to(s.dev)
        s.eng.validate(torch.zeros((len(sel),), dtype=torch.int32, device=s.dev), d["pos"][sel].contiguous())
        index, qcost, _ = s.tab.query(None, d["pos"], mask=torch.as_tensor(drawn).to(s.dev))
        assert (index.cpu().numpy()[drawn] == got["row"][drawn]).all() and (qcost.cpu().numpy()[drawn] == got["cost"][drawn]).all()
    finally:
        s.close()


# ---- plans ---------------------------------------------------------------------------------------------------------------------
def _plans_from_every_row(s, cap, tie, seed, every):
    """Plans from every row of a per-puzzle table: plan_len == cost (-1 at dead ends), the plan of every `every`-th row equal
    to the restatement's walk, the bytes beyond every plan untouched, every plan REPLAY_VALID."""
    from pushworld_amd.search import REPLAY_VALID, replay_plans

    t, dev = s.t, s.dev
    n = len(t.cost)
    assert n % 256 != 0
    index_d = torch.arange(n, dtype=torch.int32, device=dev)
    plans_d = torch.full((n, cap), 0xEE, dtype=torch.uint8, device=dev)
    len_d = torch.full((n,), -7, dtype=torch.int32, device=dev)
    got = s.tab.plans(index_d, tie=tie, seed=seed, plan_cap=cap, out=(plans_d, len_d))
    assert got[0] is plans_d and got[1] is len_d
    plans, plan_len = plans_d.cpu().numpy(), len_d.cpu().numpy()
    cost = t.cost.astype(np.int64)
    assert cost[cost != INF].max() <= cap
    assert (plan_len == np.where(cost == INF, -1, cost)).all()
    beyond = np.arange(cap)[None, :] >= np.maximum(plan_len, 0)[:, None]
    assert (plans[beyond] == 0xEE).all() and (plans[~beyond] < 4).all()
    acts, succ, clist = t.acts.tolist(), t.succ.tolist(), t.cost.tolist()  # (plain lists: the walks are plain Python)
    for i in range(0, n, every):
        want = walk_plan(acts, succ, clist, i, 1 if tie == "uniform" else 0, seed, i)
        if want is None:
            assert plan_len[i] == -1
            continue
        assert plans[i, :len(want)].tolist() == want, i
    ids_d = torch.zeros((n,), dtype=torch.int32, device=dev)
    pos = np.zeros((n, s.npad, 2), dtype=np.int8)
    pos[:, :t.n_mov] = t.states
    out = replay_plans(s.eng, ids_d, plans_d, len_d, pos=torch.as_tensor(pos).to(dev), rows=False)
    assert (out.verdict.cpu().numpy()[cost != INF] == REPLAY_VALID).all()
    return plans, plan_len


def test_plans_of_1949_actions(singles):
    """5 850 items in a plan_cap of 2 048 (item i writes at i * 2 048).  On a path puzzle every state has ONE optimal action,
    so the uniform plans must equal the lowest ones byte for byte; those are compared with the restatement for every item,
    the uniform ones -- each step a hash in plain Python -- for every 97th."""
    s = singles[OVER]
    assert len(s.t.cost) == 5850 and s.t.max_cost == 1949
    assert max(bin(int(a) & 15).count("1") for a in s.t.acts) == 1
    low, low_len = _plans_from_every_row(s, 2048, "lowest", 0, 1)
    uni, uni_len = _plans_from_every_row(s, 2048, "uniform", 99, 97)
    assert (uni == low).all() and (uni_len == low_len).all() and low_len.max() == 1949
    # plan_cap = 1948: -2 exactly for the rows of cost 1949, their plan bytes untouched
    n = len(s.t.cost)
    plans_d = torch.full((n, 1948), 0xEE, dtype=torch.uint8, device=s.dev)
    len_d = torch.full((n,), -7, dtype=torch.int32, device=s.dev)
    s.tab.plans(torch.arange(n, dtype=torch.int32, device=s.dev), plan_cap=1948, out=(plans_d, len_d))
    short, short_len = plans_d.cpu().numpy(), len_d.cpu().numpy()
    over = s.t.cost == 1949
    assert over.sum() >= 1 and (short_len[over] == -2).all() and (short[over] == 0xEE).all()
    assert (short_len[~over] == low_len[~over]).all() and (short[~over] == low[~over, :1948]).all()


@pytest.mark.parametrize("tie", ["lowest", "uniform"])
def test_plans_from_42832_rows(singles, tie):
    """Every row of `big` (167 workgroups), plan_cap 32; every 7th plan against the restatement.  In the open room optimal
    actions tie: some uniform plan differs from the lowest one."""
    s = singles["big"]
    plans, plan_len = _plans_from_every_row(s, 32, tie, 4242, 7)
    if tie == "uniform":
        low = s.tab.plans(torch.arange(len(plan_len), dtype=torch.int32, device=s.dev), plan_cap=32)[0].cpu().numpy()
        k = np.arange(32)[None, :] < np.maximum(plan_len, 0)[:, None]
        assert ((plans != low) & k).any()


# ---- a table above 2^20 rows ----------------------------------------------------------------------------------------------------
def test_a_table_above_2_20_rows():
    """The open 6 x 6 room with three boxes.  The run reports 1 412 664 states, 39 260 of them goal states, 520 040 dead ends
    and a largest cost of 22 (the count is also what a layered search over the C oracle finds); only the range 2^20 .. 2^22
    is asserted.  The count and scatter launches run 1 024 workgroups, and row numbers pass 2^20.  A host search of that size is too slow in Python, so the reference is the table's own defining
    equations, which determine the costs uniquely: goal rows cost 0; every other row costs one more than the cheapest
    successor that is not the row itself, or is a dead end when all of those are.  successors() is checked against the C
    oracle on 2 000 random rows and on 50 rows of every cost bucket (all rows of a smaller bucket)."""
    s = Single(deep_puzzles.room3(), max_states=1 << 21)
    try:
        t, tab = s.t, s.tab
        n = tab.num_states
        print("states:", n, "max_cost:", tab.max_cost, "goal states:", tab.num_goal_states, "dead ends:", tab.num_dead_ends)
        assert (1 << 20) < n < (1 << 22) and len(t.cost) == n
        states, succ, cost = t.states, t.succ, t.cost.astype(np.int64)
        # the states are distinct, inside the room, and row 0 is the start
        key = np.zeros(n, dtype=np.int64)
        for j in range(s.n_mov):
            key = (key * 64 + states[:, j, 0]) * 64 + states[:, j, 1]
        assert len(np.unique(key)) == n and states.min() >= 1 and states.max() <= 6
        assert states[0].tolist() == [[int(x), int(y)] for x, y in s.pz.initial_state]
        # cost: the defining equations
        goal = np.ones(n, dtype=bool)
        for g, (gx, gy) in enumerate(s.pz.goal_state):
            goal &= (states[:, 1 + g, 0] == gx) & (states[:, 1 + g, 1] == gy)
        assert (succ >= 0).all() and (succ < n).all()
        moved = succ != np.arange(n)[:, None]
        cs = cost[succ]
        best = np.where(moved, cs, INF).min(axis=1)
        want = np.where(goal, 0, np.where(best == INF, INF, best + 1))
        assert (cost == want).all()
        finite = cost[cost != INF]
        assert (tab.num_goal_states, tab.num_dead_ends, tab.max_cost) == (int(goal.sum()), int((cost == INF).sum()), int(finite.max()))
        assert goal.sum() > 0 and (cost == INF).sum() > 0
        # acts: as the host reference sets them
        bits = np.zeros(n, dtype=np.int64)
        live = (cost != 0) & (cost != INF)
        for a in range(4):
            bits |= np.where(cs[:, a] != INF, 16 << a, 0)
            bits |= np.where(live & moved[:, a] & (cs[:, a] == cost - 1), 1 << a, 0)
        assert (t.acts == bits).all()
        # succ: the C oracle's successors, looked up through a dict of the read-back states
        from oracle import c_oracle

        oz = c_oracle.COraclePuzzle(deep_puzzles.room3())
        row_of = dict(zip(key.tolist(), range(n)))
        rng = np.random.default_rng(2020)
        picked = [rng.integers(0, n, size=2000)]
        bucket = np.where(cost == INF, tab.max_cost + 1, cost)
        for c in range(tab.max_cost + 2):
            rows = np.flatnonzero(bucket == c)
            assert len(rows) > 0, c
            picked.append(rows if len(rows) <= 50 else rng.choice(rows, size=50, replace=False))
        picked = np.unique(np.concatenate(picked))
        assert len(picked) >= 2000
        for r in picked.tolist():
            st = tuple(map(tuple, states[r].tolist()))
            for a in range(4):
                k = 0
                for x, y in oz.get_next_state(st, a):
                    k = (k * 64 + x) * 64 + y
                assert succ[r, a] == row_of[k], (r, a)
        # the index, and 4 096 exact draws over bands of every kind
        assert_index(t)
        m = 4096
        before, d = _sentinels(m, s.npad, rng, s.dev)
        lo = rng.integers(-5, tab.max_cost + 51, size=m).astype(np.int32)
        hi = rng.integers(-5, tab.max_cost + 51, size=m).astype(np.int32)
        tab.sample(None, d["pos"], d["steps"], d["term"], d["trunc"], cost=(torch.as_tensor(lo).to(s.dev), torch.as_tensor(hi).to(s.dev)),
                   seed=2 ** 63 + 5, counter=d["counter"], out=(d["row"], d["cost"]))
        exp, drawn = _expected(before, [t] * m, np.ones(m, np.uint8), 2 ** 63 + 5, lo, hi)
        got = {k: v.cpu().numpy() for k, v in d.items()}
        assert drawn.all()
        for k in exp:
            assert (got[k] == exp[k]).all(), k
        print("largest row drawn:", int(got["row"].max()))
    finally:
        s.close()

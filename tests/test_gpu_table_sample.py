"""Drawing from the cost-to-go tables on the device (csrc/pw_table_sample.inc; search.SolutionTable / SolutionTableBatch
``cost_index`` / ``sample`` / ``plans``; VecPushWorld.reset_from_tables / optimal_demonstrations) against the numpy restatement
(tests/table_sample_restatement.py) fed with the tables and the cost index as read back.  Every result is an integer:
equality is exact.

Ten tiny hand-written puzzles in three sets (engine NP 4, 8 and 16).  A table is rooted at the initial state and PushWorld is
irreversible, so "the start is a dead end" and "no solvable state at all" are the same table: `cornered` and `sealed` are two
ways to get there."""
import numpy as np
import pytest
import torch

from table_sample_restatement import INF, draw_row, walk_plan

pytestmark = pytest.mark.gpu


def _grid(rows):
    return "\n".join(" ".join(r) for r in rows) + "\n"


def _far():
    # 14 x 14 cells (16 x 16 with the border), all wall but the last row and a stub of the last column: the goal box ends in
    # the far corner, coordinate (14, 14)
    g = [["W"] * 14 for _ in range(14)]
    for x, y in [(x, 13) for x in range(14)] + [(13, y) for y in range(10, 14)] + [(12, 11), (12, 12)]:
        g[y][x] = "."
    g[13][0], g[13][2], g[13][13], g[10][13] = "A", "M0", "G0", "M1"
    return _grid(g)


def _big():
    g = [["."] * 6 for _ in range(6)]
    g[0][0], g[2][2], g[3][3], g[5][5] = "A", "M0", "M1", "G0"
    return _grid(g)


PUZZLES = {
    "corridor": _grid([["A", ".", "M0", ".", "G0"]]),                                    # 9 states, no ties, no dead ends
    "room": _grid([[".", ".", ".", "."], [".", "A", ".", "."], [".", ".", "M0", "."], [".", ".", ".", "G0"]]),  # open: ties
    "cornered": _grid([["M0", ".", "G0"], [".", "A", "."]]),                             # the start is a dead end
    "sealed": _grid([["A", "M0", ".", "W", "G0"]]),                                      # no solvable state at all
    "two_goals": _grid([["A", "M0", ".", "G0"], [".", "M1", ".", "G1"], [".", ".", ".", "."]]),
    "big": _big(),                                                                       # 42 832 states: beyond the cap below
    "long": _grid([["A", ".", "M0"] + ["."] * 13 + ["G0"]]),                             # 19 columns with the border: status 3
    "far": _far(),
    "eight": _grid([["M1", ".", ".", ".", "M2"], ["A", "M0", ".", "G0", "."], ["M3", "M5", ".", "M6", "M4"]]),   # 8 movables
    "nine": _grid([["M1", ".", ".", ".", "M2"], ["A", "M0", ".", "G0", "M7"], ["M3", "M5", ".", "M6", "M4"]]),  # 9: status 3
}
SETS = {
    4: ["corridor", "room", "cornered", "sealed", "two_goals", "big", "long"],
    8: ["eight", "corridor", "far", "room"],
    16: ["nine", "corridor", "eight", "room"],
}
K12 = {4: "long", 8: None, 16: "nine"}   # the puzzle beyond the batch kernel's limits gets a per-puzzle table
BATCH = {4: 1000, 8: 512, 16: 512}       # 1000: not a multiple of the 256 threads of a workgroup
CAP = 500                                # max_states_each: `big` exceeds it (status 2, no rows)
BUILT, TOO_MANY, NOT_SEARCHED = 0, 2, 3


class Table:
    """One puzzle's table as read back from the device, and its cost index."""

    def __init__(self, n_mov, states, succ, cost, acts, index):
        self.n_mov, self.states = n_mov, np.asarray(states)
        self.succ, self.cost, self.acts = (t.cpu().numpy() for t in (succ, cost, acts))
        self.rows_by_cost, self.cost_start = index[0].cpu().numpy(), index[1].view(torch.int32).cpu().numpy()
        finite = self.cost[self.cost != INF]
        self.max_cost = int(finite.max()) if finite.size else 0
        self.solvable = finite.size > 0


class World:
    def __init__(self, npad, observation=None):
        from pushworld_amd.puzzle import PushWorldPuzzle
        from pushworld_amd.vec_env import VecPushWorld

        self.npad, self.names = npad, SETS[npad]
        self.puzzles = [PushWorldPuzzle(text=PUZZLES[k]) for k in self.names]
        self.B = BATCH[npad]
        self.ids = (np.arange(self.B) * 5 % len(self.names)).astype(np.int32)  # mixed (5 is coprime to 4 and 7)
        self.vec = VecPushWorld(self.puzzles, self.B, puzzle_ids=self.ids, observation=observation, max_steps=None)
        assert self.vec.engine.np == npad
        self.batch = self.vec.solution_tables(max_states_each=CAP)
        self.single = self.vec.solution_table(self.names.index(K12[npad])) if K12[npad] else None
        self.tables = [self.batch] + ([self.single] if self.single else [])
        self.status = self.batch.status.cpu().numpy()
        self.host = {}  # puzzle -> Table
        for item, p in enumerate(self.batch.puzzles):
            if self.status[item] == BUILT:
                self.host[p] = Table(self.puzzles[p].num_movables, self.batch.states(item), self.batch.successors(item),
                                     self.batch.costs(item), self.batch.actions(item), self.batch.cost_index(item))
        if self.single:
            s = self.single
            self.host[s.puzzle_index] = Table(self.puzzles[s.puzzle_index].num_movables, s.states(), s.successors(), s.costs(),
                                              s.actions(), s.cost_index())
        self.dev = self.vec.device

    def close(self):
        self.batch.close()
        if self.single:
            self.single.close()


@pytest.fixture(scope="module")
def worlds():
    w = {npad: World(npad) for npad in (4, 8, 16)}
    yield w
    for x in w.values():
        x.close()


def test_the_puzzle_set_covers_the_cases(worlds):
    w4, w8, w16 = worlds[4], worlds[8], worlds[16]
    st4 = dict(zip(w4.names, w4.status))
    assert st4["big"] == TOO_MANY and st4["long"] == NOT_SEARCHED and all(st4[k] == BUILT for k in w4.names[:5])
    assert dict(zip(w16.names, w16.status))["nine"] == NOT_SEARCHED and (w8.status == BUILT).all()
    h4 = {k: w4.host.get(i) for i, k in enumerate(w4.names)}
    assert h4["big"] is None and not h4["cornered"].solvable and not h4["sealed"].solvable
    assert h4["cornered"].cost[0] == INF  # the start is a dead end
    assert (h4["room"].cost == INF).any() and h4["long"].solvable
    ties = [bin(int(a) & 15).count("1") > 1 for a in h4["room"].acts]
    assert any(ties)  # an open room where optimal actions tie
    h8 = {k: w8.host[i] for i, k in enumerate(w8.names)}
    assert h8["eight"].n_mov == 8 and h8["far"].states.max() == 14 and w16.host[0].n_mov == 9


def assert_index(t, tag=None):
    """The cost index of one table (a Table): what every index test asserts, here and in tests/test_gpu_table_deep.py."""
    rows, start = t.rows_by_cost, t.cost_start.astype(np.int64)
    assert (np.sort(rows) == np.arange(len(t.cost))).all(), tag  # a permutation of the rows
    bucket = np.where(t.cost == INF, t.max_cost + 1, t.cost).astype(np.int64)
    want = np.concatenate([[0], np.cumsum(np.bincount(bucket, minlength=t.max_cost + 2))])
    assert len(start) == t.max_cost + 3 and (start == want).all(), tag
    for c in range(t.max_cost + 2):  # every row of bucket c has cost c; the dead ends are the last bucket
        assert (bucket[rows[start[c]:start[c + 1]]] == c).all(), (tag, c)
    assert start[-1] == len(rows)


@pytest.mark.parametrize("npad", [4, 8, 16])
def test_index(worlds, npad):
    w = worlds[npad]
    assert len(w.host) >= 3
    for p, t in w.host.items():
        assert_index(t, p)
    # built once: a second read returns the same arrays
    item = int(np.flatnonzero(w.status == BUILT)[0])
    again = w.batch.cost_index(item)[0].cpu().numpy()
    assert (again == w.host[w.batch.puzzles[item]].rows_by_cost).all()
    for item in np.flatnonzero(w.status != BUILT):
        with pytest.raises(ValueError, match="no stored table"):
            w.batch.cost_index(int(item))


def _sentinels(w, rng):
    """The state arrays of a batch before a sample: initial states with random bytes in the slots beyond N, sentinels in
    everything else."""
    dev, B, npad = w.dev, w.B, w.npad
    pos = np.zeros((B, npad, 2), dtype=np.int8)
    for e, p in enumerate(w.ids):
        n_mov = w.puzzles[p].num_movables
        pos[e, :n_mov] = np.asarray(w.puzzles[p].initial_state, dtype=np.int8)
        pos[e, n_mov:] = rng.integers(-128, 128, size=(npad - n_mov, 2))
    host = dict(pos=pos, steps=np.full(B, 77, np.int32), term=np.full(B, 3, np.uint8), trunc=np.full(B, 5, np.uint8),
                row=np.full(B, -77, np.int32), cost=np.full(B, -99, np.int32),
                counter=rng.integers(0, 1000, size=B).astype(np.int32))
    return host, {k: torch.as_tensor(v).to(dev) for k, v in host.items()}


def _expected(w, before, mask, seed, lo, hi):
    """What the sample launches of all tables leave, from the restatement."""
    exp = {k: v.copy() for k, v in before.items()}
    drawn = np.zeros(w.B, dtype=bool)
    for e in range(w.B):
        t = w.host.get(int(w.ids[e]))
        if t is None or not mask[e]:
            continue  # untouched: the sentinels, the counter included
        if not t.solvable:
            exp["row"][e] = exp["cost"][e] = -1
            continue
        ctr = int(before["counter"][e]) + 1
        row = draw_row(seed, e, ctr, int(lo[e]), int(hi[e]), t.rows_by_cost, t.cost_start)
        exp["counter"][e], exp["row"][e], exp["cost"][e] = ctr, row, t.cost[row]
        exp["pos"][e] = 0
        exp["pos"][e, :t.n_mov] = t.states[row]
        exp["steps"][e] = exp["term"][e] = exp["trunc"][e] = 0
        drawn[e] = True
    return exp, drawn


def _run_sample(w, d, cost, mask_d, seed):
    ids_d = w.vec.puzzle_id
    for table in w.tables:
        got = table.sample(ids_d, d["pos"], d["steps"], d["term"], d["trunc"], cost=cost, mask=mask_d, seed=seed,
                           counter=d["counter"], out=(d["row"], d["cost"]))
        assert got[0] is d["row"] and got[1] is d["cost"]


BANDS = ["default", "scalar", "beyond", "per_env"]


@pytest.mark.parametrize("band", BANDS)
@pytest.mark.parametrize("npad", [4, 8, 16])
def test_sample_exact_and_round_trip(worlds, npad, band):
    w = worlds[npad]
    rng = np.random.default_rng(100 + npad)
    before, d = _sentinels(w, rng)
    mask = (rng.integers(0, 4, size=w.B) > 0).astype(np.uint8)
    mask_d = torch.as_tensor(mask).to(w.dev)
    seed = 0x1234_5678_9ABC_DEF0 + npad
    big = (1 << 31) - 1
    if band == "default":
        cost, lo, hi = (1, None), np.full(w.B, 1), np.full(w.B, big)
    elif band == "scalar":
        cost, lo, hi = (0, 2), np.full(w.B, 0), np.full(w.B, 2)
    elif band == "beyond":  # lo > max_cost of every table: lo = hi = max_cost
        cost, lo, hi = (100, 200), np.full(w.B, 100), np.full(w.B, 200)
    else:  # a band per environment: hi < lo, lo > max_cost and negative values among them
        lo = rng.integers(-2, 20, size=w.B).astype(np.int32)
        hi = (lo + rng.integers(-3, 6, size=w.B)).astype(np.int32)
        assert (hi < lo).any() and (lo > 15).any() and (lo < 0).any()
        cost = (torch.as_tensor(lo).to(w.dev), torch.as_tensor(hi).to(w.dev))
    _run_sample(w, d, cost, mask_d, seed)
    exp, drawn = _expected(w, before, mask, seed, lo, hi)
    got = {k: v.cpu().numpy() for k, v in d.items()}
    assert drawn.sum() > w.B // 4 and (~drawn).sum() > w.B // 8
    for k in exp:  # drawn environments as restated; every other one bit-identical to what it held (all-dead tables: -1 / -1)
        assert (got[k] == exp[k]).all(), (k, np.flatnonzero((got[k] != exp[k]).reshape(w.B, -1).any(1))[:5])
    clo = np.array([min(max(int(a), 0), w.host[int(p)].max_cost) if dr else 0 for a, p, dr in zip(lo, w.ids, drawn)])
    chi = np.array([min(max(int(b), int(a), 0), w.host[int(p)].max_cost) if dr else 0 for a, b, p, dr in zip(lo, hi, w.ids, drawn)])
    assert ((got["cost"] >= clo) & (got["cost"] <= chi))[drawn].all()
    dead = np.array([int(p) in w.host and not w.host[int(p)].solvable for p in w.ids]) & (mask > 0)
    if npad == 4:
        assert dead.any() and (got["row"][dead] == -1).all() and (got["cost"][dead] == -1).all()
        assert (got["counter"][dead] == before["counter"][dead]).all()
    # the drawn states satisfy what the step and render kernels rely on
    sel = torch.as_tensor(np.flatnonzero(drawn)).to(w.dev)
    w.vec.engine.validate(w.vec.puzzle_id[sel].contiguous(), d["pos"][sel].contiguous())
    # round trip: the query maps every drawn state back to its row and cost (decode against pack)
    index = torch.full((w.B,), -5, dtype=torch.int32, device=w.dev)
    qcost, qacts = torch.full_like(index, -5), torch.zeros((w.B,), dtype=torch.uint8, device=w.dev)
    for table in w.tables:
        table.query(w.vec.puzzle_id, d["pos"], mask=torch.as_tensor(drawn).to(w.dev), out=(index, qcost, qacts))
    assert (index.cpu().numpy()[drawn] == got["row"][drawn]).all() and (qcost.cpu().numpy()[drawn] == got["cost"][drawn]).all()


def test_single_table_without_ids(worlds):
    """The per-puzzle form with puzzle_id None: every environment is of the table's puzzle."""
    w = worlds[4]
    t, tab = w.host[w.single.puzzle_index], w.single
    n = 300
    pos = torch.full((n, 4, 2), 9, dtype=torch.int8, device=w.dev)
    steps = torch.full((n,), 5, dtype=torch.int32, device=w.dev)
    ctr = torch.zeros((n,), dtype=torch.int32, device=w.dev)
    row, cost = tab.sample(None, pos, steps, cost=(3, 6), seed=5, counter=ctr)
    want = np.array([draw_row(5, e, 1, 3, 6, t.rows_by_cost, t.cost_start) for e in range(n)])
    assert (row.cpu().numpy() == want).all() and (ctr.cpu().numpy() == 1).all() and (steps.cpu().numpy() == 0).all()
    assert ((cost.cpu().numpy() >= 3) & (cost.cpu().numpy() <= 6)).all()
    got = pos.cpu().numpy()
    assert (got[:, :t.n_mov] == t.states[want]).all() and (got[:, t.n_mov:] == 0).all()
    plans, plan_len = tab.plans(row, plan_cap=8)
    assert (plan_len.cpu().numpy() == cost.cpu().numpy()).all()


@pytest.mark.parametrize("npad", [4, 8, 16])
def test_sampled_states_are_real(worlds, npad):
    """reset_from_tables, then every environment follows the lowest optimal action of a fresh cost_to_go: it terminates at
    exactly its start_cost-th step and not before."""
    w = worlds[npad]
    vec = w.vec
    assert vec.reset_from_tables(w.tables, seed=3) is None  # (observation=None)
    start_cost, start_row = vec.start_cost.cpu().numpy().copy(), vec.start_row.cpu().numpy()
    has = np.array([int(p) in w.host and w.host[int(p)].solvable for p in w.ids])
    assert (start_cost[has] >= 1).all() and (start_cost[~has] == -1).all() and (start_row[~has] == -1).all()
    assert (vec.table_draws.view(torch.int32).cpu().numpy() == has).all() and vec.table_draws.dtype == torch.uint32
    init = vec.states()
    for e in np.flatnonzero(~has)[:50]:  # without a table: the initial state
        n_mov = w.puzzles[w.ids[e]].num_movables
        assert (init[e, :n_mov] == np.asarray(w.puzzles[w.ids[e]].initial_state)).all()
    first_done = np.zeros(w.B, dtype=np.int64)
    for t in range(1, int(start_cost.max()) + 1):
        _, cost, acts = vec.cost_to_go(w.tables)
        live = has & (first_done == 0)
        assert (cost.cpu().numpy()[live] == start_cost[live] - (t - 1)).all(), t
        bits = acts.to(torch.int32) & 15
        action = torch.where(bits > 0, torch.log2((bits & -bits).float()).to(torch.int32), torch.zeros_like(bits))
        _, _, term, _ = vec.step(action.to(torch.uint8))
        term = term.cpu().numpy() > 0
        first_done[(first_done == 0) & term & has] = t
    assert (first_done[has] == start_cost[has]).all()
    # a second call draws again (the counters advanced); seed restarts them: the same states as the first call
    vec.reset_from_tables(w.tables)
    assert (vec.table_draws.view(torch.int32).cpu().numpy() == 2 * has).all()
    vec.reset_from_tables(w.tables, seed=3)
    assert (vec.start_row.cpu().numpy() == start_row).all() and (vec.states() == init).all()


def _all_rows(w):
    """Every row of every table as one batch of plan starts: (ids, index, pos, table of each item)."""
    ids, index, pos = [], [], []
    for p, t in sorted(w.host.items()):
        n = len(t.cost)
        ids.append(np.full(n, p, np.int32)), index.append(np.arange(n, dtype=np.int32))
        full = np.zeros((n, w.npad, 2), dtype=np.int8)
        full[:, :t.n_mov] = t.states
        pos.append(full)
    return np.concatenate(ids), np.concatenate(index), np.concatenate(pos)


def _run_plans(w, index_d, ids_d, out, **kw):
    for table in w.tables:
        own = table.covers(ids_d)
        got = table.plans(index_d, ids_d, mask=own, out=out, **kw)
        assert got[0] is out[0] and got[1] is out[1]
    return out[0].cpu().numpy(), out[1].cpu().numpy()


@pytest.mark.parametrize("npad", [4, 8, 16])
def test_plans(worlds, npad):
    from pushworld_amd.search import REPLAY_VALID, replay_plans

    w = worlds[npad]
    ids, index, pos = _all_rows(w)
    n, cap, seed = len(ids), 16, 99
    assert n <= 4096 and n % 256 != 0
    ids_d, index_d, pos_d = (torch.as_tensor(a).to(w.dev) for a in (ids, index, pos))
    cost = np.concatenate([w.host[p].cost for p in sorted(w.host)]).astype(np.int64)

    def fresh(c=cap):
        return (torch.full((n, c), 0xEE, dtype=torch.uint8, device=w.dev), torch.full((n,), -7, dtype=torch.int32, device=w.dev))

    low, low_len = _run_plans(w, index_d, ids_d, fresh(), tie="lowest", plan_cap=cap)
    uni, uni_len = _run_plans(w, index_d, ids_d, fresh(), tie="uniform", seed=seed, plan_cap=cap)
    assert cost[cost != INF].max() <= cap
    want_len = np.where(cost == INF, -1, cost)
    assert (low_len == want_len).all() and (uni_len == want_len).all()  # plan_len == cost; a dead end gives -1
    item_of = {p: i for i, p in enumerate(w.batch.puzzles)}
    differs = {p: 0 for p in w.host}
    for i in range(n):
        p, row = int(ids[i]), int(index[i])
        t = w.host[p]
        if w.single is not None and p == w.single.puzzle_index:
            want = w.single.optimal_plan(row)
        else:
            want = w.batch.optimal_plan(item_of[p], row)
        if want is None:  # dead end: plans untouched
            assert (low[i] == 0xEE).all() and (uni[i] == 0xEE).all()
            continue
        k = len(want)
        assert low[i, :k].tolist() == want and (low[i, k:] == 0xEE).all(), i
        assert uni[i, :k].tolist() == walk_plan(t.acts, t.succ, t.cost, row, 1, seed, i) and (uni[i, k:] == 0xEE).all(), i
        differs[p] += low[i, :k].tolist() != uni[i, :k].tolist()
    assert differs[w.names.index("room")] > 0  # on the open room some uniform plan differs from the lowest one
    # every plan solves its puzzle from its row's state
    for plans, plan_len in ((low, low_len), (uni, uni_len)):
        out = replay_plans(w.vec.engine, ids_d, torch.as_tensor(plans).to(w.dev), torch.as_tensor(plan_len).to(w.dev),
                           pos=pos_d, rows=False)
        assert (out.verdict.cpu().numpy()[cost != INF] == REPLAY_VALID).all()
    # index -1 and rows beyond the table: -1, plans untouched; masked items untouched; a cap below the cost: -2
    odd = index.copy()
    odd[::3] = -1
    odd[1::3] = 1 << 20
    mask = np.ones(n, dtype=np.uint8)
    mask[2::3] = 0
    out = fresh()
    for table in w.tables:
        table.plans(torch.as_tensor(odd).to(w.dev), ids_d, mask=torch.as_tensor(mask).to(w.dev) & table.covers(ids_d), plan_cap=cap,
                    out=out)
    plans, plan_len = out[0].cpu().numpy(), out[1].cpu().numpy()
    assert (plans == 0xEE).all() and (plan_len[::3] == -1).all() and (plan_len[1::3] == -1).all() and (plan_len[2::3] == -7).all()
    short, short_len = _run_plans(w, index_d, ids_d, fresh(3), tie="lowest", plan_cap=3)
    over = (cost != INF) & (cost > 3)
    assert over.any() and (short_len[over] == -2).all() and (short[over] == 0xEE).all()
    assert (short_len[~over] == want_len[~over]).all() and (cost == 4).any()  # (cost 4: plan_cap = cost - 1)
    # a puzzle without a stored table in the handle: -1
    if npad == 4:
        big = torch.full((5,), w.names.index("big"), dtype=torch.int32, device=w.dev)
        _, plan_len = w.batch.plans(torch.zeros((5,), dtype=torch.int32, device=w.dev), big)
        assert (plan_len.cpu().numpy() == -1).all()


def test_reset_from_tables_and_optimal_demonstrations():
    """A mixed list of one batch and one per-puzzle table, on an environment with cell observations."""
    from pushworld_amd.search import REPLAY_VALID, SolutionTable

    w = World(4, observation="cells")
    try:
        vec = w.vec
        reset_mask = torch.as_tensor((np.arange(w.B) % 5 != 0)).to(w.dev)
        vec.reset()
        obs = vec.reset_from_tables(w.tables, cost=(2, 6), mask=reset_mask, seed=17)
        assert obs is vec.obs
        seen = obs.clone()
        assert (seen == vec.render()).all()  # the observation is the one of the sampled states
        start_cost = vec.start_cost.cpu().numpy()
        has = np.array([int(p) in w.host and w.host[int(p)].solvable for p in w.ids])
        rm = reset_mask.cpu().numpy()
        assert (start_cost[has & rm] >= 2).all() and (start_cost[has & rm] <= 6).all() and (start_cost[~(has & rm)] == -1).all()
        foreign = SolutionTable(w.puzzles[0])  # the same puzzle, on an engine of its own
        try:
            with pytest.raises(ValueError, match="made on this environment"):
                vec.reset_from_tables([foreign])
            with pytest.raises(ValueError, match="made on this environment"):
                vec.optimal_demonstrations([foreign])
        finally:
            foreign.close()
        mask = np.arange(w.B) % 3 != 1
        _, cost, _ = vec.cost_to_go(w.tables)
        cost = cost.cpu().numpy()
        for tie in ("lowest", "uniform"):
            demo = vec.optimal_demonstrations(w.tables, tie=tie, seed=4, mask=torch.as_tensor(mask).to(w.dev))
            T = demo.num_rows
            assert T == int(cost[mask & (cost > 0)].sum()) and T > 0
            verdict = demo.verdict.cpu().numpy()
            assert (verdict[mask & (cost >= 0)] == REPLAY_VALID).all()
            item, t, dcost, acts, action, done, reward = (x.cpu().numpy() for x in (
                demo.item, demo.t, demo.cost, demo.acts, demo.action, demo.done, demo.reward))
            assert dcost.dtype == np.int32 and acts.dtype == np.uint8 and demo.obs.shape[0] == T
            assert (dcost == cost[item] - t).all() and dcost.min() == 1  # falls by 1 per row to 1
            assert (((acts >> action) & 1) == 1).all()                      # the action taken is optimal in its row's state
            last = dcost == 1
            assert (done[last] == 1).all() and (done[~last] == 0).all() and (reward[last] == 10.0).all()
            offset = demo.offset.cpu().numpy()
            assert ((offset[1:] - offset[:-1]) == np.where(mask & (cost > 0), cost, 0)).all()
            # the rows' observations are the ones of their states
            probe = np.linspace(0, T - 1, 8).astype(np.int64)
            check = torch.empty((len(probe),) + vec.engine.cells_shape(), dtype=torch.uint8, device=w.dev)
            sel = torch.as_tensor(probe).to(w.dev)
            vec.engine.render_cells(demo.puzzle_id[sel].contiguous(), demo.pos[sel].contiguous(), check)
            assert (demo.obs[sel] == check).all()
        assert (vec.obs == seen).all() and (vec.start_cost.cpu().numpy() == start_cost).all()  # the environment is not touched
    finally:
        w.close()


def test_capture(worlds):
    """The sample launch alone in a graph (one stream, no parallel branches), replayed twice."""
    w = worlds[8]
    rng = np.random.default_rng(8)
    before, d = _sentinels(w, rng)
    before["counter"][:] = 0
    d["counter"].zero_()
    seed = 21
    w.batch.cost_index(0)  # (the index exists before the capture)
    ids_d = w.vec.puzzle_id
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        w.batch.sample(ids_d, d["pos"], d["steps"], d["term"], d["trunc"], cost=(1, None), seed=seed, counter=d["counter"],
                       out=(d["row"], d["cost"]))
    for k, v in before.items():  # (whatever the capture left: back to the sentinels)
        d[k].copy_(torch.as_tensor(v))
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    before["counter"][:] = 1  # the second replay starts from counter 1
    exp, drawn = _expected(w, before, np.ones(w.B, np.uint8), seed, np.full(w.B, 1), np.full(w.B, (1 << 31) - 1))
    assert drawn.all()
    got = {k: v.cpu().numpy() for k, v in d.items()}
    assert (got["counter"] == 2).all() and (got["pos"] == exp["pos"]).all() and (got["row"] == exp["row"]).all()

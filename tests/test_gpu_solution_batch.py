"""Batched cost-to-go tables (pw_solve_batch_* / search.SolutionTableBatch / VecPushWorld.solution_tables) against a host
reference over the compiled oracle: a forward FIFO search that records the four successors of every state, predecessor
lists, then a reverse breadth-first search from the goal states.  The kernel numbers the states of a breadth-first layer
in whatever order its threads arrive, so rows are compared BY STATE.  Every result is an integer: equality is exact."""
from collections import deque

import numpy as np
import pytest
import torch

from test_gpu_solution_table import EXPECT, INF

pytestmark = pytest.mark.gpu

CASES = list(EXPECT)
BEYOND = "bench:level1/Hockey Stick.pwp"          # 14 x 17 cells: more than 16 rows with the border -> status 3
SEVEN = "bench:level1/Carry The Bucket.pwp"       # 23 x 17 cells, 7 movables -> status 3, and a set padded to 8 movables
NINE = "bench:level1/Dont Get Distracted.pwp"     # 9 movables -> status 3, and a set padded to 16 movables
BUILT, TOO_MANY, NOT_SEARCHED, SUMMARY_ONLY = 0, 2, 3, 4


class HostTable:
    """The reference table of one puzzle, keyed by state; computed once per session and never changed."""

    def __init__(self, text):
        from oracle import c_oracle

        self.oz = oz = c_oracle.COraclePuzzle(text)
        states, index, succ = [oz.initial_state], {oz.initial_state: 0}, []
        i = 0
        while i < len(states):
            row = []
            for a in range(4):
                n = oz.get_next_state(states[i], a)
                if n not in index:
                    index[n] = len(states)
                    states.append(n)
                row.append(index[n])  # (nothing moved: n is states[i], the row points at itself)
            succ.append(row)
            i += 1
        total = len(states)
        preds = [[] for _ in range(total)]
        for i, row in enumerate(succ):
            for t in row:
                if t != i:
                    preds[t].append(i)
        cost = [INF] * total
        q = deque(i for i, s in enumerate(states) if oz.py.is_goal_state(s))
        goals = len(q)
        for i in q:
            cost[i] = 0
        while q:
            t = q.popleft()
            for p in preds[t]:
                if cost[p] == INF:
                    cost[p] = cost[t] + 1
                    q.append(p)
        acts = []
        for i, row in enumerate(succ):
            bits = 0
            for a, t in enumerate(row):
                if cost[t] != INF:
                    bits |= 16 << a
                if cost[i] not in (0, INF) and t != i and cost[t] == cost[i] - 1:
                    bits |= 1 << a
            acts.append(bits)
        self.states, self.index = states, index
        self.succ = np.array(succ, dtype=np.int32)
        self.cost = np.array(cost, dtype=np.uint16)
        self.acts = np.array(acts, dtype=np.uint8)
        finite = self.cost[self.cost != INF]
        self.summary = (total, goals, int((self.cost == INF).sum()), int(finite.max()) if finite.size else 0,
                        -1 if cost[0] == INF else int(cost[0]))


class World:
    """The ten cases (+ puzzles beyond the kernel's limits) as ONE set with an engine, and their host tables."""

    def __init__(self, golden, extra):
        from pushworld_amd import _capi

        self.keys = [k for k in CASES if k in golden.meta]
        assert len(self.keys) == len(CASES)
        self.all_keys = self.keys + list(extra)
        self.texts = [golden.text(k) for k in self.all_keys]
        self.pset = _capi.PuzzleSet([_capi.ParsedPuzzle(t) for t in self.texts], 0)
        self.eng = _capi.Engine(self.pset, None, 3, 1, _capi.OBS_U8)
        self.hosts = [_host(golden, k) for k in self.keys]
        self.true_rows = sum(len(h.states) for h in self.hosts)
        self.dims = [(golden.meta[k]["width"], golden.meta[k]["height"]) for k in self.keys]


_HOST = {}


def _host(golden, key):
    if key not in _HOST:
        _HOST[key] = HostTable(golden.text(key))
    return _HOST[key]


@pytest.fixture(scope="module")
def world(golden):
    return World(golden, [BEYOND])


@pytest.fixture(scope="module")
def batch(world):
    from pushworld_amd.search import SolutionTableBatch

    b = SolutionTableBatch(world.eng)  # one summary-only run sizes the pool, ONE run builds and stores every table
    yield b
    b.close()


def _summaries(b):
    return b.status.cpu().numpy(), b.summary.cpu().numpy(), b.row_offset.cpu().numpy()


def _host_rows(b, i, host):
    """The host index of every row of item i; asserts that the rows are exactly the host's states, the start first."""
    states = b.states(i)
    hmap = np.array([host.index[tuple((int(x), int(y)) for x, y in s)] for s in states])
    assert len(hmap) == len(host.states) and len(set(hmap.tolist())) == len(hmap) and hmap[0] == 0
    return hmap


def _assert_exact(b, i, host, tag=None):
    hmap = _host_rows(b, i, host)
    succ, cost, acts = b.successors(i).cpu().numpy(), b.costs(i).cpu().numpy(), b.actions(i).cpu().numpy()
    assert succ.dtype == np.int32 and cost.dtype == np.uint16 and acts.dtype == np.uint8
    assert (cost == host.cost[hmap]).all(), (i, tag)
    assert (acts == host.acts[hmap]).all(), (i, tag)
    assert succ.shape == (len(hmap), 4) and (succ >= 0).all() and (succ < len(hmap)).all()
    assert (hmap[succ] == host.succ[hmap]).all(), (i, tag)  # every entry points at the row of the host's successor


def test_host_reference_matches_the_recorded_summary(world):
    for k, h in zip(world.keys, world.hosts):
        assert h.summary[:4] == EXPECT[k][:4] and h.summary[4] == (-1 if EXPECT[k][4] == INF else EXPECT[k][4]), k


def test_one_run_equals_the_host_reference(world, batch):
    """Ten tables from one launch: the closed set in LDS (19 .. 994 states) and at 2^16 slots (5 828 / 7 480 / 10 659), a
    puzzle without goals, one without dead ends; the puzzle beyond 16 rows in the same set is not searched."""
    status, summary, row_off = _summaries(batch)
    n = len(world.keys)
    assert status.tolist() == [BUILT] * n + [NOT_SEARCHED]
    assert row_off[n] == -1 and batch.rows_needed == world.true_rows == batch.rows
    for i, k in enumerate(world.keys):
        want = EXPECT[k]
        assert tuple(summary[i]) == want[:4] + (-1 if want[4] == INF else want[4],), k
        assert (int(batch.num_states[i]), int(batch.num_goals[i]), int(batch.dead_ends[i]), int(batch.max_cost[i]),
                int(batch.start_cost[i])) == tuple(summary[i])
        _assert_exact(batch, i, world.hosts[i], k)
    # the stored tables tile the pool without overlap
    spans = sorted((int(row_off[i]), int(summary[i, 0])) for i in range(n))
    assert spans[0][0] == 0 and all(a + c == b for (a, c), (b, _) in zip(spans, spans[1:]))
    with pytest.raises(ValueError, match="no stored table"):
        batch.costs(n)
    with pytest.raises(ValueError, match="out of bounds"):
        batch.costs(n + 1)


ROOM = "\n".join(" ".join(row) for row in [
    [".", ".", ".", ".", ".", ".", "."],
    [".", "A", ".", ".", ".", ".", "."],
    [".", ".", ".", "M0", ".", ".", "."],
    [".", ".", ".", ".", ".", ".", "."],
    [".", ".", "M1", ".", ".", "G0", "."],
    [".", ".", ".", ".", ".", ".", "."],
    [".", ".", ".", ".", ".", ".", "."],
]) + "\n"


def test_the_2_20_level_equals_the_per_puzzle_table():
    """An open 7 x 7 room with the agent, a goal box and one more box: more than 32 768 states, so the closed set climbs to
    2^20 slots.  Reference: search.SolutionTable of the same puzzle (the per-puzzle path)."""
    from pushworld_amd.puzzle import PushWorldPuzzle
    from pushworld_amd.search import SolutionTable, SolutionTableBatch

    pz = PushWorldPuzzle(text=ROOM)
    tab = SolutionTable(pz, max_states=1 << 18)
    b = SolutionTableBatch(pz._engine(), [tab.puzzle_index], max_states_each=1 << 17)
    try:
        assert int(b.status[0]) == BUILT
        assert int(b.num_states[0]) > 32768
        c0 = -1 if tab.initial_cost is None else tab.initial_cost
        assert tuple(b.summary[0].tolist()) == (tab.num_states, tab.num_goal_states, tab.num_dead_ends, tab.max_cost, c0)
        states = tab.states()
        pos = np.zeros((tab.num_states, tab.npad, 2), dtype=np.int8)
        pos[:, :states.shape[1]] = states
        ids = torch.full((tab.num_states,), tab.puzzle_index, dtype=torch.int32, device=tab.device)
        index, cost, acts = b.query(ids, torch.as_tensor(pos).to(tab.device))
        want = tab.costs().cpu().numpy().astype(np.int32)
        assert (cost.cpu().numpy() == np.where(want == INF, -1, want)).all()
        assert (acts.cpu().numpy() == tab.actions().cpu().numpy()).all()
        index = index.cpu().numpy()
        assert (np.sort(index) == np.arange(tab.num_states)).all()  # every state has a row of its own
        assert (b.states(0)[index] == states).all()
    finally:
        b.close()
        tab.close()


def test_state_cap(world):
    from pushworld_amd.search import SolutionTableBatch

    b = SolutionTableBatch(world.eng, max_states_each=300)
    try:
        status, summary, _ = _summaries(b)
        for i, (k, h) in enumerate(zip(world.keys, world.hosts)):
            if len(h.states) > 300:
                assert status[i] == TOO_MANY, k
            else:
                assert status[i] == BUILT and tuple(summary[i]) == h.summary, k
                _assert_exact(b, i, h, k)
        assert status[len(world.keys)] == NOT_SEARCHED
        assert b.rows_needed == sum(len(h.states) for h in world.hosts if len(h.states) <= 300)
    finally:
        b.close()


def test_row_pool_too_small_and_exactly_large_enough(world):
    from pushworld_amd.search import SolutionTableBatch

    n = len(world.keys)
    cap = world.true_rows // 2
    b = SolutionTableBatch(world.eng, rows=cap)
    try:
        status, summary, row_off = _summaries(b)
        assert (status[:n] == SUMMARY_ONLY).sum() >= 1 and set(status[:n].tolist()) <= {BUILT, SUMMARY_ONLY}
        assert b.rows_needed == world.true_rows  # the needed-rows word is the true sum, whatever was stored
        stored = 0
        for i, h in enumerate(world.hosts):
            assert tuple(summary[i]) == h.summary, world.keys[i]  # valid with and without rows
            if status[i] == BUILT:
                assert 0 <= row_off[i] and row_off[i] + summary[i, 0] <= cap
                stored += int(summary[i, 0])
                _assert_exact(b, i, h, world.keys[i])
            else:
                assert row_off[i] == -1
                with pytest.raises(ValueError, match="no stored table"):
                    b.costs(i)
        assert stored <= cap
    finally:
        b.close()
    for rows in (world.true_rows, world.true_rows + 1000):
        b = SolutionTableBatch(world.eng, rows=rows)
        try:
            assert b.status.cpu().tolist() == [BUILT] * n + [NOT_SEARCHED], rows  # nothing is left out
            _assert_exact(b, CASES.index("pytest:trivial_tool.pwp"), world.hosts[CASES.index("pytest:trivial_tool.pwp")])
        finally:
            b.close()
    b = SolutionTableBatch(world.eng, rows=0)  # summaries only
    try:
        status, summary, _ = _summaries(b)
        assert status.tolist() == [SUMMARY_ONLY] * n + [NOT_SEARCHED]
        assert [tuple(r) for r in summary[:n]] == [h.summary for h in world.hosts]
    finally:
        b.close()


def _sorted_rows(b, i):
    """keys / cost / acts of item i in key order, on the device (numbering inside a layer is the schedule's)."""
    k = b.keys(i)
    k, order = torch.sort(k)
    return k, b.costs(i).view(torch.int16)[order], b.actions(i)[order]


def test_scheduling_changes_nothing(world, batch):
    """The set repeated past three workgroups per CU, at 1 and at 8 persistent workgroups per CU: the same summaries and,
    state by state, the same cost and action bits as the set built once."""
    from pushworld_amd.search import SolutionTableBatch

    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    n_set = len(world.all_keys)
    rep = np.tile(np.arange(n_set, dtype=np.int32), -(-(3 * ncu + 1) // n_set))
    assert len(rep) > 3 * ncu
    base_status, base_summary, _ = _summaries(batch)
    base = [_sorted_rows(batch, i) for i in range(len(world.keys))]
    try:
        for per_cu in (1, 8):
            world.eng.set_option("search_batch_groups_per_cu", per_cu)
            b = SolutionTableBatch(world.eng, rep)
            try:
                status, summary, _ = _summaries(b)
                assert (status == base_status[rep]).all() and (summary == base_summary[rep]).all(), per_cu
                same = torch.ones((), dtype=torch.bool, device=b.device)
                for item, p in enumerate(rep):
                    if status[item] != BUILT:
                        continue
                    k, c, a = _sorted_rows(b, item)
                    same &= (k == base[p][0]).all() & (c == base[p][1]).all() & (a == base[p][2]).all()  # (equal lengths)
                assert bool(same), per_cu
            finally:
                b.close()
    finally:
        world.eng.set_option("search_batch_groups_per_cu", 0)


def _query_case(golden, extra, npad):
    """A mixed batch over the set: random walks from the initial states, one state outside the grid, one unreachable state
    per puzzle, masked items, items of puzzles without a table; garbage in the pos entries beyond each puzzle's movables."""
    from pushworld_amd.search import SolutionTableBatch

    w = World(golden, extra)
    assert w.eng.np == npad
    n_cases = len(w.keys)
    no_table = CASES.index("rand:42")  # left out of the build: a puzzle of the set without a table
    b = SolutionTableBatch(w.eng, [i for i in range(len(w.all_keys)) if i != no_table])
    item_of = {p: i for i, p in enumerate(b.puzzles)}
    rng = np.random.default_rng(2024)
    ids, states, kind = [], [], []
    for p in range(n_cases):
        h = w.hosts[p]
        W, H = w.dims[p]
        N = len(h.states[0])
        for _ in range(6):  # random walks from the initial state
            i = 0
            for _ in range(40):
                ids.append(p), states.append(h.states[i]), kind.append("in")
                i = int(h.succ[i, rng.integers(0, 4)])
        s = [list(xy) for xy in h.states[int(rng.integers(0, len(h.states)))]]
        # one coordinate outside: just past the grid (inside 0 .. 15, the case the key alone cannot tell) or far outside
        s[p % N][p % 2] = (H if p % 2 else W) if p % 3 == 0 else [-1, 16, -128, 127, 100, -2, 64, 31, 17, 20][p]
        ids.append(p), states.append(tuple(tuple(xy) for xy in s)), kind.append("off")
        for _ in range(1000):  # a state inside the grid that the start does not reach
            s = tuple((int(rng.integers(0, W)), int(rng.integers(0, H))) for _ in range(N))
            if s not in h.index:
                ids.append(p), states.append(s), kind.append("out")
                break
        for _ in range(4):
            ids.append(p), states.append(h.states[int(rng.integers(0, len(h.states)))]), kind.append("masked")
    for p in range(n_cases, len(w.all_keys)):  # not searched: no table
        ids.append(p), states.append(((1, 1),)), kind.append("foreign")
    n = len(ids)
    assert {"in", "off", "out", "masked", "foreign"} <= set(kind)
    pos = rng.integers(-128, 128, size=(n, npad, 2)).astype(np.int8)  # garbage everywhere, then the movables
    for i, s in enumerate(states):
        pos[i, :len(s)] = np.array(s, dtype=np.int64).astype(np.int8)
    mask = np.array([k != "masked" for k in kind], dtype=np.uint8)
    exp_cost, exp_acts = np.full(n, -99, dtype=np.int32), np.full(n, 0xAB, dtype=np.uint8)
    found = np.zeros(n, dtype=bool)
    for i, (p, s, k) in enumerate(zip(ids, states, kind)):
        if k in ("masked", "foreign") or p == no_table:
            continue  # left untouched: the sentinels
        if k == "in":
            j = w.hosts[p].index[s]
            c = int(w.hosts[p].cost[j])
            exp_cost[i], exp_acts[i], found[i] = (-1 if c == INF else c), w.hosts[p].acts[j], True
        else:
            exp_cost[i], exp_acts[i] = -2, 0
    untouched = np.array([k in ("masked", "foreign") or p == no_table for p, k in zip(ids, kind)])
    assert untouched.sum() > 4 * n_cases and found.sum() > 1000
    return w, b, item_of, np.array(ids, dtype=np.int32), states, pos, mask, exp_cost, exp_acts, found, untouched


@pytest.mark.parametrize("npad, extra", [(4, [BEYOND]), (8, [SEVEN]), (16, [SEVEN, NINE])])
def test_query(golden, npad, extra):
    w, b, item_of, ids, states, pos, mask, exp_cost, exp_acts, found, untouched = _query_case(golden, extra, npad)
    try:
        dev, n = b.device, len(ids)
        ids_d, pos_d, mask_d = torch.as_tensor(ids).to(dev), torch.as_tensor(pos).to(dev), torch.as_tensor(mask).to(dev)

        def sentinels():
            return (torch.full((n,), -77, dtype=torch.int32, device=dev), torch.full((n,), -99, dtype=torch.int32, device=dev),
                    torch.full((n,), 0xAB, dtype=torch.uint8, device=dev))

        def check(got):
            index, cost, acts = (t.cpu().numpy() for t in got)
            assert (cost == exp_cost).all() and (acts == exp_acts).all()
            assert (index[untouched] == -77).all() and (index[~untouched & ~found] == -1).all()
            rows = {}
            for i in np.flatnonzero(found):  # the row a state is mapped to holds that state
                p = int(ids[i])
                if p not in rows:
                    rows[p] = b.states(item_of[p])
                assert tuple(map(tuple, rows[p][index[i]])) == states[i], i

        out = sentinels()
        got = b.query(ids_d, pos_d, mask=mask_d, out=out)
        assert all(g is o for g, o in zip(got, out))
        check(got)
        fresh = b.query(ids_d, pos_d, mask=mask_d.bool())  # without `out` the untouched items are -1 / -2 / 0
        assert (fresh[0].cpu().numpy()[untouched] == -1).all() and (fresh[1].cpu().numpy()[untouched] == -2).all()
        assert (fresh[2].cpu().numpy()[untouched] == 0).all()
        assert (fresh[1].cpu().numpy()[~untouched] == exp_cost[~untouched]).all()
        # captured once, replayed on other inputs: one stream, no parallel branches
        static_pos, graphed = torch.zeros_like(pos_d), sentinels()
        static_pos[:, 0] = 1  # (any valid-looking input for the capture run)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            b.query(ids_d, static_pos, mask=mask_d, out=graphed)
        for t, s in zip(graphed, sentinels()):
            t.copy_(s)
        static_pos.copy_(pos_d)
        g.replay()
        torch.cuda.synchronize()
        check(graphed)
    finally:
        b.close()


def test_vec_env_tables_equal_the_per_puzzle_tables(golden):
    """solution_tables() + cost_to_go([batch]) on a stepped mixed batch equals cost_to_go over per-puzzle solution_table()s
    (cost and action bits; the row numbers name the same states); optimal_plan(i) is a valid plan of length start_cost."""
    from pushworld_amd.puzzle import PushWorldPuzzle
    from pushworld_amd.vec_env import VecPushWorld

    keys = ["pytest:trivial_tool.pwp", "l0:level0/base/train/level_0_base_train_0.pwp", "pytest:transitive_pushing.pwp",
            "rand:3"]
    puzzles = [PushWorldPuzzle(text=golden.text(k)) for k in keys]
    B = 256
    ids = np.arange(B) % 4
    vec = VecPushWorld(puzzles, B, puzzle_ids=ids, observation=None, max_steps=None)
    singles = [vec.solution_table(i) for i in range(3)]  # puzzle 3 has a table in the batch only
    tabs = vec.solution_tables()
    try:
        assert tabs.status.cpu().tolist() == [BUILT] * 4
        single_states = [t.states() for t in singles]
        batch_states = [tabs.states(i) for i in range(4)]
        vec.reset()
        rng = np.random.default_rng(11)
        for step in range(25):
            bi, bc, ba = (t.cpu().numpy() for t in vec.cost_to_go([tabs]))
            si, sc, sa = (t.cpu().numpy() for t in vec.cost_to_go(singles))
            has = ids < 3
            assert (bc[has] == sc[has]).all() and (ba[has] == sa[has]).all(), step
            assert (sc[~has] == -2).all() and (bc[~has] >= -1).all()
            live = vec.states()
            for e in range(B):
                p = int(ids[e])
                n_mov = puzzles[p].num_movables
                assert (batch_states[p][bi[e]] == live[e][:n_mov]).all(), (step, e)
                if p < 3:
                    assert (single_states[p][si[e]] == live[e][:n_mov]).all(), (step, e)
            # a batch and per-puzzle tables in one list fill the same outputs
            mi, mc, ma = (t.cpu().numpy() for t in vec.cost_to_go([singles[0], tabs]))
            assert (mc == bc).all() and (ma == ba).all()
            vec.step(torch.as_tensor(rng.integers(0, 4, size=B).astype(np.uint8), device=vec.device))
        for i, k in enumerate(keys):
            plan = tabs.optimal_plan(i)
            assert len(plan) == int(tabs.start_cost[i]) == EXPECT[k][4], k
            assert puzzles[i].is_valid_plan(plan), k
    finally:
        tabs.close()
        for t in singles:
            t.close()


def test_difficulty_labels(world):
    from pushworld_amd import generate

    plan_len, states, share = generate.difficulty(world.pset)
    for i, h in enumerate(world.hosts):
        assert (plan_len[i], states[i]) == (h.summary[4], h.summary[0]) and share[i] == h.summary[2] / h.summary[0]
    assert plan_len[-1] == -1 and states[-1] == 0 and np.isnan(share[-1])


@pytest.mark.parametrize("per_cu", [1, 8])
def test_deep_and_large_tables_in_one_launch(golden, per_cu):
    """Both 14-wide serpentines (largest cost 102 and 101: a hundred sweeps inside the persistent workgroup, a barrier each),
    the 42 832 rows of the open room with two boxes and three tiny puzzles in ONE launch, at 1 and at 8 workgroups per CU:
    every table BUILT, summaries and -- state by state -- successors, costs and action bits equal to the host reference."""
    import deep_puzzles
    from pushworld_amd import _capi
    from pushworld_amd.search import SolutionTableBatch

    names, texts, hosts = deep_puzzles.batch_set(golden)
    pset = _capi.PuzzleSet([_capi.ParsedPuzzle(t) for t in texts], 0)
    eng = _capi.Engine(pset, None, 3, 1, _capi.OBS_U8)
    eng.set_option("search_batch_groups_per_cu", per_cu)
    try:
        b = SolutionTableBatch(eng, max_states_each=deep_puzzles.BATCH_CAP)
        try:
            status, summary, _ = _summaries(b)
            assert status.tolist() == [BUILT] * len(names)
            assert b.rows_needed == b.rows == sum(len(h.states) for h in hosts)
            for i, (k, h) in enumerate(zip(names, hosts)):
                c0 = -1 if h.summary[4] == INF else h.summary[4]
                assert tuple(summary[i]) == tuple(h.summary[:4]) + (c0,), k
                _assert_exact(b, i, h, k)
            for i, k in enumerate(deep_puzzles.BATCH_DEEP):
                assert tuple(summary[i])[:4] == deep_puzzles.EXPECT[k][:4], k
        finally:
            b.close()
    finally:
        eng.set_option("search_batch_groups_per_cu", 0)


def _host_layers(oz, limit):
    """One layer-synchronous breadth-first search that goes on past goal states: the number of states the start reaches
    (None beyond ``limit``) and, per depth 1, 2 ..., (states seen so far, whether the layer holds the first goal state), up
    to the first layer that ends beyond ``limit``."""
    is_goal = oz.py.is_goal_state
    s0 = oz.initial_state
    seen, layer, layers, solved = {s0}, [s0], [], is_goal(s0)
    while layer:
        nxt, found = [], False
        for s in layer:
            for a in range(4):
                n = oz.get_next_state(s, a)
                if n not in seen:
                    seen.add(n)
                    nxt.append(n)
                    found = found or is_goal(n)
        layers.append((len(seen), found and not solved))
        solved = solved or found
        if len(seen) > limit:
            return None, is_goal(s0), layers
        layer = nxt
    return len(seen), is_goal(s0), layers


def _host_verdict(start_is_goal, layers, cap):
    """pw_search_batch's (verdict, plan_len) from _host_layers: a goal state found in a layer decides, even when the store
    fills up inside it; otherwise more than ``cap`` states = unknown (tests/test_gpu_search.py's _host_bfs_verdict)."""
    if start_is_goal:
        return 1, 0
    for depth, (count, goal) in enumerate(layers, 1):
        if goal:
            return 1, depth
        if count > cap:
            return 2, -1
    return 0, -1


def test_the_three_batched_searches_agree_where_they_meet(golden):
    """pw_search_batch (K5b), pw_solve_batch (K13) and pw_push_solve_batch (K22) share one closed set (csrc/pw_batch_set.inc):
    one set through all three on one engine, at caps of 300 and 5 000 states.  Who exhausts, who solves and who passes the cap
    is worked out on the host first (breadth-first searches over the oracle, and the recorded summaries where there are any),
    so every branch below is known to be taken before anything is launched."""
    from oracle import c_oracle
    from pushworld_amd import _capi
    from pushworld_amd.search import PushSolutionTableBatch, SolutionTableBatch, search_batch

    keys = [k for k in golden.keys if k.startswith(("pytest:", "cpptest:"))] + [k for k in golden.keys if k.startswith("l0:")][::20]
    texts = [golden.text(k) for k in keys]
    oracles = [c_oracle.COraclePuzzle(t) for t in texts]
    fits = [golden.meta[k]["num_movables"] <= 8 and golden.meta[k]["width"] <= 16 and golden.meta[k]["height"] <= 16 for k in keys]
    searched = [_host_layers(oz, 5000) if f else (None, False, []) for oz, f in zip(oracles, fits)]
    totals = [t for t, _, _ in searched]
    for i, k in enumerate(keys):  # the recorded summaries: number of states and cost of the start
        if k in EXPECT and EXPECT[k][0] <= 5000:
            assert totals[i] == EXPECT[k][0], k
    host = {}
    for cap in (300, 5000):
        verdicts = [_host_verdict(g, layers, cap) if f else (3, -1) for (_, g, layers), f in zip(searched, fits)]
        builds = [f and t is not None and t <= cap for f, t in zip(fits, totals)]
        exhausted = [i for i, v in enumerate(verdicts) if v[0] == 0]
        solved = [i for i, v in enumerate(verdicts) if v[0] == 1 and builds[i]]
        assert all(builds[i] for i in exhausted)
        past_cap = [i for i, f in enumerate(fits) if f and not builds[i]]
        assert exhausted and solved and past_cap, cap
        assert any(totals[i] <= 1024 for i in exhausted + solved), cap  # inside the LDS set of all three
        host[cap] = verdicts, builds, exhausted, solved
    for i in host[5000][3]:
        if keys[i] in EXPECT:
            assert host[5000][0][i][1] == EXPECT[keys[i]][4], keys[i]
    # past the LDS set (2 048 states at half load): the closed set climbs to 2^16 slots, with and without reaching the cap
    assert any(b and totals[i] > 2048 for i, b in enumerate(host[5000][1]))
    assert any(f and t is None for f, t in zip(fits, totals))

    pset = _capi.PuzzleSet([_capi.ParsedPuzzle(t) for t in texts], 0)
    eng = _capi.Engine(pset, None, 3, 1, _capi.OBS_U8)
    both_dead = both_live = k22_past_lds = 0
    for cap in (300, 5000):
        verdicts, builds, exhausted, solved = host[cap]
        v5, len5, n5 = search_batch(eng, None, max_states=cap)
        k13 = SolutionTableBatch(eng, max_states_each=cap)
        k22 = PushSolutionTableBatch(eng, max_states_each=cap)
        try:
            s13, sum13 = k13.status.cpu().numpy(), k13.summary.cpu().numpy()
            s22, sum22 = k22.status.cpu().numpy(), k22.summary.cpu().numpy()
        finally:
            k13.close()
            k22.close()
        assert [(int(v), int(p)) for v, p in zip(v5, len5)] == verdicts, cap
        assert [s in (BUILT, SUMMARY_ONLY) for s in s13] == builds, cap
        assert [s == NOT_SEARCHED for s in s13] == [not f for f in fits] == [s == NOT_SEARCHED for s in s22], cap
        for i in exhausted:  # K5b exhausts, K13 builds: the same closed set, and no way to a goal state
            assert v5[i] == 0 and sum13[i, 0] == n5[i] == totals[i] and sum13[i, 4] == -1, (keys[i], cap)
        for i in solved:  # K5b's shortest plan is K13's cost of the start
            assert v5[i] == 1 and sum13[i, 4] == len5[i] >= 0 and sum13[i, 0] == totals[i], (keys[i], cap)
        for i in range(len(keys)):
            if builds[i] and s22[i] in (BUILT, SUMMARY_ONLY):  # solvable by steps = solvable by pushes
                assert (sum13[i, 4] == -1) == (sum22[i, 5] == -1) and sum13[i, 4] >= -1 and sum22[i, 5] >= -1, (keys[i], cap)
                assert sum22[i, 0] <= sum13[i, 0], (keys[i], cap)  # (a canonical state stands for states the steps reach)
                both_dead += sum22[i, 5] == -1
                both_live += sum22[i, 5] >= 0
        k22_past_lds += int(((s22 == TOO_MANY) | (sum22[:, 0] > 1024)).sum())
        assert (s22 == TOO_MANY).any() and ((s22 == BUILT) & (sum22[:, 0] <= 1024)).any(), cap
    assert both_dead > 0 and both_live > 0 and k22_past_lds > 0

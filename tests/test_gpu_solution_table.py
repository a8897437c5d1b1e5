"""Exact cost-to-go tables (pw_search_solve / pw_search_table_read / pw_search_table_query, search.SolutionTable,
VecPushWorld.solution_table / cost_to_go) against a host reference over the compiled oracle: the FIFO search of
tests/test_gpu_search.py::host_bfs extended to record the four successor indices of every state, predecessor lists built from
them, and a reverse breadth-first search from every goal state.  Every result is an integer: equality is exact."""
import ctypes
from collections import deque

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

INF = 0xFFFF
CAP = 60000

# case -> (states, goal states, dead ends, largest finite cost, cost of state 0)
EXPECT = {
    "pytest:trivial.pwp": (19, 6, 6, 5, 4),
    "pytest:trivial_obstacle.pwp": (507, 70, 165, 19, 10),
    "pytest:trivial_tool.pwp": (538, 68, 355, 18, 8),
    "pytest:pushing.pwp": (28, 28, 0, 0, 0),
    "pytest:transitive_pushing.pwp": (150, 50, 10, 10, 3),
    "l0:level0/base/train/level_0_base_train_0.pwp": (994, 100, 694, 12, 2),
    "l0:level0/all/train/level_0_all_train_3.pwp": (10659, 632, 8180, 23, 8),
    "rand:3": (5828, 769, 294, 16, 10),
    "rand:17": (7480, 7480, 0, 0, 0),
    "rand:42": (14, 14, 0, 0, 0),
}
CASES = list(EXPECT)
LOWEST_BIT = np.array([0, 0, 1, 0, 2, 0, 1, 0, 3, 0, 1, 0, 2, 0, 1, 0], dtype=np.uint8)  # of a 4-bit mask (0 for none)
QUERY_CASES = ["pytest:trivial_tool.pwp", "l0:level0/base/train/level_0_base_train_0.pwp", "rand:3"]


class HostTable:
    """The reference table of one puzzle; computed once per session and never changed."""

    def __init__(self, text):
        from oracle import c_oracle

        self.text = text
        self.oz = oz = c_oracle.COraclePuzzle(text)
        states, index, succ = [oz.initial_state], {oz.initial_state: 0}, []
        i = 0
        while i < len(states):  # FIFO order, actions 0..3: host_bfs's numbering
            row = []
            for a in range(4):
                n = oz.get_next_state(states[i], a)
                if n == states[i]:
                    row.append(i)
                    continue
                if n not in index:
                    assert len(states) < CAP
                    index[n] = len(states)
                    states.append(n)
                row.append(index[n])
            succ.append(row)
            i += 1
        total = len(states)
        preds = [[] for _ in range(total)]
        for i, row in enumerate(succ):
            for t in row:
                if t != i:
                    preds[t].append(i)
        cost = [INF] * total
        q = deque()
        for i, s in enumerate(states):
            if oz.py.is_goal_state(s):
                cost[i] = 0
                q.append(i)
        self.num_goals = len(q)
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
        self.summary = (total, self.num_goals, int((self.cost == INF).sum()), int(finite.max()) if finite.size else 0,
                        int(cost[0]))


_HOST = {}


def host_table(golden, key) -> HostTable:
    if key not in _HOST:
        _HOST[key] = HostTable(golden.text(key))
    return _HOST[key]


def _present(golden):
    keys = [k for k in CASES if k in golden.meta]
    assert len(keys) >= 8
    return keys


def _table(golden, key, keys="fingerprint", chunk=None, step_kernel=None, max_states=CAP + 8):
    from pushworld_amd.puzzle import PushWorldPuzzle
    from pushworld_amd.search import SolutionTable

    pz = PushWorldPuzzle(text=golden.text(key))
    pz._engine().set_option("search_keys", keys)
    if step_kernel is not None:
        pz._engine().set_option("step_kernel", step_kernel)
    return pz, SolutionTable(pz, max_states=max_states, chunk=chunk)


def test_host_reference_matches_the_recorded_summary(golden):
    """The reference itself: the figures of every case as they were recorded when the cases were chosen."""
    for key in _present(golden):
        assert host_table(golden, key).summary == EXPECT[key], key


@pytest.mark.parametrize("step_kernel", ["group", "lane"])
@pytest.mark.parametrize("chunk", [None, 7, 1000])
@pytest.mark.parametrize("keys", ["fingerprint", "exact"])
def test_table_equals_host_reference(golden, keys, chunk, step_kernel):
    """successors / costs / actions row by row, and the summary attributes, for both closed-set forms, one pass, many tiny
    passes (chunk 7, spaces up to 3 000 states) and 11 passes over the largest space (chunk 1000), with the successor pass
    on the lane-group and on the one-lane-per-parent expansion kernel."""
    ran = 0
    lane_cases = []  # cases whose successor pass really ran one lane per parent (it needs the puzzle's push tables)
    for key in _present(golden):
        want = host_table(golden, key)
        if chunk == 7 and len(want.states) > 3000:
            continue
        pz, tab = _table(golden, key, keys, chunk, step_kernel)
        try:
            tag = (key, keys, chunk, step_kernel)
            per = len(want.states) if chunk is None else chunk
            assert tab.solve_passes == -(-len(want.states) // per), tag
            assert tab.solve_lane_passes in (0, tab.solve_passes), tag
            if step_kernel == "group":
                assert tab.solve_lane_passes == 0, tag
            elif tab.solve_lane_passes:
                lane_cases.append(key)
            assert (tab.num_states, tab.num_goal_states, tab.num_dead_ends, tab.max_cost) == EXPECT[key][:4], tag
            assert tab.initial_cost == (None if EXPECT[key][4] == INF else EXPECT[key][4]), tag
            got = tab.states()
            assert (got == np.array(want.states, dtype=np.int64).reshape(got.shape)).all(), tag
            succ, cost, acts = tab.successors().cpu().numpy(), tab.costs().cpu().numpy(), tab.actions().cpu().numpy()
            assert succ.dtype == np.int32 and cost.dtype == np.uint16 and acts.dtype == np.uint8
            assert succ.shape == want.succ.shape and (succ == want.succ).all(), tag
            assert (cost == want.cost).all(), tag
            assert (acts == want.acts).all(), tag
            if len(want.states) > 5:  # a range in the middle
                assert (tab.successors(3, 2).cpu().numpy() == want.succ[3:5]).all()
                assert (tab.costs(3, 2).cpu().numpy() == want.cost[3:5]).all()
                assert (tab.actions(3, 2).cpu().numpy() == want.acts[3:5]).all()
            with pytest.raises(ValueError):
                tab.costs(1, len(want.states))
        finally:
            tab.close()
        ran += 1
    assert ran >= (5 if chunk == 7 else 8)
    print("one lane per parent:", lane_cases)
    if step_kernel == "lane":
        assert lane_cases, "no case ran the one-lane-per-parent successor pass: the parametrisation repeats 'group'"


def test_optimal_plans(golden):
    """optimal_plan() from state 0 is a valid plan of length initial_cost; from 50 random solvable states it reaches a goal
    state at exactly step cost[i] and not before; None for dead ends."""
    ran = 0
    for key in _present(golden):
        want = host_table(golden, key)
        pz, tab = _table(golden, key)
        try:
            if tab.initial_cost is not None:
                plan = tab.optimal_plan()
                assert len(plan) == tab.initial_cost == EXPECT[key][4], key
                assert pz.is_valid_plan(plan), key
            states = tab.states()
            rng = np.random.default_rng(1234)
            solvable = np.flatnonzero(want.cost != INF)
            for i in rng.choice(solvable, size=min(50, solvable.size), replace=False):
                plan = tab.optimal_plan(int(i))
                assert len(plan) == want.cost[i], (key, i)
                s = tuple((int(x), int(y)) for x, y in states[i])
                for a in plan:
                    assert not want.oz.py.is_goal_state(s), (key, i)
                    s = want.oz.get_next_state(s, a)
                assert want.oz.py.is_goal_state(s), (key, i)
            dead = np.flatnonzero(want.cost == INF)
            for i in dead[:3]:
                assert tab.optimal_plan(int(i)) is None
            with pytest.raises(ValueError):
                tab.optimal_plan(len(want.states))
        finally:
            tab.close()
        ran += 1
    assert ran >= 8


def _rows(states, npad):
    pos = np.zeros((len(states), npad, 2), dtype=np.int8)
    for i, s in enumerate(states):
        pos[i, :len(s)] = np.array(s, dtype=np.int64).astype(np.int8)
    return pos


@pytest.mark.parametrize("keys", ["fingerprint", "exact"])
@pytest.mark.parametrize("key", QUERY_CASES)
def test_query(golden, key, keys):
    """Every reachable state (shuffled), 200 in-grid states outside the table, 16 states with a coordinate outside the grid,
    32 masked items and 32 items of another puzzle in one batch; then n = 1 and n = 65."""
    if key not in golden.meta:
        pytest.skip("case missing from the golden set")
    want = host_table(golden, key)
    pz, tab = _table(golden, key, keys)
    try:
        W, H = pz.dimensions
        N = pz.num_movables
        rng = np.random.default_rng(99)
        order = rng.permutation(len(want.states))
        inside = [want.states[i] for i in order]
        outside = []
        while len(outside) < 200:
            s = tuple((int(rng.integers(0, W)), int(rng.integers(0, H))) for _ in range(N))
            if s not in want.index:
                outside.append(s)
        off_grid = []
        bad_x, bad_y = [-1, W, -128, 127, W + 1, 100, -2, W], [-1, H, -128, 127, H + 1, 100, -2, H]
        for k in range(16):  # one coordinate of one movable of a reachable state moved outside the grid
            s = [list(p) for p in want.states[int(order[k])]]
            s[k % N][k % 2] = (bad_y if k % 2 else bad_x)[k // 2]
            off_grid.append(tuple(tuple(p) for p in s))
        masked = [want.states[int(i)] for i in order[:32]]
        foreign = [want.states[int(i)] for i in order[-32:]]
        states = inside + outside + off_grid + masked + foreign
        n_in, n = len(inside), len(states)
        ids = np.full(n, tab.puzzle_index, dtype=np.int32)
        ids[-32:] = tab.puzzle_index + 5
        mask = np.ones(n, dtype=np.uint8)
        mask[-64:-32] = 0
        exp_index = np.full(n, -1, dtype=np.int32)
        exp_cost = np.full(n, -2, dtype=np.int32)
        exp_acts = np.zeros(n, dtype=np.uint8)
        exp_index[:n_in] = order
        c = want.cost[order].astype(np.int32)
        exp_cost[:n_in] = np.where(c == INF, -1, c)
        exp_acts[:n_in] = want.acts[order]
        exp_index[-64:], exp_cost[-64:], exp_acts[-64:] = -77, -99, 0xAB  # untouched: the sentinels below
        dev = tab.device
        pos = torch.as_tensor(_rows(states, tab.npad)).to(dev)
        ids_d, mask_d = torch.as_tensor(ids).to(dev), torch.as_tensor(mask).to(dev)
        out = (torch.full((n,), -77, dtype=torch.int32, device=dev), torch.full((n,), -99, dtype=torch.int32, device=dev),
               torch.full((n,), 0xAB, dtype=torch.uint8, device=dev))
        got = tab.query(ids_d, pos, mask=mask_d, out=out)
        assert all(g is o for g, o in zip(got, out))
        assert (got[0].cpu().numpy() == exp_index).all()
        assert (got[1].cpu().numpy() == exp_cost).all()
        assert (got[2].cpu().numpy() == exp_acts).all()
        # without `out` the untouched items are -1 / -2 / 0; a bool mask works too
        fresh = tab.query(ids_d, pos, mask=mask_d.bool())
        assert (fresh[0].cpu().numpy()[-64:] == -1).all() and (fresh[1].cpu().numpy()[-64:] == -2).all()
        assert (fresh[2].cpu().numpy()[-64:] == 0).all()
        assert (fresh[0].cpu().numpy()[:-64] == exp_index[:-64]).all()
        # a single item, and a partial wavefront; no puzzle_id and no mask: every item is the table's
        for lo, cnt in ((n_in - 1, 1), (n_in - 30, 65)):
            part = tab.query(None, pos[lo:lo + cnt].contiguous())
            assert (part[0].cpu().numpy() == exp_index[lo:lo + cnt]).all()
            assert (part[1].cpu().numpy() == exp_cost[lo:lo + cnt]).all()
            assert (part[2].cpu().numpy() == exp_acts[lo:lo + cnt]).all()
    finally:
        tab.close()


def test_table_is_discarded_and_refused(golden):
    """No table before the search is exhausted, none after begin(): the entry points say so with PW_EINVAL."""
    from pushworld_amd import _capi
    from pushworld_amd.puzzle import PushWorldPuzzle
    from pushworld_amd.search import BreadthFirstSearch, SolutionTable

    pz, tab = _table(golden, "pytest:trivial_tool.pwp")
    try:
        dev, lib = tab.device, _capi.lib
        pos = torch.as_tensor(_rows([pz.initial_state], tab.npad)).to(dev)
        out = torch.full((1,), -5, dtype=torch.int32, device=dev)
        args = (None, _capi._ptr(pos), tab.npad, None, 1, _capi._ptr(out), None, None, None)
        assert lib.pw_search_table_query(tab.search.handle, *args) == _capi.PW_OK
        assert out.cpu().tolist() == [0]  # NULL puzzle_id, NULL mask: the initial state is row 0
        tab.search.begin()
        assert lib.pw_search_table_query(tab.search.handle, *args) == _capi.PW_EINVAL
        assert "pw_search_table_query" in _capi.last_error() and "no table" in _capi.last_error()
        assert lib.pw_search_table_read(tab.search.handle, 0, 1, None, None, None, None) == _capi.PW_EINVAL
        assert "pw_search_table_read" in _capi.last_error()
        info = (ctypes.c_int64 * 4)()
        assert lib.pw_search_solve(tab.search.handle, info, None) == _capi.PW_EINVAL
        assert "not exhausted" in _capi.last_error()
    finally:
        tab.close()
    # a width-limited search has no table; a space beyond max_states raises as the search does
    bfs = BreadthFirstSearch(pz, max_states=4096, novelty_width=1)
    try:
        bfs.begin()
        while not bfs.exhausted:
            bfs.expand()
        assert _capi.lib.pw_search_solve(bfs.handle, (ctypes.c_int64 * 4)(), None) == _capi.PW_EINVAL
        assert "novelty_width" in _capi.last_error()
    finally:
        bfs.close()
    with pytest.raises(ValueError, match="store is full"):
        SolutionTable(PushWorldPuzzle(text=golden.text("pytest:trivial_tool.pwp")), max_states=100)


def test_mixed_batch_cost_to_go(golden):
    """192 environments over three puzzles, tables for the first two: after reset and after each of 30 random steps the
    looked-up rows are the host's; then the lowest optimal action solves every environment in exactly initial_cost steps."""
    from pushworld_amd.puzzle import PushWorldPuzzle
    from pushworld_amd.vec_env import VecPushWorld

    keys = ["pytest:trivial_tool.pwp", "l0:level0/base/train/level_0_base_train_0.pwp", "pytest:transitive_pushing.pwp"]
    for k in keys:
        if k not in golden.meta:
            pytest.skip("case missing from the golden set")
    hosts = [host_table(golden, k) for k in keys]
    puzzles = [PushWorldPuzzle(text=golden.text(k)) for k in keys]
    B = 192
    ids = np.arange(B) % 3
    vec = VecPushWorld(puzzles, B, puzzle_ids=ids, observation=None, max_steps=None)
    tables = [vec.solution_table(0, max_states=CAP), vec.solution_table(1)]
    try:
        assert [t.initial_cost for t in tables] == [EXPECT[keys[0]][4], EXPECT[keys[1]][4]]

        def check():
            index, cost, acts = (t.cpu().numpy() for t in vec.cost_to_go(tables))
            states = vec.states()
            for i in range(B):
                pid = int(ids[i])
                if pid == 2:
                    assert (index[i], cost[i], acts[i]) == (-1, -2, 0), i
                    continue
                h = hosts[pid]
                s = tuple((int(x), int(y)) for x, y in states[i][:puzzles[pid].num_movables])
                j = h.index[s]
                c = int(h.cost[j])
                assert (index[i], cost[i], acts[i]) == (j, -1 if c == INF else c, h.acts[j]), (i, pid)
            return cost, acts

        vec.reset()
        check()
        rng = np.random.default_rng(7)
        for _ in range(30):
            vec.step(torch.as_tensor(rng.integers(0, 4, size=B).astype(np.uint8), device=vec.device))
            check()

        vec.reset()
        want_len = np.array([tables[0].initial_cost, tables[1].initial_cost, -1])[ids]
        done_at = np.full(B, -1)
        for t in range(1, int(want_len.max()) + 1):
            cost, acts = check()
            live = (ids != 2) & (done_at < 0)
            assert (cost[live] >= 1).all()  # never a dead end (-1) on the way, never outside the table
            opt = acts & 15
            assert (opt[live] != 0).all()
            action = LOWEST_BIT[opt]
            _, reward, terminated, _ = vec.step(torch.as_tensor(action, device=vec.device))
            reward, terminated = reward.cpu().numpy(), terminated.cpu().numpy()
            newly = live & (terminated != 0)
            assert (reward[newly] == 10.0).all()
            done_at[newly] = t
            assert (terminated[live & ~newly] == 0).all()
        assert (done_at[ids != 2] == want_len[ids != 2]).all()
    finally:
        for t in tables:
            t.close()


# ---- deep spaces (tests/deep_puzzles.py): the sweep loop of pw_search_solve beyond two batches of 16 sweeps ---------------------
# largest cost 15 / 16 / 17 / 31 / 32 / 33: the last settling sweep is the last of a batch, the first of the next one, and one
# further; 253 / 254: the cost_start tables of 256 and 257 words; 1950 / 1949: 122 batches of sweeps
DEEP = (["corridor %d" % L for L in (17, 18, 19, 33, 34, 35)] +
        ["serpentine 30x29 max 253", "serpentine 30x29 max 254", "serpentine 62x61", "serpentine 62x61 overshoot"])


@pytest.mark.parametrize("name", DEEP)
def test_deep_table_equals_host_reference(name):
    """successors / costs / actions row by row and the summary, max_cost included, on path puzzles whose largest cost is 15 ..
    1950; optimal_plan(0) replayed on the oracle reaches a goal state at exactly step cost[0] and not before."""
    import deep_puzzles
    from pushworld_amd.puzzle import PushWorldPuzzle
    from pushworld_amd.search import SolutionTable

    want = deep_puzzles.host_table(name)
    assert want.summary == deep_puzzles.EXPECT[name]
    pz = PushWorldPuzzle(text=deep_puzzles.text(name))
    tab = SolutionTable(pz, max_states=CAP + 8)
    try:
        assert (tab.num_states, tab.num_goal_states, tab.num_dead_ends, tab.max_cost, tab.initial_cost) == want.summary
        got = tab.states()
        assert (got == np.array(want.states, dtype=np.int64).reshape(got.shape)).all()
        succ, cost, acts = tab.successors().cpu().numpy(), tab.costs().cpu().numpy(), tab.actions().cpu().numpy()
        assert succ.shape == want.succ.shape and (succ == want.succ).all()
        assert (cost == want.cost).all()
        assert (acts == want.acts).all()
        plan = tab.optimal_plan(0)
        assert len(plan) == int(want.cost[0]) == want.summary[4]
        assert pz.is_valid_plan(plan)
        s = want.states[0]
        for a in plan:
            assert not want.oz.py.is_goal_state(s)
            s = want.oz.get_next_state(s, a)
        assert want.oz.py.is_goal_state(s)
    finally:
        tab.close()

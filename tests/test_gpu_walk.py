"""Walk regions and push moves on the device (pw_walk_regions / pw_walk_pushes, search.walk_regions, VecPushWorld.push_moves,
search.PushSearch) against the restatement of tests/walk_restatement.py over the C oracle's step function.  Every
listed state is compared field by field: region_size, canon, the whole walk map, offset, and every row's from / action / walk /
moved / goal / next_pos with its zero padding."""
import os

import numpy as np
import pytest
import torch

import deep_puzzles
import rgd_puzzles
import walk_restatement as WR
from oracle import c_oracle
from pushworld_amd.puzzle import PushWorldPuzzle
from pushworld_amd.search import REPLAY_VALID, WALK_OUTSIDE, BreadthFirstSearch, PushSearch, replay_plans, walk_regions
from pushworld_amd.vec_env import VecPushWorld
from test_walk_host import HAND

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "pushworld_amd", "data")
REF = os.path.join(ROOT, "tests", "puzzles", "ref_python")
TABLES = ["all", "big", "none"]  # the engine's three table forms: every puzzle, some, none


def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def _level(level, name):
    return _read(DATA, "puzzles", f"level{level}", name + ".pwp")


def _human_plan(level, name):
    for line in _read(DATA, "solutions", f"level{level}", name + ".yaml").splitlines():
        if line.startswith("plan:"):
            return ["LRUD".index(c) for c in line.split(":", 1)[1].strip()]
    raise ValueError(name)


# a bar of 9 x 1 cells that the agent can push down onto its goal: a movable beyond 8 x 8, so under step_tables="big" this
# puzzle gets overlap tables and its neighbours in a set do not (the kernels' "some puzzles" form)
WIDE = "A . . . . . . . . .\n" + " ".join(["M0"] * 9) + " .\n" + ". " * 9 + ".\n" + " ".join(["G0"] * 9) + " .\n"
SEALED = "A W M0 . G0\n"  # the agent sealed in one cell: a region of one position, no push


class Batch:
    """A puzzle set on the device, its oracles, and the restatement's regions of the states asked for (computed once each)."""

    def __init__(self, texts, tables="all"):
        self.texts = list(texts)
        self.cps = [c_oracle.COraclePuzzle(t) for t in self.texts]
        self.vec = VecPushWorld([PushWorldPuzzle(text=t) for t in self.texts], len(self.texts), observation=None,
                                max_steps=None, engine_options={"step_tables": tables})
        self.dev, self.npad = self.vec.device, self.vec.num_objects_padded
        self.map_h = max(cp.height for cp in self.cps)
        self.map_w = max(cp.width for cp in self.cps)
        self._regions = {}

    def region(self, pid, state):
        key = (pid, tuple(map(tuple, state)))
        if key not in self._regions:
            self._regions[key] = WR.region(self.cps[pid], key[1])
        return self._regions[key]

    def pos(self, states):
        arr = np.zeros((len(states), self.npad, 2), np.int8)
        for i, s in enumerate(states):
            arr[i, :len(s)] = np.asarray(s, np.int8)
        return torch.as_tensor(arr, device=self.dev)

    def check(self, ids, states, mask=None, skipped=(), pos=None):
        """Runs both entry points over (ids, states) and compares every field of every item; `skipped`: the items that must
        come back with region_size -1 and no rows.  Returns (WalkRegions, PushMoves, expected rows per item)."""
        n = len(ids)
        t_ids = torch.as_tensor(np.asarray(ids, np.int32), device=self.dev)
        t_pos = self.pos(states) if pos is None else pos
        t_mask = None if mask is None else torch.as_tensor(np.asarray(mask, np.uint8), device=self.dev)
        reg = walk_regions(self.vec, t_ids, t_pos, t_mask, maps=True)
        rows = reg.pushes()
        size, canon, offset, wmap = (x.cpu().numpy() for x in (reg.region_size, reg.canon, reg.offset, reg.walk_map))
        assert wmap.shape == (n, self.map_h, self.map_w) and wmap.dtype == np.uint16
        item, frm, act, walk, moved, goal, nxt = (x.cpu().numpy() for x in (rows.item, rows.frm, rows.action, rows.walk,
                                                                          rows.moved, rows.goal, rows.next_pos))
        assert int(rows.dropped.item()) == 0 and rows.num_rows == offset[n] == reg.num_pushes
        want_rows, at = [], 0
        for i in range(n):
            assert offset[i] == at, i
            if i in skipped:
                assert size[i] == -1 and (canon[i] == 0).all() and (wmap[i] == WALK_OUTSIDE).all(), i
                want_rows.append([])
                continue
            r = self.region(ids[i], states[i])
            assert size[i] == len(r.dist) and tuple(canon[i]) == r.canon, (i, ids[i])
            want = np.full((self.map_h, self.map_w), WALK_OUTSIDE, np.uint16)
            for (x, y), d in r.dist.items():
                want[y, x] = d | (r.parent.get((x, y), 0) << 12)
            assert (wmap[i] == want).all(), (i, ids[i])
            k = len(r.pushes)
            assert (item[at:at + k] == i).all()
            for j, pm in enumerate(r.pushes):
                got = (tuple(frm[at + j]), act[at + j], walk[at + j], int(moved[at + j]) & 0xFFFFFFFF, goal[at + j])
                assert got == (pm.frm, pm.action, pm.walk, pm.moved, int(pm.goal)), (i, ids[i], j)
                m = len(pm.next_state)
                assert (nxt[at + j, :m] == np.asarray(pm.next_state, np.int8)).all() and (nxt[at + j, m:] == 0).all(), (i, j)
            want_rows.append(r.pushes)
            at += k
        assert offset[n] == at
        return reg, rows, want_rows


def _corner_texts(npad):
    texts = [_read(REF, k + ".pwp") for k in ("trivial", "trivial_tool", "transitive_pushing", "trivial_obstacle", "pushing",
                                              "agent_movement")] + [HAND, WIDE]
    extra = {4: None, 8: 4, 16: 10, 32: deep_puzzles.POCKETS_EXTRA}[npad]
    return texts + ([deep_puzzles.pockets(extra)] if extra else [])


@pytest.mark.parametrize("tables", TABLES)
@pytest.mark.parametrize("npad", [4, 8, 16, 32])
def test_dynamics_corners(npad, tables):
    texts = [t for t in _corner_texts(npad) if npad > 4 or c_oracle.COraclePuzzle(t).num_movables <= 4]
    b = Batch(texts, tables)
    assert b.npad == npad and any(cp.py.has_agent_walls for cp in b.cps)
    if npad == 32:
        assert b.cps[-1].num_movables == 17
    assert max(max(sz) for sz in b.cps[texts.index(WIDE)].py.sizes) == 9
    with_tables = b.vec.engine.get_option("step_table_puzzles")
    if tables == "big":  # WIDE alone has a movable beyond 8 x 8: tables for some puzzles, not for all
        assert 0 < with_tables < len(texts)
    else:
        assert with_tables == (len(texts) if tables == "all" else 0)
    # the initial states, and the successors of their push moves (states the boxes have left their places in)
    ids = list(range(len(texts)))
    states = [cp.initial_state for cp in b.cps]
    _, _, want = b.check(ids, states)
    assert sum(len(w) for w in want) > 0
    ids2 = [i for i, w in zip(ids, want) for pm in w if WR.in_grid(b.cps[i], pm.next_state)]
    states2 = [pm.next_state for i, w in zip(ids, want) for pm in w if WR.in_grid(b.cps[i], pm.next_state)]
    b.check(ids2, states2)
    # NULL pos: the initial states
    reg = walk_regions(b.vec, torch.arange(len(texts), dtype=torch.int32, device=b.dev))
    assert reg.walk_map is None
    assert reg.region_size.cpu().tolist() == [len(b.region(i, s).dist) for i, s in zip(ids, states)]


def test_argument_checks_that_need_an_engine():
    """npad below the set's largest number of movables, map_h / map_w below its largest dimensions: PW_EINVAL before any launch."""
    from pushworld_amd import _capi

    b = Batch(_corner_texts(32), "all")
    eng, n = b.vec.engine, len(b.texts)
    assert b.npad == 32 and b.vec.pset.max_movables == 17
    ids = torch.arange(n, dtype=torch.int32, device=b.dev)
    size = torch.full((n,), -9, dtype=torch.int32, device=b.dev)
    offset = torch.full((n + 1,), -9, dtype=torch.int64, device=b.dev)
    wmap = torch.full((n, b.map_h, b.map_w), 7, dtype=torch.uint16, device=b.dev)
    ptr = _capi._ptr

    def regions(npad, walk_map=None, map_h=0, map_w=0):
        return _capi.lib.pw_walk_regions(eng.handle, ptr(ids), None, npad, None, n, ptr(size), None, ptr(offset), walk_map,
                                         map_h, map_w, None)

    def pushes(npad):
        return _capi.lib.pw_walk_pushes(eng.handle, ptr(ids), None, npad, None, n, ptr(offset), 0, None, None, None, None, None,
                                        None, None, None, None)

    for npad in (4, 8, 16):
        for call, name in ((regions, "pw_walk_regions"), (pushes, "pw_walk_pushes")):
            assert call(npad) == _capi.PW_EINVAL
            msg = _capi.last_error()
            assert name in msg and "npad" in msg and "movables" in msg
    for (mh, mw), word in (((b.map_h - 1, b.map_w), "map_h"), ((b.map_h, b.map_w - 1), "map_w"), ((1, 64), "map_h"),
                           ((64, 1), "map_w")):
        assert regions(32, ptr(wmap), mh, mw) == _capi.PW_EINVAL
        msg = _capi.last_error()
        assert "pw_walk_regions" in msg and word in msg and "largest" in msg
    torch.cuda.synchronize()
    assert bool((size == -9).all()) and bool((offset == -9).all()) and bool((wmap == 7).all())  # nothing was launched
    assert regions(32, ptr(wmap), b.map_h, b.map_w) == _capi.PW_OK  # the exact dimensions pass
    assert size.cpu().tolist() == [len(b.region(i, cp.initial_state).dist) for i, cp in enumerate(b.cps)]


BENCH = [(1, "2 Obstacle"), (1, "Pulling"), (1, "Irrelevant Obstacles"), (2, "Clean Sweep")]


def _bench_states(b):
    """(ids, states): the initial state and every 10th state of the human plan of every puzzle of BENCH."""
    ids, states = [], []
    for pid, (level, name) in enumerate(BENCH):
        s = b.cps[pid].initial_state
        trace = [s]
        for a in _human_plan(level, name):
            s = b.cps[pid].get_next_state(s, a)
            trace.append(s)
        for s in trace[::10]:
            ids.append(pid)
            states.append(s)
    return ids, states


_BENCH = {}


def _bench(tables):
    if tables not in _BENCH:
        _BENCH[tables] = Batch([_level(lv, name) for lv, name in BENCH], tables)
    return _BENCH[tables]


@pytest.mark.parametrize("tables", TABLES)
def test_benchmark_states_one_mixed_batch(tables):
    b = _bench(tables)
    assert b.cps[0].py.has_agent_walls and (b.cps[1].width, b.cps[1].height) in ((42, 51), (44, 53), (51, 42), (53, 44))
    assert b.cps[2].num_movables >= 9 and b.cps[3].num_movables == 19 and b.npad == 32
    with_tables = b.vec.engine.get_option("step_table_puzzles")
    if tables == "big":  # `Pulling` has movables of 8 x 11 and 10 x 11 cells, the others none beyond 8 x 8
        assert 0 < with_tables < len(BENCH)
    else:
        assert with_tables == (len(BENCH) if tables == "all" else 0)
    ids, states = _bench_states(b)
    n0 = len(ids)
    mask = [1] * n0
    skipped = set()
    for k in (3, n0 // 2):  # masked items
        mask[k] = 0
        skipped.add(k)
    for bad_id in (-1, len(BENCH), 1 << 20):  # ids outside the set
        ids.append(bad_id)
        states.append(states[0])
        mask.append(1)
        skipped.add(len(ids) - 1)
    # a movable outside its grid: the last movable of `2 Obstacle` one column beyond the border
    out = list(b.cps[0].initial_state)
    out[-1] = (b.cps[0].width, out[-1][1])
    ids.append(0)
    states.append(tuple(out))
    mask.append(1)
    skipped.add(len(ids) - 1)
    _, rows, want = b.check(ids, states, mask, skipped)
    assert rows.num_rows > 100 and max(len(w) for w in want) > 4


_DEEP = {}


def _deep():
    if not _DEEP:
        _DEEP["b"] = Batch([deep_puzzles.serpentine(62, 61), rgd_puzzles.room(62, 61), SEALED], "all")
    return _DEEP["b"]


def test_depth_and_size():
    b = _deep()
    assert (b.map_h, b.map_w) == (63, 64)
    states = [cp.initial_state for cp in b.cps]
    reg, rows, want = b.check([0, 1, 2], states)
    size = reg.region_size.cpu().tolist()
    serp = b.region(0, states[0])
    assert size[0] == len(serp.dist) and 1940 <= size[0] <= 1960 and max(serp.dist.values()) > 1900  # the 12-bit field
    assert size[1] == 62 * 61 - 1 or size[1] == 62 * 61  # the open room: every free cell of the largest board
    assert size[2] == 1 and want[2] == [] and len(want[0]) == 1 and want[0][0].walk > 1900 and len(want[1]) >= 2


def _thousand(b, ids, states, seed):
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, len(ids), size=1000)
    return [ids[k] for k in pick], [states[k] for k in pick]


def test_ragged_emit_with_cap():
    b = _bench("all")
    ids0, states0 = _bench_states(b)
    ids, states = _thousand(b, ids0, states0, 5)
    t_ids = torch.as_tensor(np.asarray(ids, np.int32), device=b.dev)
    t_pos = b.pos(states)
    reg = walk_regions(b.vec, t_ids, t_pos)
    counts = [len(b.region(i, s).pushes) for i, s in zip(ids, states)]
    total = sum(counts)
    assert reg.num_pushes == total and total > 2000
    assert (reg.offset.cpu().numpy() == np.concatenate([[0], np.cumsum(counts)])).all()
    full = reg.pushes()
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
    b.vec.engine.walk_pushes(t_ids, t_pos, None, reg.offset, cap, item, frm, act, walk, moved, goal, nxt, dropped)
    assert int(dropped.item()) == total - cap
    for got, want, fill in ((item, full.item, -7), (frm, full.frm, -7), (act, full.action, 77), (walk, full.walk, -7),
                            (moved, full.moved, -7), (goal, full.goal, 77), (nxt, full.next_pos, -7)):
        assert torch.equal(got[:cap], want[:cap]) and bool((got[cap:] == fill).all())
    # the full rows are the restatement's
    at = 0
    fi, fa, fw = full.item.cpu().numpy(), full.action.cpu().numpy(), full.walk.cpu().numpy()
    for i, (pid, s) in enumerate(zip(ids, states)):
        for pm in b.region(pid, s).pushes:
            assert (fi[at], fa[at], fw[at]) == (i, pm.action, pm.walk)
            at += 1
    # every output NULL but row_item
    only = torch.full((total,), -7, dtype=torch.int32, device=b.dev)
    b.vec.engine.walk_pushes(t_ids, t_pos, None, reg.offset, total, item=only)
    assert torch.equal(only, full.item)


def test_path_replays_through_plan_states():
    b = _bench("all")
    eng = b.vec.engine
    ids, states = _bench_states(b)
    pick = [k for k in range(len(ids)) if ids[k] in (0, 1)][::2]
    reg = walk_regions(b.vec, torch.as_tensor(np.asarray([ids[k] for k in pick], np.int32), device=b.dev),
                       b.pos([states[k] for k in pick]), maps=True)
    checked = 0
    for i, k in enumerate(pick):
        r = b.region(ids[k], states[k])
        far = sorted(r.dist, key=lambda q: (-r.dist[q], q))[:3] + [states[k][0]]
        for q in far:
            acts = reg.path(i, q)
            assert len(acts) == r.dist[q] and acts == WR.path(r, q)
            start = np.ascontiguousarray(np.asarray(states[k], np.int8))
            got, _ = eng.plan_states(ids[k], bytes(acts), start=start)
            assert tuple(got[-1, 0]) == q and (got[:, 1:] == start[None, 1:]).all()
            checked += 1
        outside = next((x, y) for y in range(b.cps[ids[k]].height) for x in range(b.cps[ids[k]].width) if (x, y) not in r.dist)
        with pytest.raises(ValueError, match="not in the walk region"):
            reg.path(i, outside)
    assert checked >= 12
    with pytest.raises(ValueError, match="not requested"):
        walk_regions(b.vec, torch.zeros(1, dtype=torch.int32, device=b.dev)).path(0, (1, 1))


def test_vec_push_moves_after_random_steps():
    names = sorted(f for f in os.listdir(os.path.join(DATA, "puzzles", "level1")) if f.endswith(".pwp"))[:32]
    texts = [_read(DATA, "puzzles", "level1", f) for f in names]
    cps = [c_oracle.COraclePuzzle(t) for t in texts]
    B = 256
    vec = VecPushWorld([PushWorldPuzzle(text=t) for t in texts], B, puzzle_ids=[i % len(texts) for i in range(B)],
                       observation=None, max_steps=None)
    vec.reset()
    gen = torch.Generator().manual_seed(11)
    for _ in range(20):
        vec.step(torch.randint(0, 4, (B,), generator=gen, dtype=torch.uint8).to(vec.device))
    pos = vec.states()
    ids = vec.puzzle_id.cpu().tolist()
    reg = vec.walk_regions(maps=True)
    rows = vec.push_moves()
    size, canon, offset = reg.region_size.cpu().numpy(), reg.canon.cpu().numpy(), reg.offset.cpu().numpy()
    item, frm, act, walk, moved, goal, nxt = (x.cpu().numpy() for x in (rows.item, rows.frm, rows.action, rows.walk, rows.moved,
                                                                      rows.goal, rows.next_pos))
    at = 0
    for i in range(B):
        cp = cps[ids[i]]
        s = tuple(tuple(int(v) for v in xy) for xy in pos[i, :cp.num_movables])
        r = WR.region(cp, s)
        assert size[i] == len(r.dist) and tuple(canon[i]) == r.canon and offset[i] == at
        for pm in r.pushes:
            assert (item[at], tuple(frm[at]), act[at], walk[at], int(moved[at]) & 0xFFFFFFFF, goal[at]) == (i, pm.frm, pm.action, pm.walk,
                                                                                         pm.moved, int(pm.goal))
            assert (nxt[at, :cp.num_movables] == np.asarray(pm.next_state, np.int8)).all() and (nxt[at, cp.num_movables:] == 0).all()
            at += 1
    assert offset[B] == at == rows.num_rows and at > B


def _level0(member):
    import zipfile

    with zipfile.ZipFile(os.path.join(DATA, "puzzles", "level0.zip")) as z:
        return z.read(member).decode()


SEARCH_CASES = {
    "Single Obstacle": lambda: _level(1, "Single Obstacle"),
    "Two Goals": lambda: _level(1, "Two Goals"),
    "2 Obstacle": lambda: _level(1, "2 Obstacle"),
    "level_0_walls_train_1732": lambda: _level0("level0/walls/train/level_0_walls_train_1732.pwp"),
}


def _pushing_steps(cp, plan):
    s, count = cp.initial_state, 0
    for a in plan:
        s, moved = cp.get_next_state_moved(s, a)
        count += len(moved) > 1
    return count


@pytest.mark.parametrize("name", list(SEARCH_CASES))
def test_push_search(name):
    text = SEARCH_CASES[name]()
    cp = c_oracle.COraclePuzzle(text)
    want = WR.push_search(cp)
    pz = PushWorldPuzzle(text=text)
    ps = PushSearch(pz)
    plan = ps.solve()
    assert plan == want.plan
    assert (ps.layer_states, ps.num_states, ps.pushes) == (want.layer_states, want.num_states, want.pushes)
    assert (ps.push_rows, ps.largest_region) == (want.push_rows, want.largest_region)
    assert pz.is_valid_plan(plan)
    assert _pushing_steps(cp, plan) == ps.pushes
    eng = pz._engine()
    plans = torch.as_tensor(np.asarray([plan], np.uint8), device=eng.device)
    out = replay_plans(eng, torch.zeros(1, dtype=torch.int32, device=eng.device), plans,
                       torch.as_tensor([len(plan)], dtype=torch.int32, device=eng.device), rows=False)
    assert out.verdict.cpu().tolist() == [REPLAY_VALID]
    # no plan has fewer steps that push: the shortest one move by move among them
    assert ps.pushes <= _pushing_steps(cp, BreadthFirstSearch(pz, max_states=1 << 16).solve())
    # a bound on the pushes below the plan's: None
    assert PushSearch(pz).solve(max_pushes=want.pushes - 1) is None


def test_push_search_exhausts_the_space():
    text = SEARCH_CASES["level_0_walls_train_1732"]()
    cp = c_oracle.COraclePuzzle(text)
    want = WR.push_search(cp, stop_at_goal=False)
    assert want.num_states == 380
    ps = PushSearch(PushWorldPuzzle(text=text))
    assert ps.solve(max_pushes=1 << 30, stop_at_goal=False) is None
    assert (ps.layer_states, ps.num_states, ps.pushes) == (want.layer_states, 380, None)
    assert (ps.push_rows, ps.largest_region) == (want.push_rows, want.largest_region)
    with pytest.raises(ValueError, match="max_states"):
        PushSearch(PushWorldPuzzle(text=text), max_states=100).solve(stop_at_goal=False)


def test_push_search_goal_start_and_no_solution():
    cp = c_oracle.COraclePuzzle(HAND)
    m0 = cp.py.names.index("m0")
    solved = tuple((4, 2) if k == m0 else xy for k, xy in enumerate(cp.initial_state))
    ps = PushSearch(PushWorldPuzzle(text=HAND))
    assert ps.solve(start=solved) == [] and ps.pushes == 0
    for outside in ((cp.width, 2), (-1, 2), (300, 2)):  # a goal start is checked like any other
        with pytest.raises(ValueError, match="outside the grid"):
            ps.solve(start=(outside,) + solved[1:])
    assert ps.solve() == [1] and (ps.pushes, ps.layer_states, ps.num_states) == (1, [], 3)
    # the box can only be pushed away from its goal: exhausted without one
    text = "G0 . A . M0 . .\n"
    want = WR.push_search(c_oracle.COraclePuzzle(text))
    assert want.plan is None
    ps = PushSearch(PushWorldPuzzle(text=text))
    assert ps.solve() is None
    assert (ps.layer_states, ps.num_states, ps.pushes) == (want.layer_states, want.num_states, None)
    assert want.push_rows == ps.push_rows >= 2
    assert PushSearch(PushWorldPuzzle(text=SEALED)).solve() is None

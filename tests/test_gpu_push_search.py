"""Breadth-first search over pushes with its closed set on the device (pw_push_search_*, search.PushBreadthFirstSearch;
DESIGN.md K16) against the store restatement of tests/push_search_restatement.py over the C oracle's step function: the states
as reached, their canon and their links are compared field by field, in store order.  A large space without a CPU reference
(`room3`) is checked against the move-by-move search: the canonical rows of every state it reaches are the store's."""
import os
import zipfile

import numpy as np
import pytest
import torch

import deep_puzzles
import push_search_restatement as PR
from oracle import c_oracle
from pushworld_amd.puzzle import PushWorldPuzzle
from pushworld_amd.search import (REPLAY_VALID, BreadthFirstSearch, PushBreadthFirstSearch, PushSearch, SetPuzzle, replay_plans,
                                  walk_regions)
from pushworld_amd.vec_env import VecPushWorld
from test_walk_host import HAND

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "pushworld_amd", "data")
SEALED = "A W M0 . G0\n"  # the agent sealed in one cell: a region of one position, no push


def _level(level, name):
    with open(os.path.join(DATA, "puzzles", f"level{level}", name + ".pwp")) as f:
        return f.read()


def _level0(member):
    with zipfile.ZipFile(os.path.join(DATA, "puzzles", "level0.zip")) as z:
        return z.read(member).decode()


SEARCH_CASES = {  # (a copy of test_gpu_walk.SEARCH_CASES)
    "Single Obstacle": lambda: _level(1, "Single Obstacle"),
    "Two Goals": lambda: _level(1, "Two Goals"),
    "2 Obstacle": lambda: _level(1, "2 Obstacle"),
    "level_0_walls_train_1732": lambda: _level0("level0/walls/train/level_0_walls_train_1732.pwp"),
}

_REF = {}


def _reference(key, text, **kw):
    """(oracle puzzle, restatement store) of a case: computed once per session and never changed."""
    if key not in _REF:
        cp = c_oracle.COraclePuzzle(text)
        _REF[key] = (cp, PR.search_store(cp, **kw))
    return _REF[key]


def _counters(s):
    return (s.layer_states, s.num_states, s.pushes, s.push_rows, s.largest_region)


def _store_arrays(bfs):
    pos, canon = bfs.states()
    parent, frm, action, walk, goal = bfs.links()
    return tuple(t.cpu().numpy() for t in (pos, canon, parent, frm, action, walk, goal))


def _check_store(bfs, cp, st):
    """Every field of every state of the store against the restatement's, in store order."""
    pos, canon, parent, frm, action, walk, goal = _store_arrays(bfs)
    n, N = st.num_states, cp.num_movables
    assert bfs.num_states == n and pos.shape == (n, int(bfs._engine.np), 2) and pos.dtype == np.int8
    assert (pos[:, :N] == np.asarray(st.states, np.int8)).all() and (pos[:, N:] == 0).all()
    assert (canon == np.asarray(st.canons, np.int8)).all()
    assert parent.tolist() == [ln.parent for ln in st.links]
    assert [tuple(q) for q in frm.tolist()] == [tuple(ln.frm) for ln in st.links]
    assert action.tolist() == [ln.action for ln in st.links]
    assert walk.tolist() == [ln.walk for ln in st.links]
    assert goal.tolist() == [int(ln.goal) for ln in st.links]
    assert bfs.layers == st.layers and bfs.goal_index == st.goal_index
    return pos, canon, parent, frm, action, walk, goal


def _replays_valid(pz, plan):
    eng = pz._engine()
    plans = torch.as_tensor(np.asarray([plan], np.uint8), device=eng.device)
    out = replay_plans(eng, torch.zeros(1, dtype=torch.int32, device=eng.device), plans,
                       torch.as_tensor([len(plan)], dtype=torch.int32, device=eng.device), rows=False)
    return out.verdict.cpu().tolist() == [REPLAY_VALID]


# ---- 1. the four search cases ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SEARCH_CASES))
def test_search_cases(name):
    text = SEARCH_CASES[name]()
    cp, st = _reference(name, text)
    pz = PushWorldPuzzle(text=text)
    with PushBreadthFirstSearch(pz) as bfs:
        plan = bfs.solve()
        assert plan == PR.plan_of(cp, st, st.goal_index)
        assert _counters(bfs) == _counters(st)
        assert bfs.num_states == bfs.goal_index + 1
        _check_store(bfs, cp, st)
        assert bfs.plan(0) == []
    assert pz.is_valid_plan(plan) and _replays_valid(pz, plan)
    with PushBreadthFirstSearch(pz) as bfs:
        assert bfs.solve(max_pushes=st.pushes - 1) is None
        assert bfs.layer_states == st.layer_states[:st.pushes - 1] and bfs.pushes is None


# ---- 2. `big` to exhaustion ---------------------------------------------------------------------------------------------------
BIG_LAYERS = [8, 36, 100, 220, 296, 278, 168, 96, 40, 12, 4, 1, 0]
_BIG = {}


def _big_reference():
    return _reference("big", deep_puzzles.big(), stop_at_goal=False)


def _big_baseline():
    """The store of `big` from a search with default options (checked against the restatement by test_big_exhausted)."""
    if not _BIG:
        with PushBreadthFirstSearch(PushWorldPuzzle(text=deep_puzzles.big()), stop_at_goal=False) as bfs:
            assert bfs.solve() is None
            _BIG["counters"] = _counters(bfs)
            _BIG["store"] = _store_arrays(bfs)
    return _BIG


def _pushing_steps(states):
    return int((states[1:, 1:] != states[:-1, 1:]).any(axis=(1, 2)).sum())


def test_big_exhausted():
    cp, st = _big_reference()
    pz = PushWorldPuzzle(text=deep_puzzles.big())
    with PushBreadthFirstSearch(pz, stop_at_goal=False) as bfs:
        assert bfs.solve() is None and bfs.exhausted
        assert _counters(bfs) == (BIG_LAYERS, 1260, None, 6464, 34) == _counters(st)
        pos, *_ = _check_store(bfs, cp, st)
        depth = np.zeros(bfs.num_states, np.int64)
        for d, (first, n) in enumerate(bfs.layers):
            depth[first:first + n] = d
        eng = pz._engine()
        for i in range(0, bfs.num_states, 97):
            plan = bfs.plan(i)
            assert plan == PR.plan_of(cp, st, i)
            got, _ = eng.plan_states(0, bytes(plan))
            assert (got[-1] == pos[i, :cp.num_movables]).all() and _pushing_steps(got) == depth[i]
    base = _big_baseline()
    assert base["counters"] == _counters(st)


# ---- 3. the same run under different options ----------------------------------------------------------------------------------
def _same_as_baseline(bfs, npad=4):
    base = _big_baseline()
    assert bfs.solve() is None
    assert _counters(bfs) == base["counters"]
    got = _store_arrays(bfs)
    assert got[0].shape[1] == npad
    assert (got[0][:, :4] == base["store"][0]).all() and (got[0][:, 4:] == 0).all()
    for g, w in zip(got[1:], base["store"][1:]):
        assert g.shape == w.shape and (g == w).all()


def test_big_many_passes_per_layer():
    with PushBreadthFirstSearch(PushWorldPuzzle(text=deep_puzzles.big()), stop_at_goal=False, chunk=7) as bfs:
        _same_as_baseline(bfs)


@pytest.mark.parametrize("bits", [1, 2, 32])
def test_big_fingerprint_bits(bits):
    pz = PushWorldPuzzle(text=deep_puzzles.big())
    eng = pz._engine()
    eng.set_option("push_search_fp_bits", bits)
    try:
        assert eng.get_option("push_search_fp_bits") == bits
        with PushBreadthFirstSearch(pz, stop_at_goal=False, chunk=7 if bits == 1 else None) as bfs:
            _same_as_baseline(bfs)
    finally:
        eng.set_option("push_search_fp_bits", 0)
    for bad in (-1, 33):
        with pytest.raises(ValueError, match="PW_OPT_PUSH_SEARCH_FP_BITS"):
            eng.set_option("push_search_fp_bits", bad)


@pytest.mark.parametrize("tables", ["all", "big", "none"])
def test_big_step_tables(tables):
    vec = VecPushWorld([PushWorldPuzzle(text=deep_puzzles.big())], 1, observation=None, max_steps=None,
                       engine_options={"step_tables": tables})
    with PushBreadthFirstSearch(SetPuzzle(vec.pset, 0, vec.engine), stop_at_goal=False) as bfs:
        _same_as_baseline(bfs)


@pytest.mark.parametrize("npad, index", [(4, 0), (8, 0), (8, 1), (16, 1), (32, 0), (32, 2)])
def test_big_padded(npad, index):
    """`big` as puzzle `index` of a set padded to `npad` by puzzles with more movables."""
    extra = {4: None, 8: 4, 16: 10, 32: deep_puzzles.POCKETS_EXTRA}[npad]
    texts = [deep_puzzles.pockets(extra)] * max(index, 1) if extra else []
    texts.insert(index, deep_puzzles.big())
    vec = VecPushWorld([PushWorldPuzzle(text=t) for t in texts], len(texts), observation=None, max_steps=None)
    assert vec.num_objects_padded == npad and texts.index(deep_puzzles.big()) == index
    with PushBreadthFirstSearch(SetPuzzle(vec.pset, index, vec.engine), stop_at_goal=False) as bfs:
        _same_as_baseline(bfs, npad)
        if index:  # the plan's own flood takes the puzzle's index too
            cp, st = _big_reference()
            for i in (1, 700, bfs.num_states - 1):
                assert bfs.plan(i) == PR.plan_of(cp, st, i)


# ---- 4. more than 16 movables: no 63-bit key ----------------------------------------------------------------------------------
def _with_bits(pz, bits, run):
    eng = pz._engine()
    eng.set_option("push_search_fp_bits", bits)
    try:
        return run()
    finally:
        eng.set_option("push_search_fp_bits", 0)


@pytest.mark.parametrize("bits", [0, 1])
def test_pockets_17_movables(bits):
    text = deep_puzzles.pockets(15)
    pz = PushWorldPuzzle(text=text)
    assert pz.num_movables == 17

    def run():
        cp, st = _reference("pockets", text)
        with PushBreadthFirstSearch(pz) as bfs:
            plan = bfs.solve()
            assert plan == PR.plan_of(cp, st, st.goal_index) and pz.is_valid_plan(plan)
            assert _counters(bfs) == _counters(st)
            _check_store(bfs, cp, st)
        cp, st = _reference("pockets exhausted", text, stop_at_goal=False)
        with PushBreadthFirstSearch(pz, stop_at_goal=False) as bfs:
            assert bfs.solve() is None and _counters(bfs) == _counters(st)
            _check_store(bfs, cp, st)

    _with_bits(pz, bits, run)


@pytest.mark.parametrize("bits", [0, 1])
def test_clean_sweep_two_layers(bits):
    text = _level(2, "Clean Sweep")
    pz = PushWorldPuzzle(text=text)
    cp, st = _reference("Clean Sweep 2", text, max_pushes=2)
    assert cp.num_movables == 19 and st.goal_index == -1 and st.num_states > 100

    def run():
        with PushBreadthFirstSearch(pz, chunk=5 if bits else None) as bfs:
            assert bfs.solve(max_pushes=2) is None
            assert _counters(bfs) == _counters(st)
            _check_store(bfs, cp, st)

    _with_bits(pz, bits, run)


# ---- 5. against the search move by move ---------------------------------------------------------------------------------------
def _canonical_keys(pos, canon):
    k = pos.clone()
    k[:, 0, :] = canon
    return k.view(torch.uint8).reshape(pos.shape[0], -1)


def _cross_check(text, max_states):
    pz = PushWorldPuzzle(text=text)
    eng = pz._engine()
    npad, N = int(eng.np), pz.num_movables
    eng.set_option("search_keys", 1)
    try:
        moves = BreadthFirstSearch(pz, max_states=max_states)
        moves.begin()
        while not moves.exhausted:
            moves.expand()
    finally:
        eng.set_option("search_keys", 0)
    reached = torch.zeros((moves.total_states, npad, 2), dtype=torch.int8, device=eng.device)
    reached[:, :N] = torch.as_tensor(moves.states().astype(np.int8), device=eng.device)
    moves.close()
    reg = walk_regions(eng, torch.zeros(reached.shape[0], dtype=torch.int32, device=eng.device), reached)
    assert bool((reg.region_size > 0).all())
    want = torch.unique(_canonical_keys(reached, reg.canon), dim=0)  # (sorted rows)
    with PushBreadthFirstSearch(pz, max_states=max_states, stop_at_goal=False) as bfs:
        assert bfs.solve() is None and bfs.exhausted
        pos, canon = bfs.states()
        got = torch.unique(_canonical_keys(pos, canon), dim=0)
        assert got.shape[0] == bfs.num_states  # no two equal canonical rows in the store
        assert got.shape == want.shape and torch.equal(got, want)
        assert sum(bfs.layer_states) + 1 == bfs.num_states
        parent = bfs.links()[0].cpu().numpy()
        depth = np.zeros(bfs.num_states, np.int64)
        for d, (first, n) in enumerate(bfs.layers):
            depth[first:first + n] = d
        assert parent[0] == -1 and (depth[parent[1:]] == depth[1:] - 1).all()
        return moves.total_states, bfs.num_states


def test_big_against_moves():
    assert _cross_check(deep_puzzles.big(), 1 << 16) == (42832, 1260)


def test_room3_against_moves():
    moves, pushes = _cross_check(deep_puzzles.room3(), 1 << 21)
    assert 1 << 20 < moves <= 36 * 35 * 34 * 33 and 1260 < pushes < moves


# ---- 6. limits and edges ----------------------------------------------------------------------------------------------------------
def test_store_full_and_begin_again():
    text = SEARCH_CASES["level_0_walls_train_1732"]()
    cp, st = _reference("1732 exhausted", text, stop_at_goal=False)
    assert st.num_states == 380
    with PushBreadthFirstSearch(PushWorldPuzzle(text=text), max_states=100, stop_at_goal=False) as bfs:
        with pytest.raises(ValueError, match="max_states"):
            bfs.solve()
        assert bfs.num_states == 100
        with pytest.raises(ValueError, match="max_states"):
            bfs.expand()
        bfs.begin()  # the handle is usable again
        info = bfs.expand()
        assert (info.depth, info.new_states, info.total_states, info.goal_index) == (1, st.layer_states[0], 1 + st.layer_states[0], -1)
        pos, canon = bfs.states()
        assert (pos.cpu().numpy()[:, :cp.num_movables] == np.asarray(st.states[:bfs.num_states], np.int8)).all()
        assert (canon.cpu().numpy() == np.asarray(st.canons[:bfs.num_states], np.int8)).all()
    # layers of thousands of rows against a store of 300 and a table of 1 024 slots: the probes end at the table's size
    with PushBreadthFirstSearch(PushWorldPuzzle(text=deep_puzzles.room3()), max_states=300, stop_at_goal=False) as bfs:
        with pytest.raises(ValueError, match="max_states"):
            bfs.solve()
        assert bfs.num_states == 300
        bfs.begin()
        assert bfs.expand().new_states > 0
    with PushBreadthFirstSearch(PushWorldPuzzle(text=text), max_states=380, stop_at_goal=False) as bfs:  # exactly full is not over
        assert bfs.solve() is None and _counters(bfs) == _counters(st)


def test_goal_start_no_solution_and_bad_start():
    cp = c_oracle.COraclePuzzle(HAND)
    m0 = cp.py.names.index("m0")
    solved = tuple((4, 2) if k == m0 else xy for k, xy in enumerate(cp.initial_state))
    with PushBreadthFirstSearch(PushWorldPuzzle(text=HAND)) as bfs:
        bfs.begin(solved)
        assert bfs.solve() == [] and (bfs.pushes, bfs.num_states, bfs.layer_states, bfs.goal_index) == (0, 1, [], 0)
        assert bfs.links()[4].cpu().tolist() == [1]
        with pytest.raises(ValueError, match="ended"):
            bfs.expand()
        for outside in ((cp.width, 2), (-1, 2), (300, 2)):  # a goal start is checked like any other
            with pytest.raises(ValueError, match="outside the grid"):
                bfs.begin((outside,) + solved[1:])
            with pytest.raises(ValueError, match="begin"):
                bfs.expand()
        bfs.begin()
        assert bfs.solve() == [1] and (bfs.pushes, bfs.layer_states, bfs.num_states) == (1, [], 3)
        first = _store_arrays(bfs)
        bfs.begin()  # twice on one handle: identical
        assert bfs.solve() == [1] and (bfs.pushes, bfs.layer_states, bfs.num_states) == (1, [], 3)
        assert all((g == w).all() for g, w in zip(_store_arrays(bfs), first))
    # the box can only be pushed away from its goal: exhausted without one
    text = "G0 . A . M0 . .\n"
    cp, st = _reference("away", text)
    assert st.goal_index == -1 and st.push_rows >= 2
    with PushBreadthFirstSearch(PushWorldPuzzle(text=text)) as bfs:
        assert bfs.solve() is None and _counters(bfs) == _counters(st)
        _check_store(bfs, cp, st)
    with PushBreadthFirstSearch(PushWorldPuzzle(text=SEALED)) as bfs:
        assert bfs.solve() is None
        assert (bfs.layer_states, bfs.num_states, bfs.push_rows, bfs.largest_region) == ([0], 1, 0, 1)


def test_begin_twice_on_a_long_search():
    name = "Two Goals"
    cp, st = _reference(name, SEARCH_CASES[name]())
    with PushBreadthFirstSearch(PushWorldPuzzle(text=SEARCH_CASES[name]()), chunk=3) as bfs:
        for _ in range(2):
            bfs.begin()
            assert bfs.solve() == PR.plan_of(cp, st, st.goal_index) and _counters(bfs) == _counters(st)
            _check_store(bfs, cp, st)


def test_small_store_where_moves_do_not_fit():
    pz = PushWorldPuzzle(text=SEARCH_CASES["2 Obstacle"]())
    with PushBreadthFirstSearch(pz, max_states=4096) as bfs:
        plan = bfs.solve()
        assert bfs.num_states == 416 and pz.is_valid_plan(plan)
    with pytest.raises(ValueError, match="max_states"):
        BreadthFirstSearch(pz, max_states=4096).solve()


# ---- 7. agreement with the first search over pushes ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SEARCH_CASES))
def test_agrees_with_push_search(name):
    pz = PushWorldPuzzle(text=SEARCH_CASES[name]())
    old = PushSearch(pz)
    plan = old.solve()
    with PushBreadthFirstSearch(pz) as bfs:
        assert bfs.solve() == plan
        assert _counters(bfs) == _counters(old)

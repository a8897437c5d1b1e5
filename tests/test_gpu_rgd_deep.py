"""RGD on the device at its limits (pw_rgd_*, and the copies of its LDS layout in pw_plan_batch): the shipped Level-2..4
puzzles, ladders of up to 32 movables whose first finite pushing depth is N - 2 (30 stack frames), the budget counted all the
way down such a chain, distance tables on 64 x 64 boards and on a path 1 951 edges long, and the planners on ladders.  Every
value is compared with the plain-Python restatement (tests/rgd_restatement.py) bit for bit, +inf and NaN included: costs are
integers in float32, so no tolerance is involved.  The constructed puzzles are in tests/rgd_puzzles.py and pinned without a
device in tests/test_rgd_puzzles_host.py.

Host seconds measured (restatement only): Level 2 / 3 / 4 8.7 / 11.0 / 4.1; the ladder walks 0.1 - 3.3 each, (31, 0) with
fewest_tools 5; the room's distances 3; the planner restatement on the two ladders 3 per heuristic."""
import os
import random
import sys
import zlib

import numpy as np
import pytest
import torch

from oracle import pw_oracle
from pushworld_amd.puzzle import PushWorldPuzzle
from pushworld_amd.search import BestFirstSearch, PlanBatch, RecursiveGraphDistance
from pushworld_amd.vec_env import VecPushWorld

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deep_puzzles  # noqa: E402
import planner_restatement  # noqa: E402
import rgd_puzzles as P  # noqa: E402
import rgd_restatement as R  # noqa: E402
from rgd_helpers import MAX_CALLS, ROOT, compare, dev, enc  # noqa: E402

pytestmark = pytest.mark.gpu

REF_CPP = os.path.join(ROOT, "tests", "puzzles", "ref_cpp")


def bits(values):
    """float32 bit patterns (NaN compares equal to NaN, +inf to +inf)."""
    return np.asarray(values, dtype=np.float32).view(np.uint32)


# ---- a. Levels 2, 3 and 4 -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [2, 3, 4])
def test_levels_match_the_restatement(level):
    """Every puzzle of the level, 8 states each (initial, five along the shipped plan, two of a random walk), fewest_tools.
    The restatement takes the library's host-built movement graphs, which tests/test_rgd_host.py pins equal to its own on
    every one of these puzzles (growing them in Python is 20 of the 30 seconds a level would take).  Measured: 592 / 536 /
    112 states, none skipped, at most 124 calls."""
    compared = skipped = many = 0
    for path in P.level_paths(level):
        with open(path) as f:
            text = f.read()
        pz, oz = PushWorldPuzzle(text=text), pw_oracle.OraclePuzzle(text)
        graphs = [pz.movement_graph(j) for j in range(pz.num_movables)]
        states = P.level_states(path, level, oz, zlib.crc32(os.path.basename(path).encode()))
        h = RecursiveGraphDistance(pz)
        c, s = compare(h, R.RecursiveGraphDistance(oz, True, MAX_CALLS, graphs=graphs), states)
        assert h.exceeded <= s, path  # what the restatement finishes within 4 000 calls never runs out of 4 096 frames
        h.close()
        compared += c
        skipped += s
        if pz.num_movables >= 12:
            assert c >= 5, path
            many += 1
    assert many == {2: 3, 3: 5, 4: 5}[level]  # the 13 puzzles with 12 movables and more
    assert skipped <= 0.05 * (compared + skipped), (compared, skipped)
    assert compared >= 6 * len(P.level_paths(level))


# ---- b. full depth on many movables ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,gap,fewest", P.MODES)
def test_ladder_walks_match_the_restatement(k, gap, fewest):
    text, states, costs, calls = P.ladder_reference(k, gap, fewest)
    skipped = costs.count(None)
    if (k, gap) in P.NEVER_SKIPPED:
        assert skipped == 0
    assert skipped <= P.SKIP_CAP * len(states)
    assert costs[0] == P.ladder_cost(k, gap)
    pz = PushWorldPuzzle(text=text)
    assert pz.num_movables == k + 1
    limit = P.max_calls(k, gap, fewest)
    h = RecursiveGraphDistance(pz, fewest_tools=fewest, budget=None if limit == P.DEFAULT_CALLS else limit)
    got = h.evaluate(dev(states, h)).cpu().numpy()
    keep = [i for i, c in enumerate(costs) if c is not None]
    for i in keep:
        assert bits(got[i]) == bits(costs[i]), (states[i], float(got[i]), costs[i], calls[i])
    assert h.exceeded <= skipped
    # the same states in launches of 1, 63, 64 and 65 rows: the lanes of a wavefront at different stack depths
    base = dev([states[i] for i in keep], h)
    want = np.asarray([costs[i] for i in keep], dtype=np.float32)
    order = np.random.default_rng(k * 10 + gap).permutation(len(keep))
    for F in (1, 63, 64, 65):
        idx = order[np.arange(F) % len(order)]
        out = h.evaluate(base[torch.as_tensor(idx, device=h.device)].contiguous()).cpu().numpy()
        assert (bits(out) == bits(want[idx])).all(), (F, out, want[idx])
    assert h.exceeded <= skipped
    h.close()


# ---- c. the budget at depth 30 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,gap,fewest", [(31, 0, False), (12, 1, True), (12, 3, False)])
def test_budget_counts_every_frame_of_a_deep_chain(k, gap, fewest):
    text = P.ladder(k, gap)
    pz, oz = PushWorldPuzzle(text=text), pw_oracle.OraclePuzzle(text)
    ref = R.RecursiveGraphDistance(oz, fewest_tools=fewest)
    s0 = oz.initial_state
    want = ref.estimate(s0)
    assert want == P.ladder_cost(k, gap)
    assert ref.calls == {(31, 0): 31, (12, 1): 1242, (12, 3): 474}[(k, gap)]  # with fewest_tools summed over the depths tried
    exact = RecursiveGraphDistance(pz, fewest_tools=fewest, budget=ref.calls)
    assert exact.evaluate(dev([s0, s0], exact)).cpu().numpy().tolist() == [want, want]
    assert exact.exceeded == 0
    short = RecursiveGraphDistance(pz, fewest_tools=fewest, budget=ref.calls - 1)
    got = short.evaluate(dev([s0], short)).cpu().numpy()
    assert np.isnan(got[0]) and short.exceeded == 1
    exact.close()
    short.close()


# ---- d. distance tables at the limits -------------------------------------------------------------------------------------
def distances(h, obj, src, dst):
    return h.distance(obj, torch.tensor(enc(src), dtype=torch.int32, device=h.device),
                      torch.tensor(enc(dst), dtype=torch.int32, device=h.device)).cpu().numpy()


def check_pairs(h, dist, obj, src, dst):
    got = distances(h, obj, src, dst)
    want = [dist.get(s, t) for s, t in zip(src, dst)]
    assert (bits(got) == bits(want)).all(), [(s, t, float(g), w) for s, t, g, w in zip(src, dst, got, want)
                                             if float(g) != w][:5]
    return want


def test_distances_on_the_64x64_room():
    text = P.room(62, 62)
    pz, oz = PushWorldPuzzle(text=text), pw_oracle.OraclePuzzle(text)
    assert tuple(pz.dimensions) == (64, 64)
    graphs = R.movement_graphs(oz)
    h = RecursiveGraphDistance(pz)
    rng = random.Random(62)
    # the corners, and both sides of the middle of the 64-bit row masks (x) and of the wavefront (y)
    special = [(1, 1), (62, 1), (1, 62), (62, 62)] + [(x, y) for x in (31, 32, 33) for y in (31, 32, 33)]
    for obj in (0, 1):
        assert len(graphs[obj]) == 3844
        dist = R.PathDistances(graphs[obj])
        nodes = sorted(graphs[obj])
        src = [s for s in special for _ in special] + [rng.choice(nodes) for _ in range(200)]
        dst = [t for _ in special for t in special] + [rng.choice(nodes) for _ in range(200)]
        want = check_pairs(h, dist, obj, src, dst)
        assert max(w for w in want if w != R.INF) >= 100
        if obj == 1:  # the box leaves neither a wall nor a corner: both orders of a pair differ
            assert sum(1 for w in want if w == R.INF) >= 20
            assert sum(1 for s, t, w in zip(src, dst, want) if w != R.INF and dist.get(t, s) != w) >= 20
        for target in ((33, 32), (62, 62)):  # one whole row of the table: every source
            check_pairs(h, dist, obj, nodes, [target] * len(nodes))
    assert h.evaluate(dev([oz.initial_state], h)).cpu().numpy().tolist() == [R.RecursiveGraphDistance(oz).estimate(
        oz.initial_state)]
    h.close()


def test_distances_on_the_62x61_serpentine():
    text = deep_puzzles.serpentine(62, 61)
    pz, oz = PushWorldPuzzle(text=text), pw_oracle.OraclePuzzle(text)
    graphs = R.movement_graphs(oz)
    path = [(x + 1, y + 1) for x, y in deep_puzzles.serpentine_path(62, 61)]
    assert sorted(graphs[0]) == sorted(path)
    h = RecursiveGraphDistance(pz)
    agent = R.PathDistances(graphs[0])
    # the agent's graph is the one path: its ends are len(path) - 1 = 1 951 apart, by construction
    assert h.distance(0, path[0], path[-1]) == len(path) - 1 == 1951
    assert h.distance(0, path[-1], path[0]) == 1951
    src, dst, apart = [], [], []
    for d in (1, 254, 255, 256, 257, 511, 512, 1023, 1024, 1950):
        for i in (0, 7, 300, len(path) - 1 - d):
            if i + d < len(path):
                src += [path[i], path[i + d]]
                dst += [path[i + d], path[i]]
                apart += [d, d]
    assert distances(h, 0, src, dst).tolist() == apart
    check_pairs(h, agent, 0, src, dst)
    # every distance into a wall cell, and from a cell off the graph, is inf
    W, H = pz.dimensions
    walls = [(x, y) for y in range(H) for x in range(W) if (x, y) not in graphs[0]]
    assert len(walls) == W * H - len(path)
    assert np.isinf(distances(h, 0, [path[5]] * len(walls), walls)).all()
    assert np.isinf(distances(h, 0, walls, [path[5]] * len(walls))).all()
    # the box: the last row, pushed both ways but never out of its two end cells -- a directed graph, all pairs
    box = R.PathDistances(graphs[1])
    nodes = sorted(graphs[1])
    assert len(nodes) == 62
    check_pairs(h, box, 1, [s for s in nodes for _ in nodes], [t for _ in nodes for t in nodes])
    start, goal = oz.initial_state[1], oz.goal_state[0]
    assert h.distance(1, start, goal) == 2 and np.isinf(h.distance(1, goal, start))
    assert h.distance(1, (2, 61), (1, 61)) == 1 and np.isinf(h.distance(1, (1, 61), (2, 61)))
    # the start's cost: 1 947 steps up to the box and the first push, then one more cell
    assert h.evaluate(dev([oz.initial_state], h)).cpu().numpy().tolist() == [R.RecursiveGraphDistance(oz).estimate(
        oz.initial_state)] == [1950.0]
    h.close()


def test_all_pairs_of_a_wide_movable_at_the_board_edge():
    """Level 3 `Bear Claw`, movable 5: 9 x 7 cells, 234 nodes, 13 of them against the right border and 18 against the
    bottom one."""
    path = os.path.join(ROOT, "pushworld_amd", "data", "puzzles", "level3", "Bear Claw.pwp")
    with open(path) as f:
        text = f.read()
    pz, oz = PushWorldPuzzle(text=text), pw_oracle.OraclePuzzle(text)
    obj = 5
    assert oz.sizes[obj] == (9, 7)
    graph = R.movement_graphs(oz)[obj]
    nodes = sorted(graph)
    assert len(nodes) == 234
    assert sum(1 for x, y in nodes if x + 9 == oz.width - 1) == 13 and sum(1 for x, y in nodes if y + 7 == oz.height - 1) == 18
    h = RecursiveGraphDistance(pz)
    check_pairs(h, R.PathDistances(graph), obj, [s for s in nodes for _ in nodes], [t for _ in nodes for t in nodes])
    h.close()


# ---- e. the planners' copy of the stack ---------------------------------------------------------------------------------
PLAN_ROUNDS = 40  # both ladders are solved sooner (3 and 18 rounds); the restatement takes 3 s per heuristic (measured)
PLAN_STATES = 1 << 12


def planner_texts():
    with open(os.path.join(REF_CPP, "trivial.pwp")) as f:
        trivial = f.read()
    with open(P.level_paths(2)[0]) as f:
        level2 = f.read()
    return [P.ladder(31, 0), trivial, P.ladder(16, 1), level2]


def single(pz, mode, start=None):
    bfs = BestFirstSearch(pz, heuristic=mode, batch=1, max_states=PLAN_STATES, action_order="fixed")
    try:
        bfs.begin(start=start)
        info = bfs.run(PLAN_ROUNDS)
        return tuple(info), bfs.plan()
    finally:
        bfs.close()


@pytest.mark.parametrize("mode", ["RGD", "N+RGD"])
def test_plan_batch_with_ladders_equals_the_planner_and_the_restatement(mode):
    texts = planner_texts()
    puzzles = [PushWorldPuzzle(text=t) for t in texts]
    assert [p.num_movables for p in puzzles][:3] == [32, 2, 17]
    pb = PlanBatch(puzzles, heuristic=mode, batch=1, max_states=PLAN_STATES, action_order="fixed")
    try:
        pb.run(max_rounds=PLAN_ROUNDS)
        got = pb.results()
    finally:
        pb.close()
    for i, (plan, info, _) in enumerate(got):
        want_info, want_plan = single(puzzles[i], mode)
        assert tuple(info) == want_info, (i, mode)
        assert plan == want_plan, (i, mode)
    assert got[0][0] == [1, 1, 1] and got[1][1].status == "solved"
    for i in (0, 2):  # the ladders against the restatement (4 096: the kernel's default budget of frames)
        oz = pw_oracle.OraclePuzzle(texts[i])
        ref = planner_restatement.PlannerRestatement(oz, mode, batch=1, max_states=PLAN_STATES, rgd_max_calls=4096)
        ref.begin()
        want = ref.run(PLAN_ROUNDS)
        plan, info, _ = got[i]
        assert info.status == want["status"], (i, mode)
        assert (info.rounds, info.expanded, info.visited, info.open) == \
            (want["rounds"], want["expanded"], want["visited"], want["open"]), (i, mode)
        assert info.rgd_exceeded == ref.rgd_exceeded, (i, mode)
        assert plan == ref.plan(), (i, mode)
    assert got[2][1].rgd_exceeded > 0  # the first states of ladder(16, 1) take more than 4 096 frames: NaN keys, popped last


def test_state_planner_with_ladders_equals_the_planner():
    puzzles = [PushWorldPuzzle(text=t) for t in planner_texts()]
    ids = np.repeat(np.arange(4), 3)
    vec = VecPushWorld(puzzles, len(ids), puzzle_ids=ids, observation=None, max_steps=None)
    vec.reset()
    assert vec.num_objects_padded == 32
    initial = vec.states().copy()
    rng = np.random.default_rng(31)
    for t in range(4):  # a few random steps; the first environment of every puzzle goes back to its initial state
        vec.step(torch.as_tensor(rng.integers(0, 4, size=len(ids)).astype(np.uint8), device=vec.device))
    now = vec.states().copy()
    now[::3] = initial[::3]
    assert (now != initial).any()
    vec.set_states(now)
    torch.cuda.synchronize()
    for mode in ("RGD", "N+RGD"):
        sp = vec.planner(heuristic=mode, batch=1, max_states=PLAN_STATES, action_order="fixed")
        try:
            _, _, _, first = sp.plan(vec.puzzle_id, vec.pos, max_rounds=PLAN_ROUNDS, plan_cap=256)
            got = sp.results()
            first = first.cpu().numpy()
        finally:
            sp.close()
        states = vec.states()
        for i, (plan, info, _) in enumerate(got):
            pid = int(ids[i])
            start = [(int(x), int(y)) for x, y in states[i][: puzzles[pid].num_movables]]
            want_info, want_plan = single(puzzles[pid], mode, start=start)
            assert tuple(info) == want_info, (i, mode)
            assert plan == want_plan, (i, mode)
            assert first[i] == (plan[0] if plan else -1), (i, mode)
        assert first[0] == 1  # ladder(31, 0) from its initial state: push right

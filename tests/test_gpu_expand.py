"""-m gpu: config C5 -- batched 4-action successor expansion in the C++ reference's object
order and Position2D encoding, checked against the oracle (order="cpp") and the C++
reference's own known answers (cpp/test/test_pushworld_puzzle.cc, cpp/test/search/*)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "puzzles", "ref_cpp")


def p2d(state):
    return [x * 10000 + y for (x, y) in state]


def bfs(puzzle, max_states):
    """Breadth-first closure with the GPU expansion; returns the visited states (in discovery
    order) and per-state successor / moved / goal arrays."""
    init = tuple(p2d(puzzle.initial_state))
    index = {init: 0}
    order = [init]
    succs, moveds, goals = [], [], []
    lo = 0
    while lo < len(order) and len(order) < max_states:
        layer = np.array(order[lo:], dtype=np.int32)
        lo = len(order)
        s, m, g = puzzle.expand4(layer)
        s, m, g = s.cpu().numpy(), m.cpu().numpy().astype(np.uint32), g.cpu().numpy()
        succs.append(s)
        moveds.append(m)
        goals.append(g)
        for row in s.reshape(-1, s.shape[-1]):
            t = tuple(int(v) for v in row)
            if t not in index:
                index[t] = len(order)
                order.append(t)
    n = sum(len(x) for x in succs)
    return order, np.concatenate(succs), np.concatenate(moveds), np.concatenate(goals), n


@pytest.mark.parametrize("key", [
    "cpptest:trivial.pwp", "cpptest:trivial_tool.pwp", "cpptest:trivial_tool2.pwp", "cpptest:easy_search.pwp",
    "cpptest:blocked_transitive_pushing1.pwp", "cpptest:blocked_transitive_pushing2.pwp",
    "cpptest:necessary_transitive_pushing3.pwp", "cpptest:multiple_goals.pwp", "cpptest:file_parsing.pwp",
    "bench:level1/2 Obstacle.pwp", "bench:level2/Pull Dont Push.pwp", "bench:level4/Four Pistons.pwp",
    "bench:level1/Pulling.pwp", "bench:level3/Armor.pwp",
    "bench:level2/Clean Sweep.pwp",  # 19 movables: the 32-lane instantiation
    # movables beyond 8 x 8 cells: overlap tables by default (PW_OPT_STEP_TABLES, automatic), the row loops with "none"
    "bench:level4/Mind The Gap.pwp", "bench:level4/Mind The Gap.pwp|none", "bench:level2/Bubbles.pwp",
    "bench:level3/Rocky Shore.pwp", "bench:level3/Rocky Shore.pwp|none", "bench:level3/Moving Mountains.pwp",
    # ... and tables for puzzles of small movables
    "bench:level1/2 Obstacle.pwp|all", "bench:level4/Four Pistons.pwp|all", "bench:level2/Clean Sweep.pwp|all",
    "cpptest:necessary_transitive_pushing3.pwp|all",
    # 9 .. 16 movables: 8-lane groups with two movables per lane by default; "wide": one movable per lane, 16 lanes
    "bench:level4/Four Pistons.pwp|wide", "bench:level4/Mind The Gap.pwp|wide", "bench:level1/Pulling.pwp|wide",
    # one lane per state (pw_expand4_lane_kernel: what frontiers of >= 131 072 states run by themselves), forced here
    # for layers of every size incl. ragged last blocks
    "cpptest:trivial.pwp|lanes", "cpptest:trivial_tool2.pwp|lanes", "cpptest:blocked_transitive_pushing1.pwp|lanes",
    "cpptest:blocked_transitive_pushing2.pwp|lanes", "cpptest:necessary_transitive_pushing3.pwp|lanes",
    "cpptest:multiple_goals.pwp|lanes", "cpptest:file_parsing.pwp|lanes", "bench:level1/2 Obstacle.pwp|lanes",
    "bench:level2/Pull Dont Push.pwp|lanes", "bench:level4/Four Pistons.pwp|lanes", "bench:level4/Mind The Gap.pwp|lanes",
    "bench:level3/Armor.pwp|lanes", "bench:level3/Rocky Shore.pwp|lanes", "bench:level2/Bubbles.pwp|lanes",
    "bench:level3/Moving Mountains.pwp|lanes", "bench:level1/A Tight Squeeze.pwp|lanes",  # (N = 2: rows of one word)
    "bench:level2/Clean Sweep.pwp|lanes",  # 19 movables: the instance with 32 bits per action
    # "lanes" runs pw_expand4_v2_kernel (push tables in LDS) wherever it applies -- 2 .. 16 movables, tables up to 112 KB --;
    # "lanes-hbm": pw_expand4_lane_kernel (tables read through L1) for the same puzzles
    "cpptest:trivial_tool2.pwp|lanes-hbm", "cpptest:blocked_transitive_pushing2.pwp|lanes-hbm",
    "cpptest:necessary_transitive_pushing3.pwp|lanes-hbm", "cpptest:multiple_goals.pwp|lanes-hbm",
    "bench:level1/2 Obstacle.pwp|lanes-hbm", "bench:level2/Pull Dont Push.pwp|lanes-hbm", "bench:level4/Four Pistons.pwp|lanes-hbm",
    "bench:level3/Armor.pwp|lanes-hbm", "bench:level1/A Tight Squeeze.pwp|lanes-hbm",
    # tables of 50 .. 103 KB in LDS (one or two workgroups per CU)
    "bench:level3/Caged Key.pwp|lanes", "bench:level3/Crow Pulling.pwp|lanes", "bench:level2/Lock And Load.pwp|lanes",
    "bench:level1/Pulling.pwp|lanes", "bench:level3/Put Away Toys.pwp|lanes", "bench:level2/Encircle.pwp|lanes",
    "bench:level4/Pinhole Lock.pwp|lanes",
    # "lanes-hbm-runs": that kernel with all four actions staged at once and non-temporal stores (what it does by itself up to
    # 14 movables wherever the LDS kernel does not apply: tables beyond 112 KB, unaligned buffers), forced for every N
    "cpptest:multiple_goals.pwp|lanes-hbm-runs", "bench:level1/2 Obstacle.pwp|lanes-hbm-runs", "bench:level2/Pull Dont Push.pwp|lanes-hbm-runs",
    "bench:level4/Four Pistons.pwp|lanes-hbm-runs", "bench:level3/Armor.pwp|lanes-hbm-runs", "bench:level1/A Tight Squeeze.pwp|lanes-hbm-runs",
    "bench:level1/Pull Up.pwp|lanes-hbm-runs", "bench:level4/Pinhole Lock.pwp|lanes-hbm-runs", "bench:level3/Chain Link Tunnel.pwp|lanes-hbm-runs",
    "bench:level2/Simultaneous Obstacle Removal.pwp|lanes-hbm-runs", "bench:level2/Clean Sweep.pwp|lanes-hbm-runs",
    # more movable counts for the LDS kernel's per-N instances (5, 8, 9, 10, 11, 14 ...)
    # every movable count the LDS kernel is instantiated for: 4 .. 16 (2, 3, 6, 7, 12 are above)
    "bench:level1/At Crossroads.pwp|lanes", "bench:level1/Building Blocks.pwp|lanes", "bench:level1/Pull Up.pwp|lanes",
    "bench:level1/Dont Get Distracted.pwp|lanes", "bench:level1/Ignorable Obstacles.pwp|lanes",
    "bench:level1/Irrelevant Obstacles.pwp|lanes", "bench:level2/Remote Obstacle.pwp|lanes", "bench:level3/Yin Yang.pwp|lanes",
    "bench:level3/Chain Link Tunnel.pwp|lanes", "bench:level4/Tool Chain.pwp|lanes",
    "bench:level2/Simultaneous Obstacle Removal.pwp|lanes", "bench:level3/Close But Far.pwp|lanes",
    "bench:level3/Crow Pushing.pwp|lanes",
])
def test_bfs_layers_match_oracle(golden, key):
    from oracle import c_oracle
    from pushworld_amd.puzzle import PushWorldPuzzle

    key, _, tables = key.partition("|")
    if key not in golden.meta:
        pytest.skip("puzzle not in the fixture set")
    text = golden.text(key)
    pz = PushWorldPuzzle(text=text, order="cpp")
    if tables == "wide":
        pz._engine().set_option("step_wide_groups", 1)
    elif tables in ("lanes", "lanes-hbm", "lanes-hbm-runs"):
        pz._engine().set_option("step_kernel", "lane")
        pz._engine().set_option("expand_lds_tables", {"lanes": "auto", "lanes-hbm": "never", "lanes-hbm-runs": 3}[tables])
    elif tables:
        pz._engine().set_option("step_tables", tables)
        assert (pz._engine().get_option("step_table_puzzles") == 1) == (tables == "all")
    oz = c_oracle.COraclePuzzle(text, order="cpp")
    assert tuple(pz.initial_state) == tuple(oz.initial_state)
    order, succ, moved, goal, n = bfs(pz, 6000)
    assert n >= 1
    for i in range(n):
        st = tuple((v // 10000, v % 10000) for v in order[i])
        for a in range(4):
            nxt, mv = oz.get_next_state_moved(st, a)
            assert succ[i, a].tolist() == p2d(nxt), (key, i, a)
            mask = 0
            for k in mv:
                mask |= 1 << k
            assert int(moved[i, a]) == mask, (key, i, a)  # agent first, ascending; empty if blocked
            assert bool(goal[i, a]) == oz.py.is_goal_state(nxt), (key, i, a)


@pytest.mark.parametrize("key", ["bench:level1/2 Obstacle.pwp", "bench:level2/Pull Dont Push.pwp", "bench:level4/Four Pistons.pwp",
                                 "bench:level4/Mind The Gap.pwp", "bench:level1/Pulling.pwp", "bench:level2/Clean Sweep.pwp"])
def test_lane_kernel_with_unaligned_buffers_and_ragged_sizes(golden, key):
    """pw_expand4_lane_kernel picks its store width (16 / 8 / 4 bytes) and how many actions it stages at a time from N
    and from the alignment of the caller's buffers: output buffers that start 4 bytes (succ, moved) / 1 byte (goal) into
    an allocation, and state counts around the 64-state blocks, give the same successors as the lane groups."""
    import torch

    from pushworld_amd.puzzle import PushWorldPuzzle

    if key not in golden.meta:
        pytest.skip("puzzle not in the fixture set")
    pz = PushWorldPuzzle(text=golden.text(key), order="cpp")
    order, _, _, _, n = bfs(pz, 3000)
    states = np.array(order[:n], dtype=np.int32)
    N = states.shape[1]
    eng = pz._engine()
    dev = "cuda:0"
    for F in (1, 63, 64, 65, 129, min(n, 1500)):
        F = min(F, n)
        st = torch.as_tensor(states[:F]).to(dev)
        eng.set_option("step_kernel", "group")
        eng.set_option("step_lane_batch", "never")
        want = [torch.empty((F, 4, N), dtype=torch.int32, device=dev), torch.empty((F, 4), dtype=torch.int32, device=dev),
                torch.empty((F, 4), dtype=torch.uint8, device=dev)]
        eng.expand4(0, st, *want)
        eng.set_option("step_kernel", "lane")
        for off in (0, 1, 2, 0):
            # (aligned buffers: the kernel with the tables in LDS where the puzzle qualifies; the second aligned pass with that
            # kernel switched off, i.e. pw_expand4_lane_kernel's 16-byte path)
            eng.set_option("expand_lds_tables", "auto" if off else ("never" if eng.get_option("expand_lds_tables") == 0 and F == 65 else "auto"))
            raw = [torch.full((F * 4 * N + 8,), -7, dtype=torch.int32, device=dev), torch.full((F * 4 + 8,), -7, dtype=torch.int32, device=dev),
                   torch.full((F * 4 + 8,), 77, dtype=torch.uint8, device=dev)]
            got = [raw[0][off:off + F * 4 * N].view(F, 4, N), raw[1][off:off + F * 4].view(F, 4), raw[2][off:off + F * 4].view(F, 4)]
            eng.expand4(0, st, *got)
            torch.cuda.synchronize()
            for g, w in zip(got, want):
                assert torch.equal(g, w), (key, F, off)
            # nothing outside the views was written
            assert int((raw[0][:off] != -7).sum()) == 0 and int((raw[0][off + F * 4 * N:] != -7).sum()) == 0
            assert int((raw[1][:off] != -7).sum()) == 0 and int((raw[1][off + F * 4:] != -7).sum()) == 0
            assert int((raw[2][:off] != 77).sum()) == 0 and int((raw[2][off + F * 4:] != 77).sum()) == 0


@pytest.mark.parametrize("kernel", ["group", "lane"])
def test_overlapping_states_against_the_reference(golden, kernel):
    """Random in-bounds states of the fixtures in which movables overlap each other and walls, with the successors the
    REFERENCE computed for them (tests/golden/make_golden.py): pins the not-already-overlapping clause of the collision
    tables (puzzle.py:522-593) for the expansion kernels -- the lane kernel answers from the push tables, whose nibbles
    are built with exactly that clause."""
    from pushworld_amd.puzzle import PushWorldPuzzle

    n_states = n_puzzles = 0
    for k in golden.keys:
        if f"{k}|in" not in golden.states:
            continue
        st = golden.states[f"{k}|in"].astype(np.int64)            # [S][N][2]
        want = golden.states[f"{k}|out"].astype(np.int64)         # [S][4][N][2]
        pz = PushWorldPuzzle(text=golden.text(k))                 # the reference's own object order
        pz._engine().set_option("step_kernel", kernel)
        succ, moved, goal = pz.expand4(st[:, :, 0] * 10000 + st[:, :, 1])
        got = succ.cpu().numpy().astype(np.int64)
        assert (got == want[:, :, :, 0] * 10000 + want[:, :, :, 1]).all(), k
        mv = moved.cpu().numpy().astype(np.uint32)
        changed = (want != st[:, None]).any(axis=3)               # [S][4][N]: who moved
        bits = (changed * (1 << np.arange(changed.shape[2], dtype=np.uint32))).sum(axis=2).astype(np.uint32)
        assert (mv == bits).all(), k
        n_states += st.shape[0]
        n_puzzles += 1
    assert n_puzzles >= 20 and n_states >= 500


def test_lane_kernel_on_an_agent_alone():
    """N = 1 (an agent, walls, nothing to push, no goal): rows of one Position2D, divisions by one in the staging code."""
    from oracle import c_oracle
    from pushworld_amd.puzzle import PushWorldPuzzle

    text = "\n".join("  ".join(r) for r in ([".", "W", ".", "."], ["A", ".", ".", "W"], [".", ".", "AW", "."]))
    pz = PushWorldPuzzle(text=text, order="cpp")
    oz = c_oracle.COraclePuzzle(text, order="cpp")
    pz._engine().set_option("step_kernel", "lane")
    order, succ, moved, goal, n = bfs(pz, 1000)
    assert n >= 5 and len(order[0]) == 1
    for i in range(n):
        st = tuple((v // 10000, v % 10000) for v in order[i])
        for a in range(4):
            nxt, mv = oz.get_next_state_moved(st, a)
            assert succ[i, a].tolist() == p2d(nxt) and int(moved[i, a]) == (1 if mv else 0)
            assert bool(goal[i, a]) == oz.py.is_goal_state(nxt)  # vacuously true


def test_cpp_known_answers():
    """cpp/test/test_pushworld_puzzle.cc:260-394 (trivial.pwp walk), cpp/test/search/
    test_best_first_search.cc:117 (no_solution.pwp has exactly 9 reachable states) and :122
    (the shortest plan of trivial.pwp is R, D, R, U)."""
    from pushworld_amd.puzzle import PushWorldPuzzle

    L, R, U, D = 0, 1, 2, 3
    pz = PushWorldPuzzle(os.path.join(CPP, "trivial.pwp"), order="cpp")
    state = np.array([p2d(pz.initial_state)], dtype=np.int32)
    walk = [(L, (1, 2), (2, 2), False), (U, (1, 2), (2, 2), False), (D, (1, 2), (2, 2), False),
            (R, (2, 2), (3, 2), False), (R, (2, 2), (3, 2), False), (D, (2, 3), (3, 2), False),
            (D, (2, 3), (3, 2), False), (R, (3, 3), (3, 2), False), (R, (3, 3), (3, 2), False),
            (U, (3, 2), (3, 1), True), (U, (3, 2), (3, 1), True)]
    for a, agent, m0, is_goal in walk:
        succ, moved, goal = pz.expand4(state)
        nxt = succ[0, a].cpu().numpy()
        assert nxt.tolist() == p2d([agent, m0])
        assert bool(goal[0, a].item()) == is_goal
        changed = nxt.tolist() != state[0].tolist()
        assert (int(moved[0, a].item()) != 0) == changed
        state = nxt[None].astype(np.int32)

    ns = PushWorldPuzzle(os.path.join(CPP, "no_solution.pwp"), order="cpp")
    order, succ, moved, goal, n = bfs(ns, 10000)
    assert len(order) == 9 and n == 9 and not goal.any()

    # breadth-first distance to the first goal state of trivial.pwp is 4 and the plan is unique
    order, succ, moved, goal, n = bfs(pz, 10000)
    index = {s: i for i, s in enumerate(order)}
    depth = {0: 0}
    plans = {0: [""]}
    for i in range(n):
        for a in range(4):
            j = index[tuple(int(v) for v in succ[i, a])]
            if j not in depth:
                depth[j] = depth[i] + 1
                plans[j] = [p + "LRUD"[a] for p in plans[i]]
            elif depth[j] == depth[i] + 1 and j != i:
                plans[j] += [p + "LRUD"[a] for p in plans[i]]
    goal_states = {index[tuple(int(v) for v in succ[i, a])] for i in range(n) for a in range(4) if goal[i, a]}
    best = min(depth[g] for g in goal_states)
    assert best == 4
    assert sorted(p for g in goal_states if depth[g] == best for p in plans[g]) == ["RDRU"]


def test_cpp_hand_built_collision_cases():
    """cpp/test/test_pushworld_puzzle.cc:84-257 on the HIP path: the reference's hand-built ObjectCollisions cases
    (tests/cpp_cases.py) through pw_expand4 -- successor, moved_object_indices (as a bit mask) and satisfiesGoal."""
    import sys

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import cpp_cases
    from pushworld_amd.puzzle import PushWorldPuzzle

    n = 0
    for name, text, steps in cpp_cases.movement_cases():
        pz = PushWorldPuzzle(text=text, order="cpp")
        assert tuple(pz.initial_state) == steps[0][0], name
        states = np.array([p2d(st) for st, _, _, _ in steps], dtype=np.int32)
        succ, moved, goal = pz.expand4(states)
        succ, moved = succ.cpu().numpy(), moved.cpu().numpy().astype(np.uint32)
        for i, (state, action, want, want_moved) in enumerate(steps):
            assert succ[i, action].tolist() == p2d(want), (name, state, action)
            if want_moved is not None:
                assert int(moved[i, action]) == sum(1 << k for k in want_moved), (name, state, action)
            assert pz.get_next_state(state, action) == want            # the single-state surface (pw_step)
            n += 1
    assert n == 22
    for name, text, checks in cpp_cases.goal_cases():
        pz = PushWorldPuzzle(text=text, order="cpp")
        states = np.array([p2d(st) for st, _ in checks], dtype=np.int32)
        succ, moved, goal = pz.expand4(states)
        succ, moved, goal = succ.cpu().numpy(), moved.cpu().numpy().astype(np.uint32), goal.cpu().numpy()
        for i, (state, want) in enumerate(checks):
            # an action that moves at most the agent leaves the goal objects where the reference test put them:
            # the successor's flag is satisfiesGoal of exactly those positions
            quiet = [a for a in range(4) if int(moved[i, a]) in (0, 1)]
            assert quiet, (name, state)
            for a in quiet:
                assert succ[i, a, 1:].tolist() == p2d(state[1:]) and bool(goal[i, a]) == want, (name, state, a)


def test_expand_large_frontier_consistency(golden):
    """>= 100k states of 'level1/2 Obstacle': expand4 agrees with 4 single-action pw_step
    launches on the same states (two different kernels, same dynamics)."""
    import torch

    from pushworld_amd.puzzle import PushWorldPuzzle
    from pushworld_amd.vec_env import VecPushWorld

    text = golden.text("bench:level1/2 Obstacle.pwp")
    pz = PushWorldPuzzle(text=text, order="cpp")
    order, *_ = bfs(pz, 120000)
    states = np.array(order, dtype=np.int32)
    F, n = states.shape
    succ, moved, goal = pz.expand4(states)
    succ = succ.cpu().numpy()
    vec = VecPushWorld([pz], F, observation=None, device=0)
    vec.reset()
    base = np.zeros((F, vec.num_objects_padded, 2), np.int8)
    base[:, :n, 0] = states // 10000
    base[:, :n, 1] = states % 10000
    for a in range(4):
        vec.set_states(base)
        _, _, term, _ = vec.step(torch.full((F,), a, dtype=torch.uint8, device=vec.device))
        got = vec.states()[:, :n].astype(np.int32)
        assert (got[:, :, 0] * 10000 + got[:, :, 1] == succ[:, a]).all()
        assert (term.cpu().numpy() == goal[:, a].cpu().numpy()).all()


@pytest.mark.parametrize("key", ["bench:level1/2 Obstacle.pwp", "bench:level2/Pull Dont Push.pwp",
                                 "bench:level4/Four Pistons.pwp"])
def test_million_state_frontier_against_the_oracle(golden, key):
    """C5 at the size BASELINE.json names: >= 1 M distinct reachable states (all of them if the puzzle has fewer)
    in the C++ object order, collected by the GPU breadth-first search; pw_expand4's four successors, moved masks
    (= moved_object_indices, pushworld_puzzle.cc:446-457) and goal flags of EVERY state equal the C oracle's
    (tables + LIFO frontier, OpenMP over states)."""
    import torch

    from oracle import c_oracle
    from pushworld_amd.puzzle import PushWorldPuzzle
    from pushworld_amd.search import BreadthFirstSearch

    text = golden.text(key)
    pz = PushWorldPuzzle(text=text, order="cpp")
    oz = c_oracle.COraclePuzzle(text, order="cpp")
    target = 1_000_000
    bfs_gpu = BreadthFirstSearch(pz, max_states=6_000_000)
    bfs_gpu.begin()
    while bfs_gpu.total_states < target and not bfs_gpu.exhausted:
        bfs_gpu.expand()
    F = bfs_gpu.total_states
    assert F >= target or bfs_gpu.exhausted
    xy = bfs_gpu.states(0, F)
    bfs_gpu.close()
    states = (xy[:, :, 0].astype(np.int64) * 10000 + xy[:, :, 1]).astype(np.int32)
    assert len(np.unique(states, axis=0)) == F          # the search's closed set: all distinct
    succ, moved, goal = pz.expand4(states)
    want_succ, want_moved, want_goal = c_oracle.expand4_batch(oz, states)
    got_succ = succ.cpu().numpy()
    bad = np.nonzero((got_succ != want_succ).any(axis=(1, 2)))[0]
    assert bad.size == 0, (key, bad[:5])
    assert (moved.cpu().numpy().astype(np.uint32) == want_moved).all()
    assert (goal.cpu().numpy() == want_goal).all()
    # the layers the search itself produced are closed under expansion up to the last complete layer
    assert want_moved.any() and got_succ.shape == (F, 4, pz.num_movables)


def test_pair_tables_sized_per_pair_against_the_oracle():
    """pw_expand4_v2_kernel<., ., ., true>: byte pair tables sized per pair (PwPushDir::pairp_off), chosen where the set-wide
    tables exceed 16 KB -- 44 benchmark puzzles with 7 .. 16 movables, among them every one of round 4's slow tail but `Clean
    Sweep`.  For every such puzzle a breadth-first frontier of >= 140 000 states (C++ object order): successors, moved masks and
    goal flags of every state equal the C oracle's, and the kernel it replaces (PW_OPT_EXPAND_PAIR_DIMS never: set-wide tables, or
    the lane kernel where those do not fit LDS) agrees word for word."""
    from oracle import c_oracle
    from pushworld_amd import benchmark_data as bd
    from pushworld_amd.puzzle import PushWorldPuzzle
    from pushworld_amd.search import BreadthFirstSearch

    checked = 0
    for lv in (1, 2, 3, 4):
        for path in bd.level_paths(lv):
            with open(path) as f:
                text = f.read()
            oz = c_oracle.COraclePuzzle(text, order="cpp")
            n = oz.num_movables
            dims = [(1 + max(c[0] for c in s) - min(c[0] for c in s), 1 + max(c[1] for c in s) - min(c[1] for c in s)) for s in oz.py.shapes]
            uniform = n * n * (2 * max(d[1] for d in dims) + 2) * (2 * max(d[0] for d in dims) + 2)
            if not (7 <= n <= 16 and uniform > 16384):
                continue
            pz = PushWorldPuzzle(text=text, order="cpp")
            bfs_gpu = BreadthFirstSearch(pz, max_states=400_000)
            bfs_gpu.begin()
            try:
                while bfs_gpu.total_states < 140_000 and not bfs_gpu.exhausted:
                    bfs_gpu.expand()
            except ValueError:  # the store filled up inside a layer: what is in it is enough
                pass
            F = min(bfs_gpu.total_states, 200_000)
            xy = bfs_gpu.states(0, F)
            bfs_gpu.close()
            if F < 131_072:  # (a small state space: repeated up to the size from which pw_expand4 runs one lane per state)
                xy = np.tile(xy, (-(-140_000 // F), 1, 1))[:140_000]
                F = len(xy)
            states = np.ascontiguousarray((xy[:, :, 0].astype(np.int64) * 10000 + xy[:, :, 1]).astype(np.int32))
            eng = pz._engine()
            eng.set_option("expand_pair_dims", "auto")
            succ, moved, goal = (t.cpu().numpy() for t in pz.expand4(states))
            eng.set_option("expand_pair_dims", "never")
            succ0, moved0, goal0 = (t.cpu().numpy() for t in pz.expand4(states))
            eng.set_option("expand_pair_dims", "auto")
            assert (succ == succ0).all() and (moved == moved0).all() and (goal == goal0).all(), path
            want_succ, want_moved, want_goal = c_oracle.expand4_batch(oz, states)
            assert (succ == want_succ).all() and (moved.astype(np.uint32) == want_moved).all() and (goal == want_goal).all(), path
            checked += 1
    assert checked >= 40


def test_wide_work_word_17_to_20_movables_against_the_oracle():
    """pw_expand4_v2_kernel with a 128-bit work word (4 bits per movable and action): 17 .. 20 movables, per-pair byte tables
    (round 5; `Clean Sweep`, 19 movables, was the one benchmark puzzle left to the lane kernel).  `Clean Sweep` and seeded random
    puzzles with 17, 18, 19 and 20 movables (C++ object order): breadth-first frontiers of >= 140 000 states -- successors,
    moved-object masks (bits 16 .. 19 among them) and goal flags of every state against the C oracle, and word for word against
    the lane kernel (PW_OPT_EXPAND_LDS_TABLES never)."""
    from oracle import c_oracle
    from pushworld_amd import benchmark_data as bd
    from pushworld_amd.puzzle import PushWorldPuzzle
    from pushworld_amd.search import BreadthFirstSearch

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from puzzle_gen import many_movables_text

    texts = []
    for lv in (1, 2, 3, 4):
        for path in bd.level_paths(lv):
            with open(path) as f:
                text = f.read()
            if 17 <= c_oracle.COraclePuzzle(text, order="cpp").num_movables <= 20:
                texts.append((os.path.basename(path), text))
    assert any(name.startswith("Clean Sweep") for name, _ in texts)
    rng = np.random.default_rng(1719)
    for n in (17, 18, 19, 20, 20):
        texts.append((f"random{n}", many_movables_text(rng, n)))
    high_moves = 0
    for name, text in texts:
        oz = c_oracle.COraclePuzzle(text, order="cpp")
        pz = PushWorldPuzzle(text=text, order="cpp")
        bfs_gpu = BreadthFirstSearch(pz, max_states=400_000)
        bfs_gpu.begin()
        try:
            while bfs_gpu.total_states < 140_000 and not bfs_gpu.exhausted:
                bfs_gpu.expand()
        except ValueError:  # the store filled up inside a layer: what is in it is enough
            pass
        F = min(bfs_gpu.total_states, 200_000)
        xy = bfs_gpu.states(0, F)
        bfs_gpu.close()
        if F < 140_000:
            xy = np.tile(xy, (-(-140_000 // F), 1, 1))[:140_001]  # (a ragged last tile)
            F = len(xy)
        states = np.ascontiguousarray((xy[:, :, 0].astype(np.int64) * 10000 + xy[:, :, 1]).astype(np.int32))
        eng = pz._engine()
        eng.set_option("expand_lds_tables", "auto")
        succ, moved, goal = (t.cpu().numpy() for t in pz.expand4(states))
        eng.set_option("expand_lds_tables", "never")
        succ0, moved0, goal0 = (t.cpu().numpy() for t in pz.expand4(states))
        eng.set_option("expand_lds_tables", "auto")
        assert (succ == succ0).all() and (moved == moved0).all() and (goal == goal0).all(), name
        want_succ, want_moved, want_goal = c_oracle.expand4_batch(oz, states)
        assert (succ == want_succ).all() and (moved.astype(np.uint32) == want_moved).all() and (goal == want_goal).all(), name
        high_moves += int((want_moved >> 16 != 0).sum())
    assert high_moves > 100  # movables 16 .. 19 were pushed: the upper half of the word is exercised


def test_cpp_order_with_many_ids_against_the_reference():
    """tests/golden/golden_cpp_order.json: 24 puzzles with 10-13 movables whose ids run past 10 ("m10" < "m2" in the C++ order of
    pushworld_puzzle.cc:262-321), expectations from the PYTHON reference rearranged by that rule: pw_expand4's successors,
    moved-object masks (pushworld_puzzle.cc:446-457) and goal flags of the sampled states, and the engine's object order itself."""
    import json
    import os

    from pushworld_amd.puzzle import PushWorldPuzzle

    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_cpp_order.json")) as f:
        fx = json.load(f)
    pushes = 0
    for key, ent in fx.items():
        pz = PushWorldPuzzle(text=ent["text"], order="cpp")
        assert [list(p) for p in pz.initial_state] == ent["states_cpp"][0], key
        assert [list(p) for p in pz.goal_state] == ent["goal_state_cpp"], key
        smp = ent["expand"]
        st = np.array([ent["states_cpp"][s["t"]] for s in smp], dtype=np.int64)
        states = (st[:, :, 0] * 10000 + st[:, :, 1]).astype(np.int32)
        succ, moved, goal = (t.cpu().numpy() for t in pz.expand4(states))
        want = np.array([s["succ"] for s in smp], dtype=np.int64)
        assert (succ == (want[..., 0] * 10000 + want[..., 1])).all(), key
        assert (moved.astype(np.uint32) == np.array([s["moved"] for s in smp], dtype=np.uint32)).all(), key
        assert (goal.astype(bool) == np.array([s["goal"] for s in smp])).all(), key
        pushes += int(sum(bin(m).count("1") > 1 for s in smp for m in s["moved"]))
        # and the whole walk through the single-state API in this order
        s = pz.initial_state
        for t, a in enumerate(ent["actions"][:60]):
            s = pz.get_next_state(s, a)
            assert [list(p) for p in s] == ent["states_cpp"][t + 1], (key, t)
    assert pushes >= 50

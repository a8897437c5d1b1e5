"""-m gpu: every kernel instance and launch shape of pw_expand4's LDS-table kernels (pw_expand4_v2_kernel, pw_expand4_v2w_kernel,
pw_expand4_v2q_kernel) against the C oracle.  The engine's expansion options only choose which kernel computes a result, never
the result: for a corpus with every movable count 2 .. 20, frontier sizes around every tile / block / grid boundary, and a
pairwise-covering set of those options, every launch must write exactly the oracle's successors, moved masks and goal flags into
every state of its views and nothing outside them.  PW_OPT_EXPAND_FORM reports which instance ran; the forms seen must include
the table below."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from puzzle_gen import many_movables_text  # noqa: E402

# Benchmark puzzles (C++ object order), by movable count; the set-wide byte tables (auto: also the per-pair ones where the
# set-wide ones exceed 16 KB) -- comments: which forms each one is here for
BENCH = [
    "level1/A Tight Squeeze.pwp",        # N = 2
    "level1/2 Obstacle.pwp",             # 3
    "level1/At Crossroads.pwp",          # 4
    "level1/Building Blocks.pwp",        # 5
    "level1/Friendly Obstacle.pwp",      # 6
    "level1/Carry The Bucket.pwp",       # 7 set-wide
    "level2/Dinner Table.pwp",           # 7 per-pair
    "level2/Bubbles.pwp",                # 8 both
    "level2/Encircle.pwp",               # 8: set-wide tables of 64 KB -- one workgroup per CU, 8 wavefronts (kLanes 32)
    "level1/Dont Get Distracted.pwp",    # 9 set-wide
    "level1/Pulling.pwp",                # 9 per-pair
    "level2/Pinata.pwp",                 # 10 both
    "level3/Diagonal Maze.pwp",          # 11 set-wide
    "level3/Inner Eye.pwp",              # 11 per-pair
    "level4/Four Pistons.pwp",           # 12 set-wide
    "level4/Hourglass.pwp",              # 12 per-pair
    "level3/Yin Yang.pwp",               # 13, kPipe 0
    "level4/Mind The Gap.pwp",           # 13 per-pair only (no set-wide tables: "never" runs the lane kernel)
    "level3/Chain Link Tunnel.pwp",      # 14, kPipe 0
    "level4/Pinhole Lock.pwp",           # 14: set-wide tables of 96 KB, 8 wavefronts (kLanes 16)
    "level4/Tool Chain.pwp",             # 15, kPipe 0
    "level2/Simultaneous Obstacle Removal.pwp",  # 16, both; set-wide: 8 wavefronts
    "level2/Clean Sweep.pwp",            # 19 (v2q)
]

# Seeded random puzzles for what the benchmark does not have
SYNTH = {
    # kPipe 1 needs the tables and 4 wavefronts' staging of whole tiles within 78 KB: at 13 .. 15 movables only tables of a few
    # KB fit (1-cell movables on small grids); with one 4 x 4 movable the set-wide tables exceed 16 KB -> the per-pair ones
    "n13": lambda r: many_movables_text(r, 13, cols=8, rows=6, cells=(1, 1)),
    "n13pd": lambda r: many_movables_text(r, 13, cols=10, rows=8, cells=(1, 1), big=[(4, 4)]),
    "n14": lambda r: many_movables_text(r, 14, cols=8, rows=6, cells=(1, 1)),
    "n14pd": lambda r: many_movables_text(r, 14, cols=10, rows=8, cells=(1, 1), big=[(4, 4)]),
    "n15": lambda r: many_movables_text(r, 15, cols=8, rows=6, cells=(1, 1)),
    "n15pd": lambda r: many_movables_text(r, 15, cols=10, rows=8, cells=(1, 1), big=[(4, 4)]),
    # 6 movables, one of 20 x 20 cells: set-wide tables of 62 KB -> 8 wavefronts with kLanes 64
    "n6wide": lambda r: many_movables_text(r, 6, cols=30, rows=26, big=[(20, 20)]),
    # a 62-column grid (60 + the border walls: the widest with tables) with the small movables in its right-most 10 columns,
    # two 24 x 24 movables: per-pair tables of 42 KB + 16 KB of wall tables -> 8 wavefronts, per-pair (kLanes 32); set-wide
    # tables do not exist ("never": the lane kernel)
    "n12wide62": lambda r: many_movables_text(r, 12, cols=60, rows=40, big=[(24, 24), (24, 24)], x_min=50),
    "n16wide62": lambda r: many_movables_text(r, 16, cols=60, rows=40, big=[(20, 20), (20, 20)]),  # ... kLanes 16
    # 17 .. 20 movables (v2q; Clean Sweep has 19), and puzzles where (nearly) every movable has a goal
    "n17": lambda r: many_movables_text(r, 17),
    "n18": lambda r: many_movables_text(r, 18, goal_p=1.0),
    "n20": lambda r: many_movables_text(r, 20, goal_p=1.0),
    "n9goals": lambda r: many_movables_text(r, 9, goal_p=1.0),
}

# One workgroup per CU with 8 wavefronts (pw_expand4_v2w_kernel) for every N that can reach it: tables so large that 4 wavefronts
# with their staging need more than 78 KB of LDS while 8 still fit in 156 KB.  One L-shaped movable of w x h cells (movables at most
# 32 wide: a row of a pair table is one uint64) -- set-wide tables (2 h + 2) x (2 w + 2) x N x N bytes, run with
# expand_pair_dims "never" -- or one or two of them with per-pair tables (at most 64 KB; "auto").  name: (seed, movables, L shapes,
# columns, rows); the benchmark and the puzzles above already give set-wide 6, 8, 14, 16 and per-pair 12, 16.
WIDE = {
    "w3": (5003, 3, [(32, 58)], 40, 60), "w4": (5004, 4, [(29, 29)], 59, 59), "w5": (5005, 5, [(23, 23)], 31, 31),
    "w7": (5007, 7, [(17, 17)], 33, 33), "w9": (5009, 9, [(12, 12)], 42, 42), "w10": (5010, 10, [(10, 10)], 40, 40),
    "w11": (5011, 11, [(9, 9)], 39, 39), "w12": (5012, 12, [(8, 8)], 38, 38), "w13": (5013, 13, [(9, 9)], 25, 25),
    "w15": (5015, 15, [(7, 7)], 37, 37),
    "w7pd": (5107, 7, [(32, 44)] * 2, 60, 60), "w8pd": (5108, 8, [(31, 31)] * 2, 51, 60), "w9pd": (5109, 9, [(28, 28)] * 2, 54, 60),
    "w10pd": (5110, 10, [(25, 25)] * 2, 53, 60), "w11pd": (5111, 11, [(32, 32)], 60, 60), "w13pd": (5113, 13, [(31, 31)], 60, 60),
    "w14pd": (5114, 14, [(28, 28)], 58, 58), "w15pd": (5115, 15, [(25, 25)], 55, 55),
}

# Launch options: a pairwise-covering set of rows (every value of each option meets every value of every other in some row)
FACTORS = {
    "expand_prefetch": (-1, 0, 2),
    "expand_tile_order": (0, 1, 2, 3),
    "expand_groups_per_cu": (0, 1, 7, 64),
    "expand_wg_waves": (0, 4, 8),
    "expand_pair_dims": ("auto", "never"),
}
DEFAULTS = {"expand_prefetch": -1, "expand_tile_order": 0, "expand_groups_per_cu": 0, "expand_wg_waves": 0, "expand_pair_dims": 0,
            "step_kernel": 0}


def _pairs(row):
    named = list(zip(FACTORS, row))
    return set(itertools.combinations(named, 2))


def pairwise_rows():
    """Greedy covering array (deterministic): the defaults first, then the row of the full product covering most missing pairs."""
    todo = set()
    for a, b in itertools.combinations(FACTORS, 2):
        todo |= {((a, va), (b, vb)) for va in FACTORS[a] for vb in FACTORS[b]}
    rows = [(-1, 0, 0, 0, "auto")]
    todo -= _pairs(rows[0])
    product = list(itertools.product(*FACTORS.values()))
    while todo:
        best = max(product, key=lambda r: len(_pairs(r) & todo))
        rows.append(best)
        todo -= _pairs(best)
    return rows


def test_pairwise_rows_cover_every_pair():
    rows = pairwise_rows()
    want = set()
    for a, b in itertools.combinations(FACTORS, 2):
        want |= {((a, va), (b, vb)) for va in FACTORS[a] for vb in FACTORS[b]}
    got = set().union(*(_pairs(r) for r in rows))
    assert got == want and len(rows) <= 24


# What the matrix must reach: (family, N, kPipe, kNT, kPD, wavefronts per workgroup)
EXPECTED = set()
for _n in range(2, 17):
    EXPECTED.add(("v2", _n, 0, 1, 0, 4))
for _n in range(2, 16):
    EXPECTED |= {("v2", _n, 1, 1, 0, 4), ("v2", _n, 1, 0, 0, 4)}
# kPipe 1 at N = 16 cannot be reached: a wavefront stages a whole tile -- 64 rows of 16 pieces + 64 pieces of padding + 1 =
# 1 089 x 16 = 17 424 bytes, + 64 x 9 x 4 = 2 304 bytes of positions = 19 728 bytes; 4 wavefronts take 78 912 of the 79 872 bytes
# (78 KB) the host allows a pipelined workgroup, leaving 960 bytes for tables that are at least 16 x 16 x 16 = 4 096 bytes (set-wide,
# 1-cell movables) or 16 x 16 x 4 = 1 024 bytes of descriptors alone (per-pair): the host switches the pipeline off.
for _n in range(7, 17):
    EXPECTED.add(("v2", _n, 0, 1, 1, 4))
for _n in range(7, 16):
    EXPECTED.add(("v2", _n, 1, 1, 1, 4))  # (per-pair instances have no plain-store variant: kNT = 1 whatever the tile order)
# 8 wavefronts (one workgroup per CU: more than 78 KB of LDS with 4): set-wide tables at 3 .. 16 movables, per-pair ones (which only
# exist from 7 movables on) at 7 .. 16.  N = 2 cannot be reached: 4 wavefronts stage 4 x 2 448 bytes, so the tables would have to
# exceed 79 872 - 9 792 = 70 080 bytes, and the largest set-wide tables of two movables are 2 x 2 x (2 x 62 + 2) x (2 x 32 + 2) =
# 33 264 bytes (at most 62 rows, 32 columns) plus 2 x 66 x 8 x 4 = 4 224 bytes of wall tables.
for _n in range(3, 17):
    EXPECTED.add(("v2w", _n, 0, 1, 0, 8))
for _n in range(7, 17):
    EXPECTED.add(("v2w", _n, 0, 1, 1, 8))
for _n in range(17, 21):
    EXPECTED.add(("v2q", _n, 0, 1, 1, 4))


def _states(pz, n_max):
    """Distinct reachable states of a breadth-first search (C++ object order), Position2D int32 [F, N]."""
    from pushworld_amd.search import BreadthFirstSearch

    bfs = BreadthFirstSearch(pz, max_states=4 * n_max)
    bfs.begin()
    try:
        while bfs.total_states < n_max and not bfs.exhausted:
            bfs.expand()
    except ValueError:  # the store filled up inside a layer: what is in it is enough
        pass
    F = min(bfs.total_states, n_max)
    xy = bfs.states(0, F)
    bfs.close()
    return (xy[:, :, 0].astype(np.int64) * 10000 + xy[:, :, 1]).astype(np.int32)


SENT_SUCC, SENT_MOVED, SENT_GOAL = -123456789, -0x5A5A5A5B, 0xA5
GUARD = 64  # elements of sentinel before and after every view (a multiple of 4: the views stay 16-byte aligned)


@pytest.mark.gpu
def test_every_expand4_form_against_the_oracle():
    import torch

    from oracle import c_oracle
    from pushworld_amd import _capi
    from pushworld_amd import benchmark_data as bd
    from pushworld_amd.puzzle import PushWorldPuzzle

    dev = "cuda:0"
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    # expand_groups_per_cu 1: at most ncu workgroups of at most 8 wavefronts -- 2 x 8 x ncu + 8 tiles give every wavefront at
    # least two (also with the tile order by XCD: 2 ncu + 1 tiles per eighth, ncu wavefronts per XCD), the last one ragged
    persistent = 64 * (2 * 8 * ncu + 8) - 13
    sizes = [1, 2, 63, 64, 65, 255, 256, 257, 1000, 1792, 2047, 2048, 2049, persistent]
    f_max = max(sizes)
    rows = pairwise_rows()

    corpus = []
    for rel in BENCH:
        with open(os.path.join(bd.BENCHMARK_PUZZLES_PATH, rel)) as f:
            corpus.append((rel, f.read()))
    for i, (name, make) in enumerate(SYNTH.items()):
        corpus.append((name, make(np.random.default_rng(4100 + i))))
    for name, (seed, n, big, cols, rows_) in WIDE.items():
        corpus.append((name, many_movables_text(np.random.default_rng(seed), n, cols=cols, rows=rows_, big=big)))
    assert sorted({c_oracle.COraclePuzzle(t, order="cpp").num_movables for _, t in corpus}) == list(range(2, 21))

    seen = set()         # (family, N, kPipe, kNT, kPD, waves)
    grids = set()        # (family, tile order, persistent)
    launches = 0
    small_xcd_grids = []
    for name, text in corpus:
        oz = c_oracle.COraclePuzzle(text, order="cpp")
        pz = PushWorldPuzzle(text=text, order="cpp")
        N = oz.num_movables
        base = _states(pz, 4096)
        states_np = np.ascontiguousarray(np.tile(base, (-(-f_max // len(base)), 1))[:f_max])
        w_succ, w_moved, w_goal = c_oracle.expand4_batch(oz, states_np)
        want = [torch.as_tensor(a).to(dev) for a in (w_succ, w_moved.view(np.int32), w_goal)]
        states = torch.as_tensor(states_np).to(dev)
        succ_raw = torch.empty(2 * GUARD + f_max * 4 * N, dtype=torch.int32, device=dev)
        moved_raw = torch.empty(2 * GUARD + f_max * 4, dtype=torch.int32, device=dev)
        goal_raw = torch.empty(2 * GUARD + f_max * 4, dtype=torch.uint8, device=dev)
        eng = pz._engine()
        try:
            eng.set_option("step_kernel", "lane")  # (the LDS kernels at every frontier size, not from 131 072 states on)
            for row in rows:
                for key, value in zip(FACTORS, row):
                    eng.set_option(key, value)
                for F in sizes:
                    raws = (succ_raw, moved_raw, goal_raw)
                    widths = (4 * N, 4, 4)
                    for raw, w, s in zip(raws, widths, (SENT_SUCC, SENT_MOVED, SENT_GOAL)):
                        raw[:2 * GUARD + F * w].fill_(s)
                    views = [raw[GUARD:GUARD + F * w].view((F, 4, N) if w > 4 else (F, 4)) for raw, w in zip(raws, widths)]
                    eng.expand4(0, states[:F], *views)
                    launches += 1
                    form = _capi.decode_expand_form(eng.get_option("expand_form"))
                    where = (name, F, dict(zip(FACTORS, row)), form)
                    assert form is not None and form["n"] == N, where
                    if form["family"] in ("v2", "v2w", "v2q"):
                        seen.add(tuple(form[k] for k in ("family", "n", "pipe", "nt", "pd", "waves")))
                        grids.add((form["family"], form["tile_order"], form["persistent"]))
                    bad = torch.stack([
                        (views[0] != want[0][:F]).any(), (views[1] != want[1][:F]).any(), (views[2] != want[2][:F]).any(),
                        *[(raw[:GUARD] != s).any() for raw, s in zip(raws, (SENT_SUCC, SENT_MOVED, SENT_GOAL))],
                        *[(raw[GUARD + F * w:2 * GUARD + F * w] != s).any()
                          for raw, w, s in zip(raws, widths, (SENT_SUCC, SENT_MOVED, SENT_GOAL))],
                    ]).cpu().tolist()
                    if any(bad):
                        wrong = ((views[0] != want[0][:F]).flatten(1).any(1) | (views[1] != want[1][:F]).any(1)
                                 | (views[2] != want[2][:F]).any(1)).nonzero().flatten().cpu().tolist()
                        unwritten = (views[0] == SENT_SUCC).flatten(1).all(1).nonzero().flatten().cpu().tolist()
                        raise AssertionError(
                            f"{where}: {len(wrong)} of {F} states differ from the oracle (first {wrong[:8]}); {len(unwritten)} "
                            f"still hold the sentinel (states {unwritten[:1]} .. {unwritten[-1:]}); [succ, moved, goal, guards "
                            f"before x 3, guards after x 3] wrong: {bad}")
                    if form["family"] in ("v2", "v2w", "v2q") and form["tile_order"] == 1 and form["groups"] < 8:
                        small_xcd_grids.append(where)  # (the tile order by XCD: workgroup b sweeps eighth b mod 8 -- it needs all eight)
        finally:
            for key, value in DEFAULTS.items():
                eng.set_option(key, value)
        # (raw reads: expand_prefetch's default is -1, which get_option would take for an error code)
        assert {k: _capi.lib.pw_engine_get_option(eng.handle, _capi.OPTIONS[k]) for k in DEFAULTS} == DEFAULTS
    assert not small_xcd_grids, small_xcd_grids[:4]
    missing = sorted(EXPECTED - seen)
    assert not missing, f"forms never launched: {missing}"
    # both tile orders on persistent and on non-persistent grids (8 wavefronts: persistent grids -- their tables, beyond 53 KB,
    # are beyond what the host gives a grid of a few tiles per wavefront; at least what is required, whatever else ran)
    both = {(0, 0), (0, 1), (1, 0), (1, 1)}
    for fam, want_grids in (("v2", both), ("v2q", both), ("v2w", {(0, 1), (1, 1)})):
        assert want_grids <= {(o, p) for f, o, p in grids if f == fam}, (fam, sorted(grids))
    assert launches == len(corpus) * len(rows) * len(sizes)

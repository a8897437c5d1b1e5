"""Measures the walk regions and push moves (pw_walk_regions / pw_walk_pushes) and the search over pushes built on
them, and prints the figures kept in profiles/walk.txt.

    python tools/bench_walk.py [--envs 65536] [--puzzles 2000] [--repeats 3] > profiles/walk.txt

  (a) both calls on --envs live environments of the C3 set (the 68 Level-1 puzzles, environments grouped by puzzle, 20 random
      steps from the reset);
  (b) both calls on the initial states of the --puzzles generated Level-0 puzzles of tools/bench_solution_batch.py (K13);
  (c) search.PushSearch.solve against search.BreadthFirstSearch.solve on the same puzzles: states closed by each, and the time.

Timing: the host clock around synchronised calls, best of --repeats after one warm-up run, every repeat listed.
"""
import argparse
import glob
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pushworld_amd import generate  # noqa: E402
from pushworld_amd.puzzle import PushWorldPuzzle  # noqa: E402
from pushworld_amd.search import BreadthFirstSearch, PushSearch, walk_regions  # noqa: E402
from pushworld_amd.vec_env import VecPushWorld  # noqa: E402

LEVEL1 = os.path.join(ROOT, "pushworld_amd", "data", "puzzles", "level1")
SEARCH = ["Single Obstacle", "Two Goals", "2 Obstacle"]


def timed(fn, repeats):
    """Seconds of every repeat of fn() between two synchronisations, after one warm-up."""
    fn()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def ms(ts):
    return f"best {min(ts) * 1e3:.3f} ms (" + ", ".join(f"{t * 1e3:.3f}" for t in ts) + ")"


def both_calls(vec, label, repeats):
    eng, npad = vec.engine, vec.num_objects_padded
    reg = walk_regions(vec, vec.puzzle_id, vec.pos)
    rows = reg.pushes()
    T, n = rows.num_rows, int(vec.puzzle_id.shape[0])
    size = reg.region_size.double()
    print(f"{label}: {n} states, N_pad {npad}; regions of {size.mean().item():.1f} positions on average "
          f"(largest {int(size.max().item())}), {T} push rows ({T / n:.2f} per state)")

    def regions():
        eng.walk_regions(vec.puzzle_id, vec.pos, None, reg.region_size, reg.canon, reg.offset)

    def pushes():
        eng.walk_pushes(vec.puzzle_id, vec.pos, None, reg.offset, T, rows.item, rows.frm, rows.action, rows.walk, rows.moved,
                        rows.goal, rows.next_pos, rows.dropped)

    t_r, t_p = timed(regions, repeats), timed(pushes, repeats)
    row_bytes = 4 + 2 + 1 + 4 + 4 + 1 + 2 * npad
    print(f"  pw_walk_regions (no maps): {ms(t_r)} = {n / min(t_r):.3e} states/s")
    print(f"  pw_walk_pushes:            {ms(t_p)} = {T / min(t_p):.3e} rows/s, {row_bytes} bytes per row")
    maps = walk_regions(vec, vec.puzzle_id[:4096].contiguous(), vec.pos[:4096].contiguous(), maps=True)
    m = maps.walk_map

    def with_maps():
        eng.walk_regions(maps.puzzle_id, maps.pos, None, maps.region_size, maps.canon, maps.offset, m)

    t_m = timed(with_maps, repeats)
    print(f"  pw_walk_regions with maps, first {m.shape[0]} states ({2 * m.shape[1] * m.shape[2]} bytes per state): {ms(t_m)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--puzzles", type=int, default=2000)
    ap.add_argument("--seed", type=int, default=21)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    print(f"# tools/bench_walk.py --envs {args.envs} --puzzles {args.puzzles} --seed {args.seed} --repeats {args.repeats}")
    print(f"# {torch.cuda.get_device_name(0)}; host clock around synchronised calls, best of {args.repeats} after a warm-up")

    paths = sorted(glob.glob(os.path.join(LEVEL1, "*.pwp")))
    ids = [i * len(paths) // args.envs for i in range(args.envs)]
    vec = VecPushWorld([PushWorldPuzzle(p) for p in paths], args.envs, puzzle_ids=ids, observation=None, max_steps=None)
    vec.reset()
    gen = torch.Generator().manual_seed(args.seed)
    for _ in range(20):
        vec.step(torch.randint(0, 4, (args.envs,), generator=gen, dtype=torch.uint8).to(vec.device))
    both_calls(vec, "(a) C3 set, live states after 20 random steps", args.repeats)
    del vec

    pset, _, _ = generate.generate_level0_set(args.puzzles, random_seed=args.seed)
    vec = VecPushWorld(pset, args.puzzles, puzzle_ids=list(range(args.puzzles)), observation=None, max_steps=None)
    vec.reset()
    both_calls(vec, f"(b) {args.puzzles} generated Level-0 puzzles, initial states", args.repeats)
    del vec

    print("(c) search over pushes against the search move by move (canonical states closed / states closed)")
    for name in SEARCH:
        pz = PushWorldPuzzle(os.path.join(LEVEL1, name + ".pwp"))
        stats = {}

        def push():
            ps = PushSearch(pz)
            plan = ps.solve()
            stats["push"] = (ps.num_states, ps.pushes, len(plan), ps.push_rows)

        def move():
            bfs = BreadthFirstSearch(pz, max_states=1 << 20)
            plan = bfs.solve()
            stats["move"] = (bfs.total_states, len(plan))
            bfs.close()

        t_push, t_move = timed(push, args.repeats), timed(move, args.repeats)
        n_p, pushes, len_p, rows = stats["push"]
        n_m, len_m = stats["move"]
        print(f"  {name}: PushSearch {n_p} canonical states, {pushes} pushes, plan of {len_p} actions, {rows} push rows, {ms(t_push)}")
        print(f"  {' ' * len(name)}  BreadthFirstSearch {n_m} states, plan of {len_m} actions, {ms(t_move)}; "
              f"states x{n_m / n_p:.1f}, time x{min(t_move) / min(t_push):.2f}")


if __name__ == "__main__":
    main()

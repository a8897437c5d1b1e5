"""Measures the breadth-first search over pushes with its closed set on the device (search.PushBreadthFirstSearch,
pw_push_search_*) against the first search over pushes (search.PushSearch, K15: closed set by torch.unique) and
prints the figures kept in profiles/push_search.txt.

    python tools/bench_push_search.py [--repeats 3] > profiles/push_search.txt

  (a) `2 Obstacle` to the goal, also against the search move by move (search.BreadthFirstSearch);
  (b) tests/deep_puzzles.big() to exhaustion;
  (c) tests/deep_puzzles.room3() to exhaustion.

Timing: the host clock around synchronised calls, best of --repeats after one warm-up run, every repeat listed.  A run covers
what a caller pays: creating the search (its store and table), the layers, the plan.
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import deep_puzzles  # noqa: E402
from pushworld_amd.puzzle import PushWorldPuzzle  # noqa: E402
from pushworld_amd.search import BreadthFirstSearch, PushBreadthFirstSearch, PushSearch  # noqa: E402

LEVEL1 = os.path.join(ROOT, "pushworld_amd", "data", "puzzles", "level1")


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


def case(label, pz, stop_at_goal, max_states, repeats, moves=False):
    stats = {}

    def new():
        with PushBreadthFirstSearch(pz, max_states=max_states, stop_at_goal=stop_at_goal) as s:
            plan = s.solve()
            stats["new"] = (s.num_states, len(s.layer_states), s.push_rows, s.largest_region, None if plan is None else len(plan))

    def old():
        s = PushSearch(pz, max_states=max_states)
        plan = s.solve(stop_at_goal=stop_at_goal)
        stats["old"] = (s.num_states, len(s.layer_states), s.push_rows, s.largest_region, None if plan is None else len(plan))

    t_new, t_old = timed(new, repeats), timed(old, repeats)
    n, layers, rows, largest, plan_len = stats["new"]
    print(f"{label}: {n} canonical states, {layers} completed layers, {rows} push rows, largest region {largest}, "
          f"plan of {plan_len} actions; both searches agree on these: {stats['new'] == stats['old']}")
    print(f"  PushBreadthFirstSearch  {ms(t_new)}")
    print(f"  PushSearch              {ms(t_old)}")
    spread = max(max(t_new) - min(t_new), max(t_old) - min(t_old))
    print(f"  PushSearch / PushBreadthFirstSearch = x{min(t_old) / min(t_new):.2f}; best times differ by "
          f"{(min(t_old) - min(t_new)) * 1e3:.3f} ms, the larger spread of the repeats is {spread * 1e3:.3f} ms")
    if moves:
        def move():
            bfs = BreadthFirstSearch(pz, max_states=1 << 20)
            plan = bfs.solve()
            stats["move"] = (bfs.total_states, len(plan))
            bfs.close()

        t_move = timed(move, repeats)
        print(f"  BreadthFirstSearch      {ms(t_move)}: {stats['move'][0]} states move by move, plan of {stats['move'][1]} actions; "
              f"PushBreadthFirstSearch / BreadthFirstSearch = x{min(t_new) / min(t_move):.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    print(f"# tools/bench_push_search.py --repeats {args.repeats}")
    print(f"# {torch.cuda.get_device_name(0)}; host clock around synchronised calls, best of {args.repeats} after a warm-up")
    case("(a) 2 Obstacle to the goal", PushWorldPuzzle(os.path.join(LEVEL1, "2 Obstacle.pwp")), True, 1 << 20, args.repeats, moves=True)
    case("(b) big to exhaustion", PushWorldPuzzle(text=deep_puzzles.big()), False, 1 << 20, args.repeats)
    case("(c) room3 to exhaustion", PushWorldPuzzle(text=deep_puzzles.room3()), False, 1 << 20, args.repeats)


if __name__ == "__main__":
    main()

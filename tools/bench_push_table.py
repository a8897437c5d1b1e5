"""Measures the cost-to-go tables over pushes (search.PushSolutionTable, pw_push_search_solve / pw_push_search_table_query,
DESIGN.md K18) and prints the figures kept in profiles/push_table.txt.

    python tools/bench_push_table.py [--repeats 3] > profiles/push_table.txt

  (a) pw_push_search_solve on tests/deep_puzzles.room3(), next to the exhaustion of room3 that precedes it;
  (b) pw_push_search_solve on tests/deep_puzzles.big(), against search.SolutionTable (the table move by move) on big;
  (c) the query of 65 536 live states of a big-only batch, with the walk maps (action, walk) and without them.

Timing: the host clock around synchronised calls, best of --repeats after one warm-up run, every repeat listed.
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import deep_puzzles  # noqa: E402
from pushworld_amd import _capi  # noqa: E402
from pushworld_amd.puzzle import PushWorldPuzzle  # noqa: E402
from pushworld_amd.search import BreadthFirstSearch, PushBreadthFirstSearch, PushSolutionTable, SolutionTable  # noqa: E402
from pushworld_amd.vec_env import VecPushWorld  # noqa: E402


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


def exhaust_and_solve(label, pz, max_states, repeats):
    """The exhaustion (creating the search, its layers) and, on the exhausted handle, pw_push_search_solve alone."""
    def exhaust():
        with PushBreadthFirstSearch(pz, max_states=max_states, stop_at_goal=False) as s:
            s.solve()

    t_ex = timed(exhaust, repeats)
    with PushBreadthFirstSearch(pz, max_states=max_states, stop_at_goal=False) as s:
        s.solve()
        info = s._handle.solve()
        t_solve = timed(s._handle.solve, repeats)
    print(f"{label}: {info[0]} canonical states, {info[1]} push rows, {info[2]} goal states, {info[3]} dead ends, largest cost {info[4]}")
    print(f"  exhaustion (PushBreadthFirstSearch)  {ms(t_ex)}")
    print(f"  pw_push_search_solve                 {ms(t_solve)}")
    return t_ex, t_solve


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    rep = args.repeats
    print(f"# tools/bench_push_table.py --repeats {rep}")
    print(f"# {torch.cuda.get_device_name(0)}; host clock around synchronised calls, best of {rep} after a warm-up")
    exhaust_and_solve("(a) room3", PushWorldPuzzle(text=deep_puzzles.room3()), 1 << 20, rep)
    big = PushWorldPuzzle(text=deep_puzzles.big())
    t_ex, t_solve = exhaust_and_solve("(b) big", big, 1 << 20, rep)

    def moves():
        SolutionTable(big, max_states=1 << 16).close()

    def pushes():
        PushSolutionTable(big).close()

    t_moves, t_pushes = timed(moves, rep), timed(pushes, rep)
    bfs = BreadthFirstSearch(big, max_states=1 << 16)
    bfs.begin()
    while not bfs.exhausted:
        bfs.expand()
    info = (ctypes.c_int64 * 4)()

    def move_solve():
        _capi.check(_capi.lib.pw_search_solve(bfs.handle, info, bfs._stream()))

    t_msolve = timed(move_solve, rep)
    print(f"  PushSolutionTable (search + solve)   {ms(t_pushes)}")
    print(f"  SolutionTable (search + solve)       {ms(t_moves)}: {int(info[0])} rows move by move")
    print(f"  pw_search_solve alone                {ms(t_msolve)}")
    print(f"  SolutionTable / PushSolutionTable = x{min(t_moves) / min(t_pushes):.2f}; pw_search_solve / pw_push_search_solve = "
          f"x{min(t_msolve) / min(t_solve):.2f}")
    bfs.close()

    B = 65536
    vec = VecPushWorld([big], B, observation=None, max_steps=None, seed=1)
    vec.reset()
    rng = np.random.default_rng(5)
    for _ in range(24):  # a walk of random actions: live states all over the space
        vec.step(torch.as_tensor(rng.integers(0, 4, B).astype(np.uint8), device=vec.device))
    with vec.push_table(0) as tab:
        out = tab.query(None, vec.pos)
        t_maps = timed(lambda: tab.query(None, vec.pos, out=out), rep)
        t_plain = timed(lambda: tab.query(None, vec.pos, out=out, actions=False), rep)
        nodes = int(torch.unique(out.index).numel())
        print(f"(c) query of {B} live states of big ({nodes} distinct nodes, {int((out.cost == -1).sum())} dead ends)")
        print(f"  with the walk maps (action, walk)    {ms(t_maps)}: {B / min(t_maps) * 1e-6:.2f} M states / s")
        print(f"  without them (index, cost, push)     {ms(t_plain)}: {B / min(t_plain) * 1e-6:.2f} M states / s")


if __name__ == "__main__":
    main()

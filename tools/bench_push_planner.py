"""Measures the best-first search over pushes (search.PushBestFirstSearch, pw_push_planner_*) against the
breadth-first search over pushes (search.PushBreadthFirstSearch, K16) and the best-first search move by move
(search.BestFirstSearch("RGD"), K8) and prints the figures kept in profiles/push_planner.txt.

    python tools/bench_push_planner.py [--repeats 3] > profiles/push_planner.txt

  (a) `2 Obstacle`, `Simple Tool` and `Walk Past` at K = 1, 8, 64 and 256: states stored, expansions, rounds and the time of
      a run, against BestFirstSearch("RGD") at the same K and against PushBreadthFirstSearch;
  (b) the 68 Level-1 puzzles at K = 64 with max_states = 2^20 and 2 000 rounds: how many end `solved`.

Timing: the host clock around synchronised calls, best of --repeats after one warm-up run, every repeat listed.  A run covers
what a caller pays: create + begin + run + plan.
"""
import argparse
import glob
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pushworld_amd.puzzle import PushWorldPuzzle  # noqa: E402
from pushworld_amd.search import BestFirstSearch, PushBestFirstSearch, PushBreadthFirstSearch  # noqa: E402

LEVEL1 = os.path.join(ROOT, "pushworld_amd", "data", "puzzles", "level1")
MAX_STATES = 1 << 20


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


def case(name, repeats):
    pz = PushWorldPuzzle(os.path.join(LEVEL1, name + ".pwp"), order="cpp")
    stats = {}

    def layers():
        with PushBreadthFirstSearch(pz, max_states=MAX_STATES) as s:
            plan = s.solve()
            stats["layers"] = (s.num_states, len(s.layer_states) + 1, s.push_rows, None if plan is None else len(plan))

    t_layers = timed(layers, repeats)
    n, depth, rows, plan_len = stats["layers"]
    print(f"{name}")
    print(f"  PushBreadthFirstSearch        {ms(t_layers)}: {n} states, {depth} layers, {rows} push rows, plan of {plan_len} actions")
    for k in (1, 8, 64, 256):
        def pushes():
            with PushBestFirstSearch(pz, batch=k, max_states=MAX_STATES) as s:
                s.begin()
                info = s.run()
                plan = s.plan()
                stats["pushes"] = (info, s.pushes, None if plan is None else len(plan))

        def moves():
            s = BestFirstSearch(pz, heuristic="RGD", batch=k, max_states=MAX_STATES)
            s.begin()
            info = s.run()
            plan = s.plan()
            s.close()
            stats["moves"] = (info, None if plan is None else len(plan))

        def phases():
            """One more run with a synchronisation after every phase: (create, begin, run, plan) in seconds."""
            marks = []

            def mark():
                torch.cuda.synchronize()
                marks.append(time.perf_counter())

            mark()
            with PushBestFirstSearch(pz, batch=k, max_states=MAX_STATES) as s:
                mark()
                s.begin()
                mark()
                s.run()
                mark()
                s.plan()
                mark()
            return [b - a for a, b in zip(marks, marks[1:])]

        t_pushes, t_moves = timed(pushes, repeats), timed(moves, repeats)
        split = phases()
        info, npush, plan_len = stats["pushes"]
        print(f"  K = {k:3d}  PushBestFirstSearch     {ms(t_pushes)}: {info.status}, {info.states} states, {info.expanded} expansions, "
              f"{info.rounds} rounds, {info.push_rows} push rows, plan of {plan_len} actions with {npush} pushes; "
              f"{min(t_pushes) / max(info.rounds, 1) * 1e3:.3f} ms per round with create, begin and plan counted in")
        print("           one more run, phase by phase: " + ", ".join(f"{n} {t * 1e3:.3f} ms" for n, t in
                                                                        zip(("create", "begin", "run", "plan"), split))
              + f"; run / rounds = {split[2] / max(info.rounds, 1) * 1e3:.3f} ms per round")
        info, plan_len = stats["moves"]
        print(f"           BestFirstSearch(RGD)    {ms(t_moves)}: {info.status}, {info.stored} states, {info.expanded} expansions, "
              f"{info.rounds} rounds, plan of {plan_len} actions")
        print(f"           PushBestFirstSearch / PushBreadthFirstSearch = x{min(t_pushes) / min(t_layers):.2f}, "
              f"/ BestFirstSearch(RGD) = x{min(t_pushes) / min(t_moves):.2f}")


def level1(k, rounds):
    paths = sorted(glob.glob(os.path.join(LEVEL1, "*.pwp")))
    ended = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for path in paths:
        with PushBestFirstSearch(PushWorldPuzzle(path, order="cpp"), batch=k, max_states=MAX_STATES) as s:
            s.begin()
            status = s.run(rounds).status
            ended.setdefault(status, []).append(os.path.basename(path)[:-4])
    torch.cuda.synchronize()
    t = time.perf_counter() - t0
    print(f"Level 1 at K = {k}, max_states = 2^20, at most {rounds} rounds: {len(ended.get('solved', []))} of {len(paths)} puzzles end "
          f"solved ({', '.join(f'{len(v)} {s}' for s, v in sorted(ended.items()))}); {t:.2f} s for all of them, one run each")
    for status, names in sorted(ended.items()):
        if status != "solved":
            print(f"  {status}: " + ", ".join(names))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    print(f"# tools/bench_push_planner.py --repeats {args.repeats}")
    print(f"# {torch.cuda.get_device_name(0)}; host clock around synchronised calls, best of {args.repeats} after a warm-up")
    for name in ("2 Obstacle", "Simple Tool", "Walk Past"):
        case(name, args.repeats)
    level1(64, 2000)


if __name__ == "__main__":
    main()

"""Measures the best-first search over pushes of many puzzles or live states in one launch (pw_push_plan_batch_*)
and prints the figures kept in profiles/push_plan_batch.txt.

    python tools/bench_push_plan_batch.py [--rounds 200] [--repeats 3] [--time-limit 0.4] > profiles/push_plan_batch.txt

1. The Level-1 puzzles within the kernel's limits (16 x 16 cells with the border, 8 movables) at K = 1 / 8 / 64, each search capped
   at --rounds rounds and 2^16 states: ONE PushPlanBatch launch against the loop of PushBestFirstSearch (K17) begin + run calls on
   the same puzzles with the same K, cap and max_states -- the capability before this unit.  Both compute the same searches: the
   statuses and the counts are compared before anything is printed.
2. The same puzzles, every search with --time-limit seconds on the device's clock and no cap on the rounds: PushPlanBatch against
   PlanBatch("RGD") move by move (K9), with the solved counts.
3. VecPushWorld.planned_pushes for 4 096 and 65 536 live environments of five Level-1 puzzles after 6 seeded random steps, K = 8,
   at most 64 rounds and 4 096 states per search.

Timing: the host clock around synchronised calls, best of --repeats after one warm-up, every repeat listed.  Not measured here:
per-kernel times and occupancy (no profiler run)."""
import argparse
import glob
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pushworld_amd.puzzle import PushWorldPuzzle  # noqa: E402
from pushworld_amd.search import PlanBatch, PushBestFirstSearch, PushPlanBatch  # noqa: E402
from pushworld_amd.vec_env import VecPushWorld  # noqa: E402

LEVEL1 = os.path.join(ROOT, "pushworld_amd", "data", "puzzles", "level1")
FIVE = ("Single Obstacle", "Two Goals", "2 Obstacle", "Simple Tool", "Walk Past")
MAX_STATES = 1 << 16


def ms(ts):
    return f"best {min(ts) * 1e3:.2f} ms (" + ", ".join(f"{t * 1e3:.2f}" for t in ts) + ")"


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def timed(fn, repeats):
    ts, out = [], None
    for k in range(repeats + 1):  # round 0 is the warm-up
        dt, out = clock(fn)
        if k:
            ts.append(dt)
    return ts, out


def tally(infos):
    counts = {}
    for i in infos:
        counts[i.status] = counts.get(i.status, 0) + 1
    return ", ".join(f"{v} {k}" for k, v in sorted(counts.items()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--time-limit", type=float, default=0.4)
    ap.add_argument("--seed", type=int, default=24)
    args = ap.parse_args()
    print(f"# tools/bench_push_plan_batch.py --rounds {args.rounds} --repeats {args.repeats} --time-limit {args.time_limit} "
          f"--seed {args.seed}")
    print(f"# {torch.cuda.get_device_name(0)}; host clock around synchronised calls, best of {args.repeats} after a warm-up")

    paths = sorted(glob.glob(os.path.join(LEVEL1, "*.pwp")))
    every = [PushWorldPuzzle(p) for p in paths]
    fits = [p for p in every if p._parsed.width <= 16 and p._parsed.height <= 16 and p.num_movables <= 8]
    print(f"Level 1: {len(every)} puzzles, {len(fits)} within 16 x 16 cells with the border and 8 movables")
    for name, group in (("Level 1", every), ("Level 2-4", [PushWorldPuzzle(p) for lv in "234" for p in sorted(glob.glob(
            os.path.join(os.path.dirname(LEVEL1), "level" + lv, "*.pwp")))])):
        with PushPlanBatch(group, max_states=64) as pb:  # (one round each: who is skipped?)
            pb.run(max_rounds=1)
            taken = sum(r[1].status != "skipped" for r in pb.results())
        print(f"  {name}: the kernel takes {taken} of {len(group)} (within the limits and with overlap tables)")

    print(f"1. one launch against the loop of K17 runs; every search at most {args.rounds} rounds and {MAX_STATES} states")
    for K in (1, 8, 64):
        with PushPlanBatch(fits, batch=K, max_states=MAX_STATES) as pb:
            def one_launch():
                pb.run(max_rounds=args.rounds)
                return pb.results()

            t_new, results = timed(one_launch, args.repeats)
        searches = [PushBestFirstSearch(p, batch=K, max_states=MAX_STATES) for p in fits]

        def loop():
            out = []
            for s in searches:
                s.begin()
                out.append(s.run(args.rounds))
            return out

        t_old, infos = timed(loop, args.repeats)
        for s in searches:
            s.close()
        same = sum(tuple(r[1]) == tuple(i) for r, i in zip(results, infos))
        assert same == len(fits), f"{len(fits) - same} searches differ between the two forms"
        device = sum(r[2] for r in results)
        print(f"  K = {K:2d}: {tally([r[1] for r in results])}; the ten info words of all {len(fits)} searches agree")
        print(f"    PushPlanBatch, one launch:        {ms(t_new)}; the searches' own times add up to {device * 1e3:.1f} ms")
        print(f"    PushBestFirstSearch begin + run:  {ms(t_old)}; loop / launch = {min(t_old) / min(t_new):.1f}")

    print(f"2. against PlanBatch('RGD') move by move; every search {args.time_limit} s on the device's clock, no cap on the rounds")
    for K in (1, 8, 64):
        with PushPlanBatch(fits, batch=K, max_states=MAX_STATES) as pb:
            def pushes():
                pb.run(time_limit=args.time_limit)
                return pb.results()

            t_push, r_push = timed(pushes, args.repeats)
        with_moves = PlanBatch(fits, heuristic="RGD", batch=K, max_states=1 << 20)

        def moves():
            with_moves.run(time_limit=args.time_limit)
            return with_moves.results()

        t_move, r_move = timed(moves, args.repeats)
        with_moves.close()
        print(f"  K = {K:2d}: PushPlanBatch {ms(t_push)}: {tally([r[1] for r in r_push])}")
        print(f"          PlanBatch RGD {ms(t_move)}: {tally([r[1] for r in r_move])}")

    print("3. planned_pushes from live states: five puzzles, 6 seeded random steps, K = 8, at most 64 rounds and 4 096 states")
    five = [PushWorldPuzzle(os.path.join(LEVEL1, n + ".pwp")) for n in FIVE]
    for B in (4096, 65536):
        vec = VecPushWorld(five, B, puzzle_ids=[i * 5 // B for i in range(B)], observation=None, max_steps=None)
        vec.reset()
        gen = torch.Generator().manual_seed(args.seed)
        for _ in range(6):
            vec.step(torch.randint(0, 4, (B,), generator=gen, dtype=torch.uint8).to(vec.device))
        with vec.push_planner(batch=8, max_states=1 << 12) as planner:
            ts, q = timed(lambda: vec.planned_pushes(planner, max_rounds=64), args.repeats)
            solved = int((q.pushes >= 0).sum())
            first = int((q.pushes > 0).sum())
            seconds = planner.info()[:, 10].double().sum().item() * 1e-9
        print(f"  {B:6d} environments: {ms(ts)} = {B / min(ts):.3e} plans/s; {solved} solved, {first} with a first push; the "
              f"searches' own times add up to {seconds * 1e3:.1f} ms")
        del vec


if __name__ == "__main__":
    main()

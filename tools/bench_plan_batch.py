#!/usr/bin/env python3
"""Batched best-first search (pw_plan_batch_*, search.PlanBatch) over every Level 1-4 puzzle in ONE launch per (mode, K):
the sweep that tools/bench_planner.py runs one puzzle after the other, here under a per-puzzle time limit on the device's
clock.

Per (mode, K): the wall time of the launch (run to results, on the host) and of the handle's creation (puzzle set, engine,
RGD tables, slabs), solved / exhausted / limit / timeout counts, Level-1 puzzles solved, and per puzzle its status, plan
length, rounds, visited states and device seconds.  Every plan is checked with PushWorldPuzzle.is_valid_plan.

    python tools/bench_plan_batch.py [--limit 0.4] [--batches 1,8,64] [--modes N+RGD,RGD] [--max-states 1048576]
                                     [--out profiles/plan_batch.txt]
"""
import argparse
import glob
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PUZZLES = os.path.join(ROOT, "pushworld_amd", "data", "puzzles")


def level_puzzles():
    return [(lvl, p) for lvl in (1, 2, 3, 4) for p in sorted(glob.glob(os.path.join(PUZZLES, f"level{lvl}", "*.pwp")))]


def sweep(mode, k, limit, max_states, todo):
    import torch
    from pushworld_amd.puzzle import PushWorldPuzzle
    from pushworld_amd.search import PlanBatch

    t0 = time.perf_counter()
    pb = PlanBatch([PushWorldPuzzle(p, order="cpp") for _, p in todo], heuristic=mode, batch=k, max_states=max_states)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    pb.run(time_limit=limit)
    res = pb.results()
    t2 = time.perf_counter()
    pb.close()
    rows = []
    for (lvl, path), (plan, info, dev_s) in zip(todo, res):
        valid = None
        if plan is not None:
            valid = PushWorldPuzzle(path).is_valid_plan(plan)
        rows.append(dict(level=lvl, puzzle=os.path.basename(path)[:-4], status=info.status,
                         plan_len=len(plan) if plan is not None else None, valid=valid, rounds=info.rounds,
                         visited=info.visited, device_s=dev_s))
    return t1 - t0, t2 - t1, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--limit", type=float, default=0.4, help="seconds per puzzle (device clock)")
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--modes", default="N+RGD,RGD")
    ap.add_argument("--max-states", type=int, default=1 << 20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    todo = level_puzzles()
    head, body = [], []
    for mode in args.modes.split(","):
        for k in (int(v) for v in args.batches.split(",")):
            create_s, run_s, rows = sweep(mode, k, args.limit, args.max_states, todo)
            count = {s: sum(1 for r in rows if r["status"] == s) for s in ("solved", "exhausted", "limit", "timeout", "range")}
            l1 = sum(1 for r in rows if r["level"] == 1 and r["status"] == "solved")
            n1 = sum(1 for r in rows if r["level"] == 1)
            bad = sum(1 for r in rows if r["valid"] is False)
            rates = sorted(r["rounds"] / r["device_s"] for r in rows if r["rounds"] > 50 and r["device_s"] > 0)
            med = rates[len(rates) // 2] if rates else 0.0
            line = (f"#   {mode:5s}  K={k:<3d}  launch {run_s:6.3f} s  (create {create_s:5.2f} s)  solved {count['solved']:3d}  "
                    f"exhausted {count['exhausted']:2d}  limit {count['limit']:2d}  timeout {count['timeout']:3d}  "
                    f"range {count['range']}  Level-1 solved {l1} / {n1}  invalid plans {bad}  "
                    f"median {med:8.0f} rounds/s")
            print(line, flush=True)
            head.append(line)
            body.append(f"# ---- {mode} K={k}")
            body.append("# level  status     plan  rounds     visited  device s  puzzle")
            for r in rows:
                plen = str(r["plan_len"]) if r["plan_len"] is not None else "-"
                body.append(f"{r['level']:7d}  {r['status']:9s}  {plen:>4s}  {r['rounds']:6d}  {r['visited']:10d}  "
                            f"{r['device_s']:8.4f}  {r['puzzle']}")
    text = "\n".join([
        f"# Batched best-first search (pw_plan_batch_*) on one MI355X: all {len(todo)} Level 1-4 puzzles in ONE launch per "
        "(mode, K)",
        "#",
        f"#   python tools/bench_plan_batch.py --limit {args.limit} --batches {args.batches} --modes {args.modes} "
        f"--max-states {args.max_states}",
        "#",
        f"# {args.limit} s per puzzle on the device's clock (status timeout past it), max_states {args.max_states} per puzzle,",
        "# reference action order, C++ object order.  launch: pb.run() to pb.results() on the host (one launch, all puzzles);",
        "# create: the PlanBatch (puzzle set, engine, one RGD table set per puzzle, slabs).  device s: one puzzle's search on",
        "# the device clock.  Every plan is replayed by PushWorldPuzzle.is_valid_plan.  median rounds/s: one puzzle's rounds per",
        "# device second, median over the puzzles that ran more than 50 rounds (each puzzle has its own workgroup).",
        "#",
    ] + head + ["#"] + body) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

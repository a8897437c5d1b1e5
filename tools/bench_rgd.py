#!/usr/bin/env python3
"""Throughput of the batched RGD heuristic (pw_rgd_eval) in both modes.

(a) every Level-1 puzzle: the first 2^20 states a breadth-first search reaches (BreadthFirstSearch layers, read straight
    into a device tensor; tiled up to 2^20 where the puzzle has fewer reachable states);
(b) a few heavy Level-2/3 puzzles (most movables), the same way with --heavy-states states.
Full-depth mode on puzzles with more than 6 movables gets --full-states states (its cost grows exponentially with N).
Reports states/s per puzzle and over each group (states / wall time of the launches between two synchronisations),
the states that ran out of budget, and the table build time of pw_rgd_create.

    python tools/bench_rgd.py [--states 1048576] [--reps 3] [--heavy 4] [--json out.json]
"""
import argparse
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from pushworld_amd import _capi  # noqa: E402
from pushworld_amd.puzzle import PushWorldPuzzle  # noqa: E402
from pushworld_amd.search import BreadthFirstSearch, RecursiveGraphDistance  # noqa: E402

PUZZLES = os.path.join(ROOT, "pushworld_amd", "data", "puzzles")


def reachable_states(pz, count):
    """int32 [count, N] device tensor: breadth-first layers from the initial state, tiled when there are fewer."""
    bfs = BreadthFirstSearch(pz, max_states=count)
    bfs.begin()
    try:
        while not bfs.exhausted and bfs.total_states < count:
            bfs.expand()
    except ValueError:  # the store is full: the last layer is cut short
        pass
    n = min(bfs.total_states, count)
    out = torch.empty((n, pz.num_movables), dtype=torch.int32, device=bfs.device)
    _capi.check(_capi.lib.pw_search_read_states(bfs.handle, 0, n, _capi._ptr(out), bfs._stream()))
    torch.cuda.synchronize(bfs.device)
    bfs.close()
    reps = (count + n - 1) // n
    return out.repeat(reps, 1)[:count].contiguous(), n


def run(pz, states, fewest, reps):
    t0 = time.perf_counter()
    h = RecursiveGraphDistance(pz, fewest_tools=fewest)
    build_ms = (time.perf_counter() - t0) * 1e3
    h.evaluate(states[:4096].contiguous())  # warm-up
    torch.cuda.synchronize(h.device)
    e0 = h.exceeded
    t0 = time.perf_counter()
    for _ in range(reps):
        cost = h.evaluate(states)
    torch.cuda.synchronize(h.device)
    sec = (time.perf_counter() - t0) / reps
    finite = torch.isfinite(cost).sum().item()
    nan = torch.isnan(cost).sum().item()
    exceeded = (h.exceeded - e0) // reps
    h.close()
    return {"sec": sec, "states_per_s": states.shape[0] / sec, "build_ms": build_ms, "finite": finite, "nan": nan,
            "exceeded": exceeded}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--states", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--heavy-states", type=int, default=1 << 16)
    ap.add_argument("--full-states", type=int, default=1 << 14,
                    help="states of full-depth mode on puzzles with more than 6 movables (exponential in N)")
    ap.add_argument("--heavy", type=int, default=4)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    level1 = sorted(glob.glob(os.path.join(PUZZLES, "level1", "*.pwp")))
    heavy = sorted(glob.glob(os.path.join(PUZZLES, "level2", "*.pwp")) + glob.glob(os.path.join(PUZZLES, "level3", "*.pwp")),
                   key=lambda p: (-PushWorldPuzzle(p).num_movables, p))[: args.heavy]
    record = {"states": args.states, "reps": args.reps, "groups": {}}
    for group, paths in (("level1", level1), ("heavy", heavy)):
        rows = []
        for path in paths:
            pz = PushWorldPuzzle(path)
            count = args.states if group == "level1" else args.heavy_states
            states, distinct = reachable_states(pz, count)
            for fewest in (True, False):
                n = count if fewest or pz.num_movables <= 6 else min(count, args.full_states)
                r = run(pz, states[:n].contiguous(), fewest, args.reps)
                r.update(count=n, puzzle=os.path.relpath(path, PUZZLES), N=pz.num_movables, distinct=distinct,
                         mode="fewest" if fewest else "full")
                rows.append(r)
                print("%-40s N=%2d %-6s %8d states %9.3e states/s  build %7.1f ms  inf %7d  nan %6d  exceeded %d" % (
                    r["puzzle"][:40], r["N"], r["mode"], n, r["states_per_s"], r["build_ms"],
                    n - r["finite"] - r["nan"], r["nan"], r["exceeded"]), flush=True)
            del states
        summary = {}
        for mode in ("fewest", "full"):
            sel = [r for r in rows if r["mode"] == mode]
            tot = sum(r["sec"] for r in sel)
            summary[mode] = {"states_per_s": sum(r["count"] for r in sel) / tot if tot else 0.0,
                             "exceeded_per_pass": sum(r["exceeded"] for r in sel),
                             "puzzles": len(sel)}
            print("== %s %s: %.3e states/s over %d puzzles, %d states past the budget per pass" % (
                group, mode, summary[mode]["states_per_s"], len(sel), summary[mode]["exceeded_per_pass"]), flush=True)
        record["groups"][group] = {"summary": summary, "rows": rows}
    if args.json:
        with open(args.json, "w") as f:
            json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()

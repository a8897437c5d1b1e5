#!/usr/bin/env python3
"""Best-first planner (pw_planner_*, search.BestFirstSearch) over every Level 1-4 puzzle: both modes, K in {1, 256, 4096,
65536}, a wall-clock limit per puzzle.

Each (mode, K) step runs in a child process of its own under `timeout -k` (--step-timeout seconds), which prints one JSON
line per puzzle as it goes: a step cut short by its timeout keeps the puzzles it finished.  Per puzzle: status (or
"timeout" when the wall-clock limit ran out first: the search was still running), plan length, expanded, visited,
rounds, wall seconds (begin + run, not the handle's creation), rounds/s, states/s (visited states / wall) and the
largest finite key pushed (pw_planner_max_key: RGD mode, the largest RGD cost; N+RGD, novelty * 1e6 + cost).

    python tools/bench_planner.py [--limit 0.4] [--batches 1,256,4096,65536] [--modes RGD,N+RGD] [--out planner.txt]
    python tools/bench_planner.py --worker --mode N+RGD --batch 4096 [--puzzle PATH]     (one step; used by the above)
    python tools/bench_planner.py --trace-summary DIR     (kernel time per round from a rocprofv3 --kernel-trace output)
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PUZZLES = os.path.join(ROOT, "pushworld_amd", "data", "puzzles")


def level_puzzles():
    return [(lvl, p) for lvl in (1, 2, 3, 4) for p in sorted(glob.glob(os.path.join(PUZZLES, f"level{lvl}", "*.pwp")))]


def worker(args):
    import torch
    from pushworld_amd.puzzle import PushWorldPuzzle
    from pushworld_amd.search import BestFirstSearch

    todo = [(0, args.puzzle)] if args.puzzle else level_puzzles()
    for lvl, path in todo:
        pz = PushWorldPuzzle(path, order="cpp")
        bfs = BestFirstSearch(pz, heuristic=args.mode, batch=args.batch, max_states=args.max_states)
        per_call = 1 if args.batch >= 65536 else (4 if args.batch >= 4096 else 64)  # rounds between wall-clock checks
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        bfs.begin()
        while True:
            info = bfs.run(per_call)
            wall = time.perf_counter() - t0
            if info.status != "running" or wall > args.limit:
                break
        plan = bfs.plan()
        rec = dict(level=lvl, puzzle=os.path.basename(path)[:-4], mode=args.mode, K=args.batch,
                   status=info.status if info.status != "running" else "timeout",
                   plan_len=len(plan) if plan is not None else None, expanded=info.expanded, visited=info.visited,
                   rounds=info.rounds, wall_s=round(wall, 5), rounds_per_s=round(info.rounds / wall, 1),
                   states_per_s=round(info.visited / wall, 1), max_key=bfs.max_key(), rgd_exceeded=info.rgd_exceeded)
        bfs.close()
        print(json.dumps(rec), flush=True)


def trace_summary(d):
    """Kernel time per kernel name and per round, against the span from the first round's pop to the last kernel's end,
    from a rocprofv3 --kernel-trace output directory (rocpd database or CSV)."""
    rows = []  # (name, start ns, end ns)
    for f in glob.glob(os.path.join(d, "**", "*.db"), recursive=True):
        import sqlite3
        with sqlite3.connect(f) as c:
            rows += [(n, int(s), int(e)) for n, s, e in c.execute("select name, start, end from kernels")]
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            rows += [(r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in csv.DictReader(fh)]
    first_pop = min((s for n, s, e in rows if n.startswith("pw_planner_pop_kernel")), default=None)
    if first_pop is None:
        return "no planner kernels found under " + d
    rows = [r for r in rows if r[1] >= first_pop]  # the rounds (pw_planner_run), not the handle's setup
    per = {}
    t0, t1, busy = None, None, 0
    for name, s, e in rows:
        name = name.split("(")[0].split(" [")[0]
        if "radix_sort" in name or "rocprim" in name:
            name = "rocprim radix sort kernels"
        c = per.setdefault(name, [0, 0])
        c[0] += 1
        c[1] += e - s
        busy += e - s
        t0 = s if t0 is None else min(t0, s)
        t1 = e if t1 is None else max(t1, e)
    pops = per.get("pw_planner_pop_kernel", [0, 0])[0] or 1
    out = [f"kernels: {len(rows)}, span {((t1 - t0) / 1e6):.3f} ms, kernel time {busy / 1e6:.3f} ms "
           f"({100.0 * busy / max(t1 - t0, 1):.1f} % of the span; the rest is launch gaps and host work)",
           f"rounds (pop launches): {pops}: per round {((t1 - t0) / pops / 1e3):.1f} us of span, {busy / pops / 1e3:.1f} us of kernels",
           f"{'kernel':<48} {'calls':>8} {'total ms':>10} {'us/call':>9}"]
    for name, (n, ns) in sorted(per.items(), key=lambda kv: -kv[1][1]):
        out.append(f"{name[:48]:<48} {n:>8} {ns / 1e6:>10.3f} {ns / n / 1e3:>9.2f}")
    return "\n".join(out)


def driver(args):
    lines = []
    header = (f"{'lvl':>3} {'puzzle':<34} {'mode':<6} {'K':>6} {'status':<10} {'plan':>5} {'expanded':>9} {'visited':>9} "
              f"{'rounds':>7} {'wall s':>8} {'rounds/s':>9} {'states/s':>10} {'max key':>10}")
    recs = []
    for mode in args.modes.split(","):
        for k in (int(x) for x in args.batches.split(",")):
            cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--worker",
                   "--mode", mode, "--batch", str(k), "--limit", str(args.limit), "--max-states", str(args.max_states)]
            t = time.perf_counter()
            p = subprocess.run(cmd, capture_output=True, text=True)
            got = [json.loads(x) for x in p.stdout.splitlines() if x.startswith("{")]
            recs += got
            msg = f"step {mode} K={k}: exit {p.returncode}, {len(got)} puzzles, {time.perf_counter() - t:.1f} s"
            print(msg, flush=True)
            lines.append("# " + msg)
            if p.returncode != 0:
                lines.append("# stderr tail: " + " | ".join(p.stderr.strip().splitlines()[-3:]))
            if p.returncode in (124, 137, -6, 134, -11, 139):
                break  # a step that hung or faulted ends the run: nothing more is started on the GPU
        else:
            continue
        break
    lines.append(header)
    for r in recs:
        lines.append(f"{r['level']:>3} {r['puzzle'][:34]:<34} {r['mode']:<6} {r['K']:>6} {r['status']:<10} "
                     f"{'' if r['plan_len'] is None else r['plan_len']:>5} {r['expanded']:>9} {r['visited']:>9} {r['rounds']:>7} "
                     f"{r['wall_s']:>8.3f} {r['rounds_per_s']:>9.0f} {r['states_per_s']:>10.0f} {r['max_key']:>10.0f}")
    lines.append("")
    lines.append(f"{'mode':<6} {'K':>6} {'puzzles':>7} {'solved':>6} {'exhausted':>9} {'limit':>5} {'timeout':>7} "
                 f"{'wall s':>8} {'max key':>10}")
    for mode in args.modes.split(","):
        for k in (int(x) for x in args.batches.split(",")):
            g = [r for r in recs if r["mode"] == mode and r["K"] == k]
            if not g:
                continue
            cnt = {s: sum(r["status"] == s for r in g) for s in ("solved", "exhausted", "limit", "timeout")}
            lines.append(f"{mode:<6} {k:>6} {len(g):>7} {cnt['solved']:>6} {cnt['exhausted']:>9} {cnt['limit']:>5} "
                         f"{cnt['timeout']:>7} {sum(r['wall_s'] for r in g):>8.1f} {max(r['max_key'] for r in g):>10.0f}")
    text = "\n".join(lines) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
        with open(os.path.splitext(args.out)[0] + ".jsonl", "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in recs)
    print(text)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--mode", default="N+RGD")
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--puzzle")
    ap.add_argument("--modes", default="N+RGD,RGD")
    ap.add_argument("--batches", default="1,256,4096,65536")
    ap.add_argument("--limit", type=float, default=0.4, help="wall-clock seconds per puzzle")
    ap.add_argument("--step-timeout", type=int, default=280, help="seconds per (mode, K) step")
    ap.add_argument("--max-states", type=int, default=1 << 22)
    ap.add_argument("--out")
    ap.add_argument("--trace-summary")
    args = ap.parse_args()
    if args.trace_summary:
        print(trace_summary(args.trace_summary))
    elif args.worker:
        worker(args)
    else:
        driver(args)


if __name__ == "__main__":
    main()

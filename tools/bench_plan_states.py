#!/usr/bin/env python3
"""Planning from the live states of a batch of environments (VecPushWorld.expert_actions, pw_plan_batch_run_states): 4096
environments over the 68 Level-1 puzzles, each after 16 seeded random steps, one launch per (mode, K) under a time limit
per item on the device's clock.

Per (mode, K): the wall time of the launch (expert_actions to the host copy of its result), of the planner's creation
(one RGD table set per puzzle, slabs) and of a second launch on the same handle; the statuses by count; the distribution
of the device seconds per item.  For comparison, BestFirstSearch.begin(start) + run on a sample of 64 of the same states,
one after the other on the host, in chunks of rounds until the same time limit (host clock) has passed.

    python tools/bench_plan_states.py [--envs 4096] [--steps 16] [--limit 0.2] [--batches 1,8] [--modes N+RGD,RGD]
                                      [--max-states 65536] [--sample 64] [--out profiles/plan_states.txt]
"""
import argparse
import glob
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PUZZLES = os.path.join(ROOT, "pushworld_amd", "data", "puzzles")
STATUSES = ("solved", "exhausted", "limit", "timeout", "range", "running", "skipped")


def make_vec(envs, steps, seed):
    import torch
    from pushworld_amd.puzzle import PushWorldPuzzle
    from pushworld_amd.vec_env import VecPushWorld

    paths = sorted(glob.glob(os.path.join(PUZZLES, "level1", "*.pwp")))
    vec = VecPushWorld([PushWorldPuzzle(p, order="cpp") for p in paths], envs, observation=None)
    vec.reset()
    rng = np.random.default_rng(seed)
    for _ in range(steps):
        vec.step(torch.as_tensor(rng.integers(0, 4, size=envs).astype(np.uint8), device=vec.device))
    torch.cuda.synchronize()
    return vec, paths


def host_sample(vec, mode, k, limit, max_states, sample):
    from pushworld_amd.search import BestFirstSearch

    states, ids = vec.states(), vec.puzzle_id.cpu().numpy()
    pick = np.linspace(0, vec.num_envs - 1, sample).astype(np.int64)
    bfs = {}
    count = {s: 0 for s in STATUSES}
    per = []
    for i in pick:
        pid = int(ids[i])
        if pid not in bfs:
            bfs[pid] = BestFirstSearch(vec.puzzles[pid], heuristic=mode, batch=k, max_states=max_states)
        b = bfs[pid]
        start = [(int(x), int(y)) for x, y in states[i, : vec.puzzles[pid].num_movables]]
        t0 = time.perf_counter()
        b.begin(start=start)
        info = b.run(256)
        while info.status == "running" and time.perf_counter() - t0 < limit:
            info = b.run(256)
        per.append(time.perf_counter() - t0)
        count[info.status if info.status != "running" else "timeout"] += 1
    for b in bfs.values():
        b.close()
    return sum(per), count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--limit", type=float, default=0.2, help="seconds per item (device clock)")
    ap.add_argument("--batches", default="1,8")
    ap.add_argument("--modes", default="N+RGD,RGD")
    ap.add_argument("--max-states", type=int, default=1 << 16)
    ap.add_argument("--sample", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    vec, paths = make_vec(args.envs, args.steps, args.seed)
    prop = torch.cuda.get_device_properties(vec.device)
    box = (f"{prop.name} ({getattr(prop, 'gcnArchName', '?')}, {prop.multi_processor_count} CUs), torch {torch.__version__}, "
           f"HIP {torch.version.hip}")
    head, body = [], []
    for mode in args.modes.split(","):
        for k in (int(v) for v in args.batches.split(",")):
            t0 = time.perf_counter()
            sp = vec.planner(heuristic=mode, batch=k, max_states=args.max_states)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            vec.expert_actions(sp, time_limit=args.limit).cpu()
            t2 = time.perf_counter()
            first = vec.expert_actions(sp, time_limit=args.limit).cpu().numpy()
            t3 = time.perf_counter()
            res = sp.results()
            sp.close()
            count = {s: sum(1 for _, i, _ in res if i.status == s) for s in STATUSES}
            dev = np.array([s for _, _, s in res])
            q = np.percentile(dev, [50, 90, 99])
            with_action = int((first >= 0).sum())
            host_s, host_count = host_sample(vec, mode, k, args.limit, args.max_states, args.sample)
            line = (f"#   {mode:5s}  K={k:<2d}  launch {t2 - t1:6.3f} s (again {t3 - t2:6.3f} s, create {t1 - t0:5.2f} s)  "
                    + "  ".join(f"{s} {count[s]}" for s in STATUSES if count[s] or s in ("solved", "timeout"))
                    + f"  first action for {with_action}  device s p50 {q[0]:.4f} p90 {q[1]:.4f} p99 {q[2]:.4f} "
                    f"max {dev.max():.4f} sum {dev.sum():.1f}")
            hline = (f"#          host BestFirstSearch, {args.sample} of the states one after the other: {host_s:6.2f} s  "
                     + "  ".join(f"{s} {c}" for s, c in host_count.items() if c)
                     + f"  (x {args.envs / args.sample:.0f} for all: ~{host_s * args.envs / args.sample:.0f} s)")
            print(line, flush=True)
            print(hline, flush=True)
            head += [line, hline]
            body.append(f"# ---- {mode} K={k}: per puzzle (its {args.envs // len(paths)}-{-(-args.envs // len(paths))} "
                        "environments): solved / items, median device s")
            ids = vec.puzzle_id.cpu().numpy()
            for pid, path in enumerate(paths):
                rows = [res[i] for i in np.flatnonzero(ids == pid)]
                ok = sum(1 for _, i, _ in rows if i.status == "solved")
                med = float(np.median([s for _, _, s in rows]))
                body.append(f"{ok:4d} / {len(rows):3d}  {med:8.4f}  {os.path.basename(path)[:-4]}")
    text = "\n".join([
        f"# Planning from live environment states (VecPushWorld.expert_actions, pw_plan_batch_run_states) on {box}",
        "#",
        f"#   python tools/bench_plan_states.py --envs {args.envs} --steps {args.steps} --seed {args.seed} --limit {args.limit} "
        f"--batches {args.batches} --modes {args.modes} --max-states {args.max_states} --sample {args.sample}",
        "#",
        f"# {args.envs} environments over the {len(paths)} Level-1 puzzles (C++ object order, environment i plays puzzle i mod "
        f"{len(paths)}), each after {args.steps} seeded random",
        f"# steps; one expert_actions launch per (mode, K) from those states, {args.limit} s per item on the device's clock,",
        f"# max_states {args.max_states} per item, reference action order.  launch: expert_actions to the host copy of the",
        "# first actions (the first launch of a handle adds its workgroups, up to two per CU); again: the same on the same",
        "# handle; create: VecPushWorld.planner (one RGD table set per puzzle, slabs).  device s: one item's search on the",
        "# device clock.  host: BestFirstSearch.begin(start) + run in chunks of 256 rounds until solved / ended or the",
        "# time limit passed on the host clock (counted as timeout), on an evenly spaced sample of the same states.",
        "#",
    ] + head + ["#"] + body) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()

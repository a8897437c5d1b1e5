#!/usr/bin/env python3
"""Cell-grid observations on the C3 shape: 65 536 environments over the 68 Level-1 puzzles, default
frame (51 x 42 cells, 6 426 bytes per observation).

Records, from one process:
  * pw_render_cells microseconds per launch (device events around each of --launches launches; median and best),
    the bytes it writes per launch and their fraction of the 8 TB/s HBM peak;
  * env-steps/s of --steps consecutive steps, timed with device events around the whole loop, for
    state-only pw_step, pw_step_cells, and uint8 pixels_per_cell 3 pw_step_render (untuned observation buffer);
and, with --rocprof-dir, the kernel table of a separate `rocprofv3 --kernel-trace --stats --output-format csv` run of
`--only-render` (its kernel_stats.csv).

    python tools/bench_cells.py [--envs 65536] [--steps 300] [--launches 200] [--out profiles/cells.txt]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_cells.py --only-render
    python tools/bench_cells.py --rocprof-dir DIR --out profiles/cells.txt      (appends the kernel table)
"""
import argparse
import csv
import glob
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PUZZLES = os.path.join(ROOT, "pushworld_amd", "data", "puzzles")
PEAK = 8.0e12  # bytes/s, MI355X HBM3E


def make(observation, envs, **kw):
    import torch
    from pushworld_amd.puzzle import PushWorldPuzzle
    from pushworld_amd.vec_env import VecPushWorld

    pool = [PushWorldPuzzle(p) for p in sorted(glob.glob(os.path.join(PUZZLES, "level1", "*.pwp")))]
    vec = VecPushWorld(pool, envs, observation=observation, device=0, autoreset=True, max_steps=100, tune=False, **kw)
    vec.reset()
    torch.cuda.synchronize()
    return vec


def time_launches(fn, n):
    import torch

    evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for a, b in evs:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return np.array([a.elapsed_time(b) * 1e3 for a, b in evs])  # microseconds


def rollout_rate(vec, actions):
    import torch

    for t in range(min(10, actions.shape[0])):  # warm-up
        vec.step(actions[t])
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for t in range(actions.shape[0]):
        vec.step(actions[t])
    b.record()
    torch.cuda.synchronize()
    sec = a.elapsed_time(b) * 1e-3
    return vec.num_envs * actions.shape[0] / sec, sec * 1e6 / actions.shape[0]


def rocprof_table(d):
    paths = sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True))
    if not paths:
        return [f"(no kernel_stats.csv under {d})"]
    lines = [f"rocprofv3 --kernel-trace --stats, {os.path.basename(paths[-1])}: kernel, calls, average us, min us, max us"]
    with open(paths[-1]) as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "?").replace("void ", "")
            calls = int(row.get("Calls", 0))
            avg = float(row.get("AverageNs", 0)) * 1e-3
            lo, hi = float(row.get("MinNs", 0)) * 1e-3, float(row.get("MaxNs", 0)) * 1e-3
            lines.append(f"  {name[:60]:60s} {calls:6d} {avg:9.2f} {lo:9.2f} {hi:9.2f}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cells.txt"))
    ap.add_argument("--only-render", action="store_true", help="only the pw_render_cells launches (for rocprofv3)")
    ap.add_argument("--rocprof-dir", help="append the kernel table of a rocprofv3 csv output directory to --out")
    args = ap.parse_args()
    if args.rocprof_dir:
        with open(args.out, "a") as f:
            f.write("\n".join(rocprof_table(args.rocprof_dir)) + "\n")
        return
    import torch

    B = args.envs
    cells = make("cells", B)
    S = cells.obs[0].numel()
    npad = cells.engine.np
    render = lambda: cells.engine.render_cells(cells.puzzle_id, cells.pos, cells.obs)  # noqa: E731
    us = time_launches(render, args.launches)
    if args.only_render:
        print(f"pw_render_cells: median {np.median(us):.2f} us over {args.launches} launches")
        return
    strides = {}  # the same launch into padded layouts: environments on 16-byte / 128-byte (cache line) boundaries
    for stride in ((S + 15) & ~15, (S + 127) & ~127):
        buf = torch.empty((B * stride,), dtype=torch.uint8, device=cells.device)
        strides[stride] = float(np.median(time_launches(
            lambda: cells.engine.render_cells(cells.puzzle_id, cells.pos, buf, env_stride=stride), args.launches)))
        del buf
    g = torch.Generator(device="cpu").manual_seed(0)
    actions = torch.randint(0, 4, (args.steps, B), generator=g, dtype=torch.uint8).to(cells.device)
    rate_cells, us_cells = rollout_rate(cells, actions)
    del cells
    torch.cuda.empty_cache()
    state = make(None, B)
    rate_state, us_state = rollout_rate(state, actions)
    del state
    torch.cuda.empty_cache()
    rgb = make("uint8", B, pixels_per_cell=3, border_width=1)
    rgb_bytes = rgb.engine.obs_bytes
    rate_rgb, us_rgb = rollout_rate(rgb, actions)
    del rgb
    torch.cuda.empty_cache()

    med, best = float(np.median(us)), float(us.min())
    wbytes = B * S
    lines = [
        f"cell-grid observations, {B} environments over the 68 Level-1 puzzles, frame 51 x 42 cells "
        f"({S} bytes per observation, tight stride), {torch.cuda.get_device_name(0)}",
        "",
        f"pw_render_cells ({args.launches} launches, device events): median {med:.2f} us, best {best:.2f} us per launch",
        f"  bytes written per launch {wbytes} ({S} per environment, each once); algorithmic reads per environment: "
        f"4 B puzzle id + {2 * npad} B positions from HBM, the {(S + 15) & ~15} B base image from the caches (68 puzzles, 437 KB)",
        f"  write bandwidth {wbytes / (med * 1e-6) / 1e9:.0f} GB/s at the median = {wbytes / (med * 1e-6) / PEAK:.3f} of the "
        f"8 TB/s peak (best launch {wbytes / (best * 1e-6) / PEAK:.3f})",
    ] + [
        f"  padded stride {st} B: median {t:.2f} us = {wbytes / (t * 1e-6) / PEAK:.3f} of the peak (same bytes written)"
        for st, t in strides.items()
    ] + [
        "",
        f"{args.steps}-step loops, autoreset, max_steps 100, uniform random actions (device events around the loop):",
        f"  pw_step (state only)           {us_state:9.2f} us/step  {rate_state:.3e} env-steps/s",
        f"  pw_step_cells                  {us_cells:9.2f} us/step  {rate_cells:.3e} env-steps/s  "
        f"({S} B of observation per env-step)",
        f"  pw_step_render uint8 ppc 3     {us_rgb:9.2f} us/step  {rate_rgb:.3e} env-steps/s  "
        f"({rgb_bytes} B per env-step; observation buffer untuned)",
        f"  step + cells - state-only step = {us_cells - us_state:.2f} us per step (the cells launch: median above "
        f"{med:.2f} us)",
        "",
    ]
    text = "\n".join(lines)
    print(text)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()

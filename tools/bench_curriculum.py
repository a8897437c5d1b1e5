"""Measures the statistics per puzzle and the weighted draw (pw_episode_stats / pw_curriculum_update / pw_resample_weighted,
DESIGN.md K25) and prints the figures kept in profiles/curriculum.txt.

    python tools/bench_curriculum.py [--envs 65536] [--mid-pools 256,1024] [--pool 4096] [--big-pool 15600] [--steps 50]
                                     [--repeats 3] > profiles/curriculum.txt

Two puzzle sets: the C3 set (the 68 Level-1 puzzles) and a pool of --pool generated Level-0 puzzles.  Per set, in one process and
interleaved round by round (pools of --mid-pools puzzles and one of --big-pool puzzles, the size of the whole benchmark, state only):
  (1) the step loop of VecPushWorld(autoreset=True, resample=True), state only and with the uint8 render:
        uniform     pw_resample + the step launch                                  (what exists without this feature)
        curriculum  pw_resample_weighted + the step launch + pw_episode_stats       (curriculum="frontier", weights updated before)
      milliseconds per step over --steps steps of seeded random actions, max_steps 100.
  (2) pw_curriculum_update alone (mode frontier on the statistics the loop left).
  (3) pw_resample_weighted alone with and without the fence in LDS (PW_OPT_RESAMPLE_FENCE), for a step (seeded flags: about one
      environment in twenty ends) and for a reset (every environment draws), against pw_resample on the same flags; and
      pw_episode_stats alone on the step's flags and with every environment ending, in its LDS form and its global form
      (PW_OPT_STATS_LDS_PUZZLES) with one workgroup per 256 environments, 64 and 16 workgroups (PW_OPT_STATS_GROUPS).

Timing: the host clock around synchronised calls, best of --repeats after one warm-up round, every repeat listed.  A single launch
takes a few microseconds, less than the host needs to make it: 50 launches are captured in a graph and the replay is timed, so the
figure per launch is the kernel and the gap to the next launch, not the host's call.
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
from pushworld_amd.vec_env import VecPushWorld  # noqa: E402

LEVEL1 = os.path.join(ROOT, "pushworld_amd", "data", "puzzles", "level1")
BURST = 50


def ms(ts, scale=1e3, unit="ms"):
    return f"best {min(ts) * scale:.3f} {unit} (" + ", ".join(f"{t * scale:.3f}" for t in ts) + ")"


def clock(fn, n=1):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def interleaved(fns, repeats, n=1):
    """[[seconds per call of fn, per repeat] per fn]: every fn once per round, round 0 is the warm-up."""
    out = [[] for _ in fns]
    for k in range(repeats + 1):
        for ts, fn in zip(out, fns):
            t = clock(fn, n)
            if k:
                ts.append(t)
    return out


def measure(name, puzzles, args, render=True):
    B, T = args.envs, args.steps
    for obs in (None, "uint8") if render else (None,):
        kw = dict(max_steps=100, observation=obs, pixels_per_cell=3, border_width=1, autoreset=True, resample=True,
                  seed=args.seed, tune=False)
        plain = VecPushWorld(puzzles, B, **kw)
        cur = VecPushWorld(puzzles, B, curriculum="frontier", **kw)
        P = plain.num_puzzles
        gen = torch.Generator(device=plain.device).manual_seed(args.seed)
        acts = torch.randint(0, 4, (T, B), dtype=torch.uint8, device=plain.device, generator=gen)
        age = torch.randint(0, 100, (B,), dtype=torch.int32, device=plain.device, generator=gen)
        for vec in (plain, cur):
            vec.reset()
            vec.steps.copy_(age)  # episodes of every age: about one in a hundred ends per step, not all of them every 101st
            for t in range(T):    # (some statistics, then weights that are not uniform)
                vec.step(acts[t])
        cur.curriculum.update()

        def loop(vec):
            def run():
                for t in range(T):
                    vec.step(acts[t])
            return run

        t_plain, t_cur = interleaved([loop(plain), loop(cur)], args.repeats)
        a, b = min(t_plain) / T, min(t_cur) / T
        what = "state only" if obs is None else f"uint8 render, frames of {plain.obs.shape[1]} x {plain.obs.shape[2]}"
        print(f"{name}: {P} puzzles, {B} environments, {T} steps per loop, {what}")
        print(f"  uniform (pw_resample + step):                             {ms(t_plain)} per loop = {a * 1e6:.2f} us per step")
        print(f"  curriculum (pw_resample_weighted + step + pw_episode_stats): {ms(t_cur)} per loop = {b * 1e6:.2f} us per step; "
              f"+{(b - a) * 1e6:.2f} us per step, x{b / a:.3f}")
        if obs is not None:
            del plain, cur
            continue
        # ---- single launches, on seeded flags: about one environment in twenty ends (a loop with shorter episodes than the
        # one above, where one in a hundred does)
        eng, cu = cur.engine, cur.curriculum
        st = cur.puzzle_stats()
        print(f"  statistics the loops left: {int(st.episodes.sum())} episodes, {int(st.solved.sum())} solved")
        kind = torch.randint(0, 64, (B,), device=cur.device, generator=gen)
        term, trunc = (kind == 0).to(torch.uint8), ((kind == 1) | (kind == 2)).to(torch.uint8)
        ones = torch.ones_like(term)
        done = int(((term | trunc) != 0).sum())
        pid, ep, scratch = cur.puzzle_id.clone(), cur.episode.clone(), cur.stats.tensor.clone()
        calls = {"update": cu.update,
                 "uniform step": lambda: eng.resample(pid, ep, args.seed, term, trunc),
                 "uniform reset": lambda: eng.resample(pid, ep, args.seed, ones, ones)}
        forms = [(lds, groups) for lds in ((1024, 2048) if P <= 1024 else (2048,)) for groups in (0, 64, 16)]
        for lds, groups in forms:  # (the options are read when the launch is made: one graph each)
            eng.set_option("stats_lds_puzzles", lds)
            eng.set_option("stats_groups", groups)
            calls[f"stats step {lds} {groups}"] = graph_of(eng.bind_episode_stats(pid, cur.steps, term, trunc, scratch), cur.device)
            calls[f"stats every {lds} {groups}"] = graph_of(eng.bind_episode_stats(pid, cur.steps, ones, ones, scratch), cur.device)
        eng.set_option("stats_lds_puzzles", 0)
        eng.set_option("stats_groups", 0)
        for fence in (0, 1):
            eng.set_option("resample_fence", fence)
            step_call = eng.bind_resample_weighted(pid, ep, cu.cdf, term, trunc)
            reset_call = eng.bind_resample_weighted(pid, ep, cu.cdf, ones, ones)
            calls[f"weighted step {fence}"] = graph_of(lambda c=step_call: c(args.seed), cur.device)
            calls[f"weighted reset {fence}"] = graph_of(lambda c=reset_call: c(args.seed), cur.device)
        eng.set_option("resample_fence", 0)
        for key in ("update", "uniform step", "uniform reset"):
            calls[key] = graph_of(calls[key], cur.device)
        names = list(calls)
        res = dict(zip(names, interleaved([calls[k].replay for k in names], args.repeats)))
        us = {k: [t / BURST for t in v] for k, v in res.items()}
        print(f"  single launches, {BURST} of each captured in a graph and replayed (microseconds per launch, launch gaps included); "
              f"flags of a step: {done} of {B} environments end ({100.0 * done / B:.1f} %)")
        print(f"    pw_curriculum_update (frontier, {P} puzzles):   {ms(us['update'], 1e6, 'us')}")
        print("    pw_episode_stats:")
        for lds, groups in forms:
            form = "LDS form" if lds == 1024 else "global form"
            grid = "one workgroup per 256 environments" if not groups else f"{groups} workgroups"
            print(f"      {form}, {grid}: "
                  f"step {ms(us[f'stats step {lds} {groups}'], 1e6, 'us')}; every environment ends "
                  f"{ms(us[f'stats every {lds} {groups}'], 1e6, 'us')}")
        for what, label in (("step", "a step (those flags)"), ("reset", "a reset (every flag set)")):
            print(f"    draw for {label}: pw_resample {ms(us['uniform ' + what], 1e6, 'us')}; pw_resample_weighted with the "
                  f"fence {ms(us['weighted ' + what + ' 1'], 1e6, 'us')}, without {ms(us['weighted ' + what + ' 0'], 1e6, 'us')}")
        del plain, cur, calls


def graph_of(fn, device):
    """A graph of BURST launches of ``fn`` (warmed up on a side stream first)."""
    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream(device).wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(BURST):
            fn()
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--pool", type=int, default=4096)
    ap.add_argument("--mid-pools", default="256,1024", help="further pools, measured state only")
    ap.add_argument("--big-pool", type=int, default=15600, help="a second pool, measured state only (0: none)")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--seed", type=int, default=23)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    print(f"# tools/bench_curriculum.py --envs {args.envs} --mid-pools {args.mid_pools} --pool {args.pool} "
          f"--big-pool {args.big_pool} --steps {args.steps} --seed {args.seed} "
          f"--repeats {args.repeats}")
    print(f"# {torch.cuda.get_device_name(0)}; host clock around synchronised calls, best of {args.repeats} after a warm-up; "
          f"single launches: {BURST} per graph replay")
    puzzles = [PushWorldPuzzle(p) for p in sorted(glob.glob(os.path.join(LEVEL1, "*.pwp")))]
    measure("C3 set", puzzles, args)
    for n in [int(x) for x in args.mid_pools.split(",") if x] + [args.pool, args.big_pool]:
        if n > 0:
            pset, _, _ = generate.generate_level0_set(n, random_seed=args.seed)
            measure("Level-0 pool", pset, args, render=n == args.pool)


if __name__ == "__main__":
    main()

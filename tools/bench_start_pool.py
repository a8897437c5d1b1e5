"""Measures the start-state pools (pw_start_pool_arm / pw_start_pool_draw / pw_start_pool_update_bands, start_pool.StartPool,
VecPushWorld(start_pool=...)) and prints the figures kept in profiles/start_pool.txt.

    python tools/bench_start_pool.py [--envs 65536] [--steps 50] [--repeats 3] [--parent DIR] > profiles/start_pool.txt

  (1) with --parent DIR (a checkout of the parent commit with its library built): the C3 step loop WITHOUT a pool -- state only
      and with the default uint8 render -- of the parent and of this tree, one process each, alternating, --repeats times; the
      spread of the parent's own figures is printed next to the difference.  Without --parent: "unmeasured".
  (2) the C3 set (the 68 Level-1 puzzles), max_steps 100, a pool of the states along the stored human plans (level = the steps
      the plan still takes): the state-only autoreset step without and with the pool (arm + draw), and the rendered step on the
      retained uint8 buffer -- the fused path without a pool against step + draw + render of the changed pages with one.  The
      single launches (arm, draw for a step's flags, draw for every environment, update_bands) from graphs of 50.
  (3) K26's benchmark set -- 200 of generate_level0_set(2000, random_seed=21) within 4 096 states: one pool draw for every
      environment against reset_from_push_tables over one indexed batch and over the loop of 200 push_table()s; the pool's
      build time (from the batch, host side included) and bytes.

Timing: the host clock around synchronised calls, best of --repeats after one warm-up round, every repeat listed.
"""
import argparse
import glob
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--child" in sys.argv:  # (1): the tree under test is the one named, not this file's
    sys.path.insert(0, os.path.abspath(sys.argv[sys.argv.index("--child") + 1]))
else:
    sys.path.insert(0, ROOT)

from pushworld_amd.puzzle import PushWorldPuzzle  # noqa: E402
from pushworld_amd.vec_env import VecPushWorld  # noqa: E402

DATA = os.path.join(ROOT, "pushworld_amd", "data")
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


def c3_puzzles():
    paths = sorted(glob.glob(os.path.join(DATA, "puzzles", "level1", "*.pwp")))
    return paths, [PushWorldPuzzle(p) for p in paths]


def c3_vec(puzzles, B, observation, **kw):
    ids = (np.arange(B, dtype=np.int64) * len(puzzles)) // B  # grouped by puzzle, as bench.py's C3
    return VecPushWorld(puzzles, B, puzzle_ids=ids, max_steps=100, border_width=1, pixels_per_cell=3, observation=observation,
                        autoreset=True, **kw)


def aged(vec, acts, seed):
    """Episodes of every age: about one in a hundred ends per step, not all of them every 101st."""
    gen = torch.Generator(device=vec.device).manual_seed(seed)
    vec.reset()
    vec.steps.copy_(torch.randint(0, 100, (vec.num_envs,), dtype=torch.int32, device=vec.device, generator=gen))
    for t in range(acts.shape[0]):
        vec.step(acts[t])


def loop_of(vec, acts):
    def run():
        for t in range(acts.shape[0]):
            vec.step(acts[t])
    return run


# ---------------------------------------------------------------------------------------------------------------- (1)
def child(args):
    """One process of (1): the C3 loops without a pool on the tree named by --child; one JSON line."""
    _, puzzles = c3_puzzles()
    out = {}
    for obs in (None, "uint8"):
        vec = c3_vec(puzzles, args.envs, obs)
        gen = torch.Generator(device=vec.device).manual_seed(args.seed)
        acts = torch.randint(0, 4, (args.steps, args.envs), dtype=torch.uint8, device=vec.device, generator=gen)
        aged(vec, acts, args.seed)
        ts = interleaved([loop_of(vec, acts)], args.repeats)[0]
        out["state" if obs is None else "render"] = min(ts) / args.steps * 1e6
        del vec
    print(json.dumps(out))


def against_parent(args):
    print("(1) the C3 step loop without a pool, parent commit against this tree (microseconds per step, one process per figure, "
          "alternating)")
    if not args.parent:
        print("  unmeasured (no --parent checkout given)")
        return
    res = {"parent": [], "this": []}
    for k in range(args.repeats):
        for name, root in (("parent", args.parent), ("this", ROOT)):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", root, "--envs", str(args.envs), "--steps", str(args.steps),
                   "--seed", str(args.seed), "--repeats", "3"]
            proc = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if proc.returncode != 0:
                print(f"  {name} run {k} failed:\n{proc.stderr[-2000:]}")
                return
            res[name].append(json.loads(proc.stdout.strip().splitlines()[-1]))
    for key, label in (("state", "state only"), ("render", "uint8 render (the default path)")):
        p, t = [r[key] for r in res["parent"]], [r[key] for r in res["this"]]
        print(f"  {label}: parent " + ", ".join(f"{x:.2f}" for x in p) + f" (spread {max(p) - min(p):.2f}); this tree "
              + ", ".join(f"{x:.2f}" for x in t) + f" (spread {max(t) - min(t):.2f}); best against best "
              f"{min(t) - min(p):+.2f} us, medians {np.median(t) - np.median(p):+.2f} us")


# ---------------------------------------------------------------------------------------------------------------- (2)
def plan_pool(vec, paths, puzzles):
    """The states along the stored human plans of the Level-1 puzzles; level = the steps the plan still takes."""
    from pushworld_amd.start_pool import StartPool

    pz, lv, st = [], [], []
    for p, (path, puzzle) in enumerate(zip(paths, puzzles)):
        sol = os.path.join(DATA, "solutions", "level1", os.path.splitext(os.path.basename(path))[0] + ".yaml")
        if not os.path.exists(sol):
            continue
        with open(sol) as f:
            plan = ["LRUD".index(c) for line in f if line.startswith("plan:") for c in line.split(":", 1)[1].strip()]
        state = puzzle.initial_state
        for t, a in enumerate(plan):
            pos = np.zeros((vec.num_objects_padded, 2), np.int8)
            pos[:puzzle.num_movables] = np.asarray(state, np.int8)
            pz.append(p), lv.append(len(plan) - t), st.append(pos)
            state = puzzle.get_next_state(state, a)
    return StartPool(vec, np.asarray(pz, np.int32), np.asarray(lv, np.int32), np.stack(st))


def c3_loops(args):
    B, T = args.envs, args.steps
    paths, puzzles = c3_puzzles()
    print(f"(2) C3 set: {len(puzzles)} puzzles, {B} environments, max_steps 100, {T} steps per loop")
    probe = c3_vec(puzzles, 1, None)
    t0 = time.perf_counter()
    pool = plan_pool(probe, paths, puzzles)
    torch.cuda.synchronize()
    print(f"  pool: {pool.num_entries} states along the stored plans, levels up to {int(pool.max_level.max())}, {pool.nbytes} bytes "
          f"on the device, built in {(time.perf_counter() - t0) * 1e3:.1f} ms (replaying the plans on the host included)")
    pool.set_band(1, 10)
    for obs in (None, "uint8"):
        plain, pooled = c3_vec(puzzles, B, obs), c3_vec(puzzles, B, obs, start_pool=pool)
        gen = torch.Generator(device=plain.device).manual_seed(args.seed)
        acts = torch.randint(0, 4, (T, B), dtype=torch.uint8, device=plain.device, generator=gen)
        for vec in (plain, pooled):
            aged(vec, acts, args.seed)
        t_plain, t_pool = interleaved([loop_of(plain, acts), loop_of(pooled, acts)], args.repeats)
        a, b = min(t_plain) / T, min(t_pool) / T
        if obs is None:
            print(f"  state only: without a pool {ms(t_plain)} per loop = {a * 1e6:.2f} us per step")
            print(f"              with the pool (arm + step + draw) {ms(t_pool)} per loop = {b * 1e6:.2f} us per step; "
                  f"+{(b - a) * 1e6:.2f} us per step, x{b / a:.3f}")
        else:
            opts = [vec.engine.get_option(k) for vec in (plain, pooled) for k in ("obs_padding_once", "obs_changed_pages")]
            print(f"  uint8 render, frames of {plain.obs.shape[1]} x {plain.obs.shape[2]}, library-owned buffers "
                  f"{plain.obs_owned_by_library} / {pooled.obs_owned_by_library}, obs_padding_once / obs_changed_pages {opts}")
            print(f"              without a pool (the fused pw_step_render) {ms(t_plain)} per loop = {a * 1e6:.2f} us per step")
            print(f"              with the pool (arm + step + draw + render) {ms(t_pool)} per loop = {b * 1e6:.2f} us per step; "
                  f"+{(b - a) * 1e6:.2f} us per step, x{b / a:.3f}")
            del plain, pooled
            continue
        # single launches on seeded flags: about one environment in twenty ends
        eng, dev = pooled.engine, pooled.device
        kind = torch.randint(0, 20, (B,), device=dev, generator=gen)
        term, trunc = (kind == 0).to(torch.uint8), torch.zeros((B,), dtype=torch.uint8, device=dev)
        ones = torch.ones_like(term)
        pending = torch.zeros_like(term)
        pos, steps = pooled.pos.clone(), pooled.steps.clone()
        f1, f2 = term.clone(), trunc.clone()
        ctr = torch.zeros((B,), dtype=torch.int32, device=dev).view(torch.uint32)
        out = (torch.full((B,), -1, dtype=torch.int32, device=dev), torch.full((B,), -1, dtype=torch.int32, device=dev))
        stats = torch.zeros((len(puzzles), 4), dtype=torch.int64, device=dev)
        stats[:, 0], stats[:, 1] = 1000, 900
        arm = eng.bind_start_pool_arm(term, trunc, pending)
        draw_step = eng.bind_start_pool_draw(pool, pooled.puzzle_id, pos, steps, f1, f2, ctr, out[0], out[1], mask=term, band=pool.band)
        draw_all = eng.bind_start_pool_draw(pool, pooled.puzzle_id, pos, steps, f1, f2, ctr, out[0], out[1], mask=ones, band=pool.band)
        calls = {"arm": graph_of(arm, dev), "draw step": graph_of(lambda: draw_step(7), dev),
                 "draw all": graph_of(lambda: draw_all(7), dev),
                 "bands": graph_of(lambda: pool.update_bands(stats, min_episodes=1), dev)}
        names = list(calls)
        res = dict(zip(names, interleaved([calls[k].replay for k in names], args.repeats)))
        us = {k: [t / BURST for t in v] for k, v in res.items()}
        print(f"  single launches, {BURST} of each captured in a graph and replayed (microseconds per launch, launch gaps included); "
              f"flags of a step: {int(term.sum())} of {B} environments end")
        print(f"    pw_start_pool_arm {ms(us['arm'], 1e6, 'us')}; pw_start_pool_draw for those flags {ms(us['draw step'], 1e6, 'us')}, "
              f"for every environment {ms(us['draw all'], 1e6, 'us')}; pw_start_pool_update_bands ({len(puzzles)} puzzles) "
              f"{ms(us['bands'], 1e6, 'us')}")
        del plain, pooled, calls


# ---------------------------------------------------------------------------------------------------------------- (3)
def k26_set(args):
    from pushworld_amd import generate
    from pushworld_amd.search import TABLE_BUILT, TABLE_SUMMARY_ONLY, PushSolutionTableBatch
    from pushworld_amd.start_pool import StartPool

    B, cap, rep = args.envs, 4096, args.repeats
    pset, _, _ = generate.generate_level0_set(2000, random_seed=21)
    probe = VecPushWorld(pset, 1, observation=None, max_steps=None)
    with PushSolutionTableBatch(probe, max_states_each=cap, states=0, rows=0) as dry:
        built = np.flatnonzero(dry.status.cpu().numpy() == TABLE_SUMMARY_ONLY)
    qp = [int(i) for i in built[:: max(1, len(built) // 200)][:200]]
    ids = np.asarray(qp, dtype=np.int64)[np.arange(B) % len(qp)]
    vec = VecPushWorld(pset, B, puzzle_ids=ids, observation=None, max_steps=None, seed=1)
    vec.reset()
    batch = vec.push_tables(qp, max_states_each=cap, index=True)
    assert bool((batch.status == TABLE_BUILT).all())
    tables = [vec.push_table(i, max_states=cap) for i in qp]
    print(f"(3) K26's set: {len(pset)} generated puzzles, {len(qp)} of them in the batch ({int(batch.num_states.sum())} canonical "
          f"states); {B} environments")
    t_build = []
    for _ in range(rep):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pool = StartPool.from_tables(vec, [batch])
        torch.cuda.synchronize()
        t_build.append(time.perf_counter() - t0)
    print(f"  pool from the batch: {pool.num_entries} entries (dead ends dropped), levels up to {int(pool.max_level.max())}, "
          f"{pool.nbytes} bytes on the device; built in {ms(t_build)} (the tables are read through the host)")
    ctr = torch.zeros((B,), dtype=torch.int32, device=vec.device)
    out = (torch.full((B,), -1, dtype=torch.int32, device=vec.device), torch.full((B,), -1, dtype=torch.int32, device=vec.device))

    def pool_draw():
        pool.draw(vec.puzzle_id, vec.pos, vec.steps, vec.terminated, vec.truncated, band=(1, None), seed=5, counter=ctr, out=out)

    def pool_reset():  # what reset_from_push_tables does around its draw: pw_reset first
        vec._reset_states(None)
        pool_draw()

    t_draw, t_reset, t_batch, t_loop = interleaved(
        [pool_draw, pool_reset, lambda: vec.reset_from_push_tables([batch], cost=(1, None)),
         lambda: vec.reset_from_push_tables(tables, cost=(1, None))], rep)
    print(f"  one start state for every environment, cost / level (1, None):")
    print(f"      StartPool.draw alone                          {ms(t_draw)}")
    print(f"      pw_reset + StartPool.draw                     {ms(t_reset)}")
    print(f"      reset_from_push_tables, one indexed batch     {ms(t_batch)}: x{min(t_batch) / min(t_reset):.1f}")
    print(f"      reset_from_push_tables, {len(tables)} push_table()s      {ms(t_loop)}: x{min(t_loop) / min(t_reset):.1f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--seed", type=int, default=23)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent", default=None, help="a checkout of the parent commit with its library built, for (1)")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--only", default="1,2,3", help="the parts to run")
    args = ap.parse_args()
    if args.child:
        return child(args)
    print(f"# tools/bench_start_pool.py --envs {args.envs} --steps {args.steps} --seed {args.seed} --repeats {args.repeats}"
          + (" --parent <checkout of the parent commit>" if args.parent else ""))
    print(f"# {torch.cuda.get_device_name(0)}; host clock around synchronised calls, best of {args.repeats} after a warm-up; "
          f"single launches: {BURST} per graph replay")
    parts = args.only.split(",")
    if "1" in parts:
        against_parent(args)
    if "2" in parts:
        c3_loops(args)
    if "3" in parts:
        k26_set(args)


if __name__ == "__main__":
    main()

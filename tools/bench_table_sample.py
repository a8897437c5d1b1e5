#!/usr/bin/env python
"""Drawing from the cost-to-go tables on the device (csrc/pw_table_sample.inc) against the host loops that were
the only way before it, on the device-generated Level-0 set of tools/bench_solution_batch.py and on one per-puzzle table:

  (a) the cost index of every stored table (three launches);
  (b) one sample launch for --envs environments, against states(item) + a numpy draw per puzzle + set_states;
  (c) one plans launch in both tie modes, against the host optimal_plan loop over --sample items;
  (d) VecPushWorld.optimal_demonstrations over the whole batch;
  (e) the same four for one search.SolutionTable (level_0_all_train_3, 10 659 states).

Wall-clock seconds around a synchronised call, best of --repeats after one warm-up; every repeat is printed.

    python tools/bench_table_sample.py [--puzzles 2000] [--envs 65536] > profiles/table_sample.txt
"""
import argparse
import os
import sys
import time
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, repeats):
    import torch

    fn()  # warm-up
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


def fmt(ts):
    return f"best {min(ts) * 1e3:9.3f} ms   all " + " ".join(f"{t * 1e3:.3f}" for t in ts)


def host_sample(vec, tabs, items_of_env, rng, lo, hi):
    """The way before the sample launch: the states of every table to the host, a numpy draw per puzzle, set_states."""
    pos = vec.states().copy()
    for item, envs in items_of_env.items():
        cost = tabs.costs(item).cpu().numpy()
        rows = np.flatnonzero((cost >= lo) & (cost <= min(hi, int(cost[cost != 0xFFFF].max()))))
        if rows.size == 0:
            continue
        states = tabs.states(item)
        pick = rows[rng.integers(0, rows.size, size=len(envs))]
        pos[envs] = 0
        pos[envs, :states.shape[1]] = states[pick]
    vec.set_states(pos)


def bench_tables(label, vec, tables, plan_items, plan_fn, host_sample_fn, args):
    """(b) .. (d) for the environments of `vec` over `tables`."""
    import torch

    B = vec.num_envs
    vec.reset()
    t_s = timed(lambda: vec.reset_from_tables(tables), args.repeats)
    raw = tables[0]
    ctr = torch.zeros((B,), dtype=torch.int32, device=vec.device)
    out = (torch.empty((B,), dtype=torch.int32, device=vec.device), torch.empty((B,), dtype=torch.int32, device=vec.device))
    t_l = timed(lambda: raw.sample(vec.puzzle_id, vec.pos, vec.steps, vec.terminated, vec.truncated, counter=ctr, out=out),
                args.repeats)
    t_h = timed(host_sample_fn, args.repeats)
    print(f"({label}b) sample, {B} environments: one launch              {fmt(t_l)}")
    print(f"     reset_from_tables (reset + sample, state only)       {fmt(t_s)}")
    print(f"     host: states() + numpy draw + set_states             {fmt(t_h)}   x{min(t_h) / min(t_s):.1f} of reset_from_tables")
    vec.reset_from_tables(tables, seed=1)
    index, cost, _ = vec.cost_to_go(tables)
    for tie in ("lowest", "uniform"):
        pl = raw.plans(index, vec.puzzle_id, tie=tie, plan_cap=args.plan_cap)
        t_p = timed(lambda: raw.plans(index, vec.puzzle_id, tie=tie, plan_cap=args.plan_cap, out=pl), args.repeats)
        total = int(pl[1].clamp(min=0).sum().item())
        print(f"({label}c) plans, tie {tie:8s}: one launch, {total} actions  {fmt(t_p)}   {total / min(t_p):14.0f} actions/s")
    t_o = timed(plan_fn, args.repeats)
    n_act = plan_fn()
    print(f"     host: optimal_plan loop over {plan_items} starts ({n_act} actions) {fmt(t_o)}   {n_act / min(t_o):14.0f} actions/s")
    t_d = timed(lambda: vec.optimal_demonstrations(tables, observation=None, plan_cap=args.plan_cap), args.repeats)
    rows = vec.optimal_demonstrations(tables, observation=None, plan_cap=args.plan_cap).num_rows
    print(f"({label}d) optimal_demonstrations, state only: {rows} rows        {fmt(t_d)}   {rows / min(t_d):14.0f} rows/s")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--puzzles", type=int, default=2000)
    ap.add_argument("--sample", type=int, default=200)
    ap.add_argument("--seed", type=int, default=21)
    ap.add_argument("--max-states", type=int, default=1 << 16)
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--plan-cap", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()

    import torch

    from pushworld_amd import _capi, generate
    from pushworld_amd.puzzle import PushWorldPuzzle
    from pushworld_amd.search import SolutionTableBatch
    from pushworld_amd.vec_env import VecPushWorld

    print(f"# tools/bench_table_sample.py --puzzles {args.puzzles} --sample {args.sample} --seed {args.seed} "
          f"--max-states {args.max_states} --envs {args.envs} --plan-cap {args.plan_cap} --repeats {args.repeats}")
    print(f"# {torch.cuda.get_device_name(0)}")
    pset, _, _ = generate.generate_level0_set(args.puzzles, random_seed=args.seed)
    probe = SolutionTableBatch(_capi.Engine(pset, None, 3, 1, _capi.OBS_U8), max_states_each=args.max_states, rows=0)
    status = probe.status.cpu().numpy()
    probe.close()
    stored = np.flatnonzero((status == 0) | (status == 4))
    ids = stored[np.arange(args.envs) % len(stored)].astype(np.int32)  # the environments play the puzzles that have tables
    vec = VecPushWorld(pset, args.envs, puzzle_ids=ids, observation=None, max_steps=None)
    tabs = vec.solution_tables(max_states_each=args.max_states)
    max_cost = tabs.max_cost.cpu().numpy()
    print(f"set: {len(pset)} puzzles, {len(stored)} stored tables, {tabs.rows_needed} rows, largest cost {int(max_cost[stored].max())}")

    # ---- (a) the index: built again for every repeat on a fresh run of the same pool
    def index_build():
        tabs._indexed = False
        _capi.check(_capi.lib.pw_solve_batch_run(tabs.handle, _capi._ptr(tabs._ids), len(tabs.puzzles), tabs.max_states_each,
                                                 tabs._stream()))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tabs._index()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    index_build()
    t_i = [index_build() for _ in range(args.repeats)]
    tabs._counts = tabs._max_costs = tabs._covered = None
    _capi.check(_capi.lib.pw_solve_batch_copy_results(tabs.handle, _capi._ptr(tabs.status), _capi._ptr(tabs.summary),
                                                      _capi._ptr(tabs.row_offset), tabs._stream()))
    print(f"(a) cost index of {len(stored)} tables ({tabs.rows_needed} rows, the run itself not timed): {fmt(t_i)}")

    items_of_env = {int(i): np.flatnonzero(ids == i) for i in stored}
    rng = np.random.default_rng(0)
    plan_items = [int(i) for i in stored[:: max(1, len(stored) // args.sample)][:args.sample]]

    def plan_loop():
        tabs._host = {}  # (every repeat copies the tables back, as a first call does)
        return sum(len(tabs.optimal_plan(i) or []) for i in plan_items)

    bench_tables("", vec, [tabs], len(plan_items), plan_loop, lambda: host_sample(vec, tabs, items_of_env, rng, 1, 1 << 30), args)
    tabs.close()

    # ---- (e) one per-puzzle table
    with zipfile.ZipFile(os.path.join(ROOT, "pushworld_amd", "data", "puzzles", "level0.zip")) as z:
        text = z.read("level0/all/train/level_0_all_train_3.pwp").decode()
    vec1 = VecPushWorld([PushWorldPuzzle(text=text)], args.envs, observation=None, max_steps=None)
    tab = vec1.solution_table(0)
    print(f"\none table: level_0_all_train_3, {tab.num_states} states, max cost {tab.max_cost}")

    def index_one():
        _capi.check(_capi.lib.pw_search_solve(tab.search.handle, (_capi.c_int64 * 4)(), tab.search._stream()))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _capi.check(_capi.lib.pw_search_table_index(tab.search.handle, tab.search._stream()))
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    index_one()
    t_i = [index_one() for _ in range(args.repeats)]
    print(f"(ea) cost index of {tab.num_states} rows (the solve itself not timed): {fmt(t_i)}")
    starts = np.arange(tab.num_states)[:: max(1, tab.num_states // args.sample)][:args.sample]

    def plan_loop_one():
        tab._host = None
        return sum(len(tab.optimal_plan(int(i)) or []) for i in starts)

    def host_sample_one():
        cost = tab.costs().cpu().numpy()
        rows = np.flatnonzero((cost >= 1) & (cost != 0xFFFF))
        states = tab.states()
        pos = np.zeros((args.envs, tab.npad, 2), dtype=np.int8)
        pos[:, :states.shape[1]] = states[rows[rng.integers(0, rows.size, size=args.envs)]]
        vec1.set_states(pos)

    bench_tables("e", vec1, [tab], len(starts), plan_loop_one, host_sample_one, args)
    tab.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Measures drawing from the BATCHED cost-to-go tables over pushes (search.PushSolutionTableBatch.build_index / sample / plans /
demonstration_rows, VecPushWorld.reset_from_push_tables / optimal_push_demonstrations with a batch; pw_push_solve_batch_index /
_sample / _plans / _emit) and prints the figures kept in profiles/push_batch_sample.txt.

    python tools/bench_push_batch_sample.py [--repeats 3] > profiles/push_batch_sample.txt

K22's set -- generate_level0_set(2000, random_seed=21) at a cap of 4 096 states -- with 65 536 environments over 200 of its built
puzzles.  Every call on ONE indexed batch of those 200 puzzles is timed against the same call over the list of their 200
push_table()s, the loop it replaces:
  (a) the index build (on tables without an index: a new batch / a new pw_push_search_solve before every repeat, not timed);
  (b) the sample of the whole batch of environments;
  (c) the plans from the environments' states in both tie modes;
  (d) the emit of those plans;
  (e) VecPushWorld.reset_from_push_tables and optimal_push_demonstrations (no observations).

Timing: the host clock around synchronised calls, best of --repeats after one warm-up run, every repeat listed.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pushworld_amd import generate  # noqa: E402
from pushworld_amd.search import TABLE_BUILT, TABLE_SUMMARY_ONLY, PushSolutionTableBatch  # noqa: E402
from pushworld_amd.vec_env import VecPushWorld  # noqa: E402


def timed(fn, repeats, before=None):
    """Seconds of every repeat of fn() between two synchronisations, after one warm-up; before() runs untimed ahead of each."""
    out = []
    for k in range(repeats + 1):
        if before:
            before()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if k:
            out.append(time.perf_counter() - t0)
    return out


def ms(ts):
    return f"best {min(ts) * 1e3:9.3f} ms (" + ", ".join(f"{t * 1e3:.3f}" for t in ts) + ")"


def pair(label, t_batch, t_loop, n_tables):
    print(f"  {label}")
    print(f"      one indexed batch                     {ms(t_batch)}")
    print(f"      loop over {n_tables} push_table()s          {ms(t_loop)}: x{min(t_loop) / min(t_batch):.1f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--puzzles", type=int, default=2000)
    ap.add_argument("--tables", type=int, default=200)
    ap.add_argument("--seed", type=int, default=21)
    ap.add_argument("--max-states", type=int, default=4096)
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    rep, B, cap = args.repeats, args.envs, args.max_states
    print(f"# tools/bench_push_batch_sample.py --puzzles {args.puzzles} --tables {args.tables} --seed {args.seed} --max-states {cap} "
          f"--envs {B} --repeats {rep}")
    print(f"# {torch.cuda.get_device_name(0)}; host clock around synchronised calls, best of {rep} after a warm-up")
    pset, _, _ = generate.generate_level0_set(args.puzzles, random_seed=args.seed)
    # which puzzles fit the cap: a summary-only pass over the whole set, then every k-th built one
    probe = VecPushWorld(pset, 1, observation=None, max_steps=None)
    with PushSolutionTableBatch(probe, max_states_each=cap, states=0, rows=0) as dry:
        built = np.flatnonzero(dry.status.cpu().numpy() == TABLE_SUMMARY_ONLY)  # (built, nothing stored)
    qp = [int(i) for i in built[:: max(1, len(built) // args.tables)][:args.tables]]
    ids = np.asarray(qp, dtype=np.int64)[np.arange(B) % len(qp)]
    vec = VecPushWorld(pset, B, puzzle_ids=ids, observation=None, max_steps=None, seed=1)
    dev = vec.device
    vec.reset()
    batch = vec.push_tables(qp, max_states_each=cap, index=True)
    assert bool((batch.status == TABLE_BUILT).all())
    tables = [vec.push_table(i, max_states=cap) for i in qp]
    S = int(batch.num_states.sum())
    print(f"set: {len(pset)} puzzles, {len(built)} within the cap of {cap}; {len(qp)} of them in the batch: {S} canonical states, "
          f"{int(batch.num_rows.sum())} push rows, largest cost {batch.max_cost_stored}; {B} environments")

    # (a) the index build
    fresh = {}

    def new_batch():
        if "b" in fresh:
            fresh["b"].close()
        fresh["b"] = vec.push_tables(qp, max_states_each=cap)

    def solve_again():
        for t in tables:
            t.search._handle.solve()

    t_a = timed(lambda: fresh["b"].build_index(), rep, before=new_batch)
    t_al = timed(lambda: [t.search._handle.table_index() for t in tables], rep, before=solve_again)
    fresh["b"].close()
    pair(f"(a) index build, {S} states", t_a, t_al, len(tables))

    # (b) the sample
    out = (torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev))
    counter = torch.zeros(B, dtype=torch.int32, device=dev)

    def sample(ts):
        for t in ts:
            t.sample(vec.puzzle_id, vec.pos, vec.steps, vec.terminated, vec.truncated, cost=(1, None), seed=3, counter=counter, out=out)

    t_b, t_bl = timed(lambda: sample([batch]), rep), timed(lambda: sample(tables), rep)
    pair(f"(b) sample, cost (1, None): {B / min(t_b) * 1e-6:.1f} M draws / s in the batch", t_b, t_bl, len(tables))

    # (c) the plans from the sampled states
    sample([batch])
    width = max(batch.max_cost_stored, 1)
    owns = [t.covers(vec.puzzle_id) for t in tables]
    plans = None
    for tie in ("lowest", "uniform"):
        q = vec.push_cost_to_go([batch])
        plans = batch.plans(q.index, vec.puzzle_id, tie=tie, seed=2, plan_cap=width)
        t_c = timed(lambda: batch.plans(q.index, vec.puzzle_id, tie=tie, seed=2, plan_cap=width, out=plans), rep)
        ql = vec.push_cost_to_go(tables)
        lplans = batch.plans(q.index, vec.puzzle_id, tie=tie, seed=2, plan_cap=width)

        def loop_plans():
            for t, own in zip(tables, owns):
                t.plans(ql.index, vec.puzzle_id, mask=own, tie=tie, seed=2, plan_cap=width, out=lplans)

        t_cl = timed(loop_plans, rep)
        same = bool((lplans.length == plans.length).all()) and bool((lplans.push_action == plans.push_action).all())
        pair(f"(c) plans, tie {tie}, plan_cap {width}: {min(t_c) / B * 1e9:.2f} ns / plan in the batch; same pushes: {same}",
             t_c, t_cl, len(tables))

    # (d) the emit (tie uniform's plans)
    offset = torch.zeros(B + 1, dtype=torch.int64, device=dev)
    torch.cumsum(plans.length.clamp(min=0), 0, out=offset[1:])
    T = int(offset[B].cpu())
    rows = batch.demonstration_rows(plans, pos=vec.pos, puzzle_id=vec.puzzle_id, offset=offset, rows_cap=T)
    t_d = timed(lambda: batch.demonstration_rows(plans, pos=vec.pos, puzzle_id=vec.puzzle_id, offset=offset, out=rows), rep)
    lrows = tables[0].demonstration_rows(lplans, pos=vec.pos, puzzle_id=vec.puzzle_id, mask=owns[0], offset=offset, rows_cap=T)

    def loop_emit():
        for t, own in zip(tables, owns):
            t.demonstration_rows(lplans, pos=vec.pos, puzzle_id=vec.puzzle_id, mask=own, offset=offset, out=lrows)

    t_dl = timed(loop_emit, rep)
    same = bool((lrows.pos == rows.pos).all()) and bool((lrows.cost == rows.cost).all())
    pair(f"(d) emit of {T} rows: {T / min(t_d) * 1e-6:.1f} M rows / s in the batch; same rows: {same}", t_d, t_dl, len(tables))

    # (e) the environment's entry points
    t_e = timed(lambda: vec.reset_from_push_tables([batch], cost=(1, None)), rep)
    t_el = timed(lambda: vec.reset_from_push_tables(tables, cost=(1, None)), rep)
    pair("(e) VecPushWorld.reset_from_push_tables, cost (1, None)", t_e, t_el, len(tables))
    vec.reset_from_push_tables([batch], cost=(1, None), seed=5)
    t_f = timed(lambda: vec.optimal_push_demonstrations([batch], observation=None), rep)
    t_fl = timed(lambda: vec.optimal_push_demonstrations(tables, observation=None), rep)
    pair("    VecPushWorld.optimal_push_demonstrations, observation None", t_f, t_fl, len(tables))
    for t in tables:
        t.close()
    batch.close()


if __name__ == "__main__":
    main()

#!/usr/bin/env python
"""Batched cost-to-go tables (search.SolutionTableBatch) on device-generated Level-0 puzzles:

  (a) the batched build of the whole set -- summary only (rows=0) and storing (rows = what the summary pass reports);
  (b) the per-puzzle way on a sample of the same set: a loop of search.SolutionTable;
  (c) one batched query of 65 536 live states against the loop of per-table queries over the sample;
  and the tail of the persistent schedule: the largest puzzle of the set built alone (one workgroup).

Wall-clock seconds around a synchronised call, best of --repeats after one warm-up; the spread of the repeats is printed.

    python tools/bench_solution_batch.py [--puzzles 2000] [--sample 200] > profiles/solution_batch.txt
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, repeats):
    import torch

    fn()  # warm-up: slabs, pools, code objects
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--puzzles", type=int, default=2000)
    ap.add_argument("--sample", type=int, default=200)
    ap.add_argument("--seed", type=int, default=21)
    ap.add_argument("--max-states", type=int, default=1 << 16)
    ap.add_argument("--queries", type=int, default=65536)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()

    import torch

    from pushworld_amd import _capi, generate
    from pushworld_amd.search import SetPuzzle, SolutionTable, SolutionTableBatch

    print(f"# tools/bench_solution_batch.py --puzzles {args.puzzles} --sample {args.sample} --seed {args.seed} "
          f"--max-states {args.max_states} --queries {args.queries} --repeats {args.repeats}")
    print(f"# {torch.cuda.get_device_name(0)}")
    pset, _, _ = generate.generate_level0_set(args.puzzles, random_seed=args.seed)
    eng = _capi.Engine(pset, None, 3, 1, _capi.OBS_U8)
    n = len(pset)

    # ---- (a) the batched build
    def build(rows):
        b = SolutionTableBatch(eng, max_states_each=args.max_states, rows=rows)
        b.close()

    probe = SolutionTableBatch(eng, max_states_each=args.max_states, rows=0)
    status, states = probe.status.cpu().numpy(), probe.num_states.cpu().numpy()
    needed = probe.rows_needed
    probe.close()
    valid = (status == 0) | (status == 4)
    hist = {int(s): int((status == s).sum()) for s in np.unique(status)}
    print(f"set: {n} puzzles, status histogram (summary pass) {hist}, {needed} states in {int(valid.sum())} tables "
          f"(median {int(np.median(states[valid]))}, largest {int(states[valid].max())})")
    t_sum = timed(lambda: build(0), args.repeats)
    t_store = timed(lambda: build(needed), args.repeats)
    print(f"(a) batched build, summary only : {fmt(t_sum)}   {n / min(t_sum):12.0f} puzzles/s {needed / min(t_sum):14.0f} states/s")
    print(f"(a) batched build, rows stored  : {fmt(t_store)}   {n / min(t_store):12.0f} puzzles/s {needed / min(t_store):14.0f} states/s")
    full = SolutionTableBatch(eng, max_states_each=args.max_states, rows=needed)
    st = full.status.cpu().numpy()
    print(f"    status histogram (storing pass) { {int(s): int((st == s).sum()) for s in np.unique(st)} }")

    # the tail: the largest puzzle alone occupies ONE workgroup for as long as the whole launch cannot be shorter than
    largest = int(np.argmax(np.where(valid, states, -1)))

    def alone():
        b = SolutionTableBatch(eng, [largest], max_states_each=args.max_states, rows=int(states[largest]))
        b.close()

    t_tail = timed(alone, args.repeats)
    print(f"    largest puzzle alone ({int(states[largest])} states, one workgroup): {fmt(t_tail)}   "
          f"{min(t_tail) / min(t_store):.2f} of the storing build")

    # ---- (b) the per-puzzle way on a sample
    sample = [int(i) for i in np.flatnonzero(valid)[:: max(1, int(valid.sum()) // args.sample)][:args.sample]]
    sample_states = int(states[sample].sum())

    def loop():
        for i in sample:
            SolutionTable(SetPuzzle(pset, i, eng), max_states=args.max_states).close()

    t_loop = timed(loop, args.repeats)
    per_batch, per_loop = min(t_store) / n, min(t_loop) / len(sample)
    print(f"(b) loop of SolutionTable, {len(sample)} puzzles ({sample_states} states): {fmt(t_loop)}   "
          f"{len(sample) / min(t_loop):12.0f} puzzles/s {sample_states / min(t_loop):14.0f} states/s")
    spread = (max(t_loop) - min(t_loop)) / min(t_loop)
    print(f"    per puzzle: batched {per_batch * 1e6:.2f} us, loop {per_loop * 1e6:.2f} us: x{per_loop / per_batch:.1f} "
          f"(spread of the loop's repeats {spread * 100:.1f} %, of the batched build's "
          f"{(max(t_store) - min(t_store)) / min(t_store) * 100:.1f} %)")

    # ---- (c) queries: the initial states of the sample's puzzles, cycled
    tables = [SolutionTable(SetPuzzle(pset, i, eng), max_states=args.max_states) for i in sample]
    ids = np.array(sample, dtype=np.int32)[np.arange(args.queries) % len(sample)]
    pos = np.zeros((args.queries, eng.np, 2), dtype=np.int8)
    starts = {i: np.array(SetPuzzle(pset, i, eng).initial_state, dtype=np.int8) for i in sample}
    for k, i in enumerate(ids):
        pos[k, :len(starts[int(i)])] = starts[int(i)]
    ids_d, pos_d = torch.as_tensor(ids).to(eng.device), torch.as_tensor(pos).to(eng.device)
    out = full.query(ids_d, pos_d)
    t_q = timed(lambda: full.query(ids_d, pos_d, out=out), args.repeats)

    def query_loop():
        for t in tables:
            t.query(ids_d, pos_d, out=out2)

    out2 = tables[0].query(ids_d, pos_d)
    t_ql = timed(query_loop, args.repeats)
    same = all(bool((a[1] == b[1]).all()) and bool((a[2] == b[2]).all()) for a, b in ((out, out2),))
    print(f"(c) query of {args.queries} states: batched (1 launch) {fmt(t_q)}")
    print(f"    loop of {len(tables)} per-table queries      {fmt(t_ql)}   x{min(t_ql) / min(t_q):.1f}   same cost / acts: {same}")
    for t in tables:
        t.close()
    full.close()


if __name__ == "__main__":
    main()

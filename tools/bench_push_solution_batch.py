#!/usr/bin/env python
"""Batched cost-to-go tables over pushes (search.PushSolutionTableBatch) on device-generated Level-0 puzzles:

  (a) the batched build of the whole set -- summary only (pools 0 / 0) and storing (pools = what the summary pass reports);
  (b) the tail of the persistent schedule: the largest item of the set built alone (one workgroup);
  (c) the per-puzzle way on a sample of the built puzzles, on the same device in the same session: a loop of
      search.PushSolutionTable;
  (d) one batched query of 65 536 live states over 200 puzzles against 200 per-table queries (pw_push_search_table_query).

Wall-clock seconds around a synchronised call that includes creating and destroying the handle, best of --repeats after one
warm-up; every repeat is printed.

    python tools/bench_push_solution_batch.py [--puzzles 2000] [--sample 100] > profiles/push_solution_batch.txt
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
    ap.add_argument("--sample", type=int, default=100)
    ap.add_argument("--query-puzzles", type=int, default=200)
    ap.add_argument("--seed", type=int, default=21)
    ap.add_argument("--max-states", type=int, default=4096)
    ap.add_argument("--queries", type=int, default=65536)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()

    import torch

    from pushworld_amd import _capi, generate
    from pushworld_amd.search import PushSolutionTable, PushSolutionTableBatch, SetPuzzle

    print(f"# tools/bench_push_solution_batch.py --puzzles {args.puzzles} --sample {args.sample} --query-puzzles "
          f"{args.query_puzzles} --seed {args.seed} --max-states {args.max_states} --queries {args.queries} --repeats {args.repeats}")
    print(f"# {torch.cuda.get_device_name(0)}")
    pset, _, _ = generate.generate_level0_set(args.puzzles, random_seed=args.seed)
    eng = _capi.Engine(pset, None, 3, 1, _capi.OBS_U8)
    n = len(pset)

    # ---- (a) the batched build
    def build(states, rows):
        PushSolutionTableBatch(eng, max_states_each=args.max_states, states=states, rows=rows).close()

    probe = PushSolutionTableBatch(eng, max_states_each=args.max_states, states=0, rows=0)
    status, summary = probe.status.cpu().numpy(), probe.summary.cpu().numpy()
    need_s, need_r = probe.states_needed, probe.rows_needed
    probe.close()
    valid = (status == 0) | (status == 4)
    S, R = summary[:, 0], summary[:, 1]
    hist = {int(s): int((status == s).sum()) for s in np.unique(status)}
    tot_s, tot_r = int(S[valid].sum()), int(R[valid].sum())
    print(f"set: {n} puzzles, cap {args.max_states} states; status histogram (summary pass) {hist}; {int(valid.sum())} spaces fit "
          f"the cap ({valid.mean() * 100:.1f} %): {tot_s} states (median {int(np.median(S[valid]))}, largest {int(S[valid].max())}), "
          f"{tot_r} rows ({tot_r / max(tot_s, 1):.2f} per state)")
    solved = valid & (summary[:, 5] >= 0)
    print(f"     solvable {int(solved.sum())}, fewest pushes: median {int(np.median(summary[solved, 5])) if solved.any() else -1}, "
          f"largest {int(summary[solved, 5].max()) if solved.any() else -1}; dead-end share of the built spaces "
          f"{summary[valid, 3].sum() / max(tot_s, 1):.3f}")
    t_sum = timed(lambda: build(0, 0), args.repeats)
    t_store = timed(lambda: build(need_s, need_r), args.repeats)
    for name, ts in (("summary only", t_sum), ("stored      ", t_store)):
        print(f"(a) batched build, {name}: {fmt(ts)}   {n / min(ts):10.0f} puzzles/s {tot_s / min(ts):12.0f} states/s "
              f"{tot_r / min(ts):12.0f} rows/s")
    full = PushSolutionTableBatch(eng, max_states_each=args.max_states, states=need_s, rows=need_r)
    st = full.status.cpu().numpy()
    print(f"    status histogram (storing pass) { {int(s): int((st == s).sum()) for s in np.unique(st)} }, missing successors {full.missing}")

    # ---- (b) the tail
    largest = int(np.argmax(np.where(valid, S, -1)))

    def alone():
        PushSolutionTableBatch(eng, [largest], max_states_each=args.max_states, states=int(S[largest]) + 1, rows=int(R[largest])).close()

    t_tail = timed(alone, args.repeats)
    print(f"(b) largest item alone ({int(S[largest])} states, {int(R[largest])} rows, one workgroup): {fmt(t_tail)}   "
          f"{min(t_tail) / min(t_store):.2f} of the storing build")

    # ---- (c) the per-puzzle way on a sample of the built puzzles
    built = np.flatnonzero(valid)
    sample = [int(i) for i in built[:: max(1, len(built) // args.sample)][:args.sample]]
    sample_s, sample_r = int(S[sample].sum()), int(R[sample].sum())

    def loop():
        for i in sample:
            PushSolutionTable(SetPuzzle(pset, i, eng), max_states=args.max_states).close()

    t_loop = timed(loop, args.repeats)
    per_batch, per_loop = min(t_store) / n, min(t_loop) / len(sample)
    print(f"(c) loop of PushSolutionTable, {len(sample)} puzzles ({sample_s} states, {sample_r} rows): {fmt(t_loop)}   "
          f"{len(sample) / min(t_loop):10.0f} puzzles/s {sample_s / min(t_loop):12.0f} states/s")
    print(f"    per puzzle: batched {per_batch * 1e6:.2f} us (every puzzle of the set, those beyond the cap included), loop "
          f"{per_loop * 1e6:.2f} us: x{per_loop / per_batch:.1f}; per state: batched {min(t_store) / max(tot_s, 1) * 1e9:.1f} ns, loop "
          f"{min(t_loop) / max(sample_s, 1) * 1e9:.1f} ns: x{(min(t_loop) / max(sample_s, 1)) / (min(t_store) / max(tot_s, 1)):.1f}")
    print(f"    spread of the repeats: loop {(max(t_loop) - min(t_loop)) / min(t_loop) * 100:.1f} %, batched build "
          f"{(max(t_store) - min(t_store)) / min(t_store) * 100:.1f} %")

    # ---- (d) queries: the initial states of the query puzzles, cycled
    qp = [int(i) for i in built[:: max(1, len(built) // args.query_puzzles)][:args.query_puzzles]]
    tables = [PushSolutionTable(SetPuzzle(pset, i, eng), max_states=args.max_states) for i in qp]
    ids = np.array(qp, dtype=np.int32)[np.arange(args.queries) % len(qp)]
    pos = np.zeros((args.queries, eng.np, 2), dtype=np.int8)
    starts = {i: np.array(SetPuzzle(pset, i, eng).initial_state, dtype=np.int8) for i in qp}
    for k, i in enumerate(ids):
        pos[k, :len(starts[int(i)])] = starts[int(i)]
    ids_d, pos_d = torch.as_tensor(ids).to(eng.device), torch.as_tensor(pos).to(eng.device)
    out = full.query(ids_d, pos_d)
    t_q = timed(lambda: full.query(ids_d, pos_d, out=out), args.repeats)
    t_q0 = timed(lambda: full.query(ids_d, pos_d, out=out, actions=False), args.repeats)
    out2 = tables[0].query(ids_d, pos_d)

    def query_loop():
        for t in tables:
            t.query(ids_d, pos_d, out=out2)

    t_ql = timed(query_loop, args.repeats)
    same = all(bool((getattr(out, f) == getattr(out2, f)).all()) for f in ("cost", "action", "push_from", "push_action", "walk"))
    print(f"(d) query of {args.queries} states over {len(qp)} puzzles: batched (1 launch) {fmt(t_q)}")
    print(f"    the same without walk / action                {fmt(t_q0)}")
    print(f"    loop of {len(tables)} per-table queries              {fmt(t_ql)}   x{min(t_ql) / min(t_q):.1f}   "
          f"same cost / action / push / walk: {same}")
    for t in tables:
        t.close()
    full.close()


if __name__ == "__main__":
    main()

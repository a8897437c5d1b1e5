"""Measures pushes unrolled into primitive actions (search.unroll_pushes / push_rows_to_plans, VecPushWorld.fewest_push_plans;
pw_push_unroll_count / _write / _plans) and prints the figures kept in profiles/push_unroll.txt.

    python tools/bench_push_unroll.py [--repeats 3] [--sample 512] > profiles/push_unroll.txt

On tests/deep_puzzles.room3() and big(), a batch of 65 536 environments drawn with reset_from_push_tables, over the rows of
VecPushWorld.optimal_push_demonstrations (observation None):
  (a) pw_push_unroll_count and pw_push_unroll_write over the rows, each by itself;
  (b) the gather pw_push_unroll_plans;
  (c) VecPushWorld.fewest_push_plans as a whole (query, plans, emit, count, write, gather; two host waits);
  (d) fewest_push_plans followed by search.replay_plans (verdicts and one row per primitive step);
  (e) the procedure this replaces, on the same rows: walk_regions(maps=True) over the rows and the copy of the maps to the
      host (timed over all rows), then WalkRegions.path per row on the host, timed over --sample rows and scaled to all of
      them; and PushSolutionTable.optimal_plan per plan on 64 states, scaled to the batch.

Timing: the host clock around synchronised calls, best of --repeats after one warm-up run, every repeat listed.
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import deep_puzzles  # noqa: E402
from pushworld_amd.puzzle import PushWorldPuzzle  # noqa: E402
from pushworld_amd.search import REPLAY_VALID, replay_plans, unroll_pushes, walk_regions  # noqa: E402
from pushworld_amd.vec_env import VecPushWorld  # noqa: E402

B = 65536


def timed(fn, repeats):
    """Seconds of every repeat of fn() between two synchronisations, after one warm-up."""
    out = []
    for k in range(repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if k:
            out.append(time.perf_counter() - t0)
    return out


def ms(ts):
    return f"best {min(ts) * 1e3:.3f} ms (" + ", ".join(f"{t * 1e3:.3f}" for t in ts) + ")"


def measure(label, text, rep, sample):
    pz = PushWorldPuzzle(text=text)
    vec = VecPushWorld([pz], B, observation=None, max_steps=None, seed=1)
    dev, engine = vec.device, vec.engine
    with vec.push_table(0, max_states=1 << 20) as tab:
        vec.reset_from_push_tables([tab], cost=(1, None), seed=3)
        d = vec.optimal_push_demonstrations([tab], observation=None)
        T = d.num_rows
        ids = d.puzzle_id
        u = unroll_pushes(engine, ids, d.push_from, d.push_action, pos=d.pos)
        assert int((u.length < 0).sum()) == 0
        print(f"{label}: {tab.num_states} canonical states, largest cost {tab.max_cost}; {B} environments, {T} push rows, "
              f"{u.num_actions} primitive actions ({u.num_actions / T:.2f} per push, {int(u.length.max())} at the most)")
        # (a)
        length = torch.empty(T, dtype=torch.int32, device=dev)
        offset = torch.empty(T + 1, dtype=torch.int64, device=dev)
        actions = torch.empty(u.num_actions, dtype=torch.uint8, device=dev)
        t_count = timed(lambda: engine.push_unroll_count(ids, d.pos, d.push_from, d.push_action, None, length, offset), rep)
        t_write = timed(lambda: engine.push_unroll_write(ids, d.pos, d.push_from, d.push_action, None, offset, u.num_actions,
                                                         actions), rep)
        assert torch.equal(actions, u.actions)
        print(f"  (a) pw_push_unroll_count (flood to `from`, scan)   {ms(t_count)}: {T / min(t_count) * 1e-6:.1f} M rows / s")
        print(f"      pw_push_unroll_write (flood, walk back)        {ms(t_write)}: {u.num_actions / min(t_write) * 1e-6:.1f} M actions / s")
        # (b)
        item_offset = torch.zeros(B + 1, dtype=torch.int64, device=dev)
        torch.cumsum(torch.bincount(d.item.long(), minlength=B), 0, out=item_offset[1:])
        plans = torch.zeros((B, 1024), dtype=torch.uint8, device=dev)
        plan_len = torch.zeros(B, dtype=torch.int32, device=dev)
        t_gather = timed(lambda: engine.push_unroll_plans(item_offset, length, offset, actions, T, u.num_actions, plans, plan_len),
                         rep)
        print(f"  (b) pw_push_unroll_plans (gather, plan_cap 1024)   {ms(t_gather)}")
        # (c), (d)
        t_all = timed(lambda: vec.fewest_push_plans([tab]), rep)
        print(f"  (c) fewest_push_plans                              {ms(t_all)}: {min(t_all) / B * 1e6:.3f} us / plan")
        r = vec.fewest_push_plans([tab])
        assert torch.equal(r.plans, plans) and torch.equal(r.plan_len, plan_len)

        def both():
            q = vec.fewest_push_plans([tab])
            return replay_plans(vec, vec.puzzle_id, q.plans, q.plan_len, pos=vec.pos)

        rp = both()
        assert bool((rp.verdict == REPLAY_VALID).all()) and rp.num_rows == u.num_actions
        t_both = timed(both, rep)
        print(f"  (d) fewest_push_plans + replay_plans ({rp.num_rows} rows)  {ms(t_both)}")
        # (e)
        host = {}

        def maps():
            reg = walk_regions(engine, ids, d.pos, maps=True)
            host["maps"] = reg.walk_map.cpu()
            host["reg"] = reg

        t_maps = timed(maps, rep)
        reg = host["reg"]
        n = min(sample, T)
        pick = torch.linspace(0, T - 1, n).long().tolist()
        frm = d.push_from.cpu().tolist()
        maps_np = host["maps"].numpy()
        reg._host_maps = {i: maps_np[i] for i in pick}  # (the maps are on the host already: path() copies none again)

        def paths():
            for i in pick:
                reg.path(i, frm[i])

        t_path = timed(paths, rep)
        per_row = min(t_path) / n
        print(f"  (e) host: walk_regions(maps=True) + maps to the host ({host['maps'].numel() * 2 / 2**20:.0f} MiB)  {ms(t_maps)}")
        print(f"      host: WalkRegions.path on a sample of {n} rows   {ms(t_path)}: {per_row * 1e6:.1f} us / row; "
              f"{T} rows at that rate {per_row * T:.1f} s")
        print(f"      (maps + paths at that rate) / (count + write + gather) = "
              f"{(min(t_maps) + per_row * T) / (min(t_count) + min(t_write) + min(t_gather)):.0f}")
        hpos = vec.pos[:64, :pz.num_movables].cpu().numpy()
        starts = [tuple(tuple(int(v) for v in xy) for xy in s) for s in hpos]
        t_loop = timed(lambda: [tab.optimal_plan(s) for s in starts], rep)
        print(f"      host: optimal_plan loop on 64 states            {ms(t_loop)}: {min(t_loop) / 64 * 1e3:.2f} ms / plan; "
              f"{B} plans at that rate {min(t_loop) / 64 * B:.0f} s against {min(t_all) * 1e3:.3f} ms (c)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sample", type=int, default=512)
    args = ap.parse_args()
    print(f"# tools/bench_push_unroll.py --repeats {args.repeats} --sample {args.sample}")
    print(f"# {torch.cuda.get_device_name(0)}; host clock around synchronised calls, best of {args.repeats} after a warm-up")
    measure("room3", deep_puzzles.room3(), args.repeats, args.sample)
    measure("big", deep_puzzles.big(), args.repeats, args.sample)


if __name__ == "__main__":
    main()

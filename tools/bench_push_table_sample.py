"""Measures drawing from the cost-to-go tables over pushes (search.PushSolutionTable.cost_index / sample / plans /
demonstration_rows, VecPushWorld.optimal_push_demonstrations; pw_push_search_table_index / _sample / _plans / _emit, DESIGN.md
K20) and prints the figures kept in profiles/push_table_sample.txt.

    python tools/bench_push_table_sample.py [--repeats 3] > profiles/push_table_sample.txt

On tests/deep_puzzles.room3() and big(), a batch of 65 536 environments:
  (a) the index build (on a table whose index was discarded: a new pw_push_search_solve before every repeat, not timed);
  (b) the sample of the whole batch, against the host procedure it replaces -- states() / costs() to the host, a numpy draw
      from the band, set_states;
  (c) the plans of the whole batch in both tie modes, against PushSolutionTable.optimal_plan (one query launch and two waits
      per primitive step) on 64 states, scaled per state;
  (d) the emit of those plans;
  (e) VecPushWorld.optimal_push_demonstrations, without observations and with the environment's own.

Timing: the host clock around synchronised calls, best of --repeats after one warm-up run, every repeat listed.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import deep_puzzles  # noqa: E402
from pushworld_amd.puzzle import PushWorldPuzzle  # noqa: E402
from pushworld_amd.vec_env import VecPushWorld  # noqa: E402

B = 65536


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
    return f"best {min(ts) * 1e3:.3f} ms (" + ", ".join(f"{t * 1e3:.3f}" for t in ts) + ")"


def measure(label, text, rep):
    pz = PushWorldPuzzle(text=text)
    vec = VecPushWorld([pz], B, observation="cells", max_steps=None, seed=1)
    dev = vec.device
    vec.reset()
    with vec.push_table(0, max_states=1 << 20) as tab:
        h = tab.search._handle
        print(f"{label}: {tab.num_states} canonical states, {tab.num_rows} push rows, largest cost {tab.max_cost}; {B} environments")
        # (a)
        t_index = timed(h.table_index, rep, before=h.solve)
        print(f"  (a) index build (sort by bucket, scan)           {ms(t_index)}")
        # (b)
        out = (torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev))
        counter = torch.zeros(B, dtype=torch.int32, device=dev)

        def sample():
            tab.sample(None, vec.pos, vec.steps, vec.terminated, vec.truncated, cost=(1, None), seed=3, counter=counter, out=out)

        rng = np.random.default_rng(3)

        def host_sample():
            pos = tab.states()[0].cpu().numpy()
            cost = tab.costs().cpu().numpy()
            band = np.flatnonzero(cost >= 1)
            vec.set_states(pos[band[rng.integers(0, band.size, B)]])

        t_sample, t_host = timed(sample, rep), timed(host_sample, rep)
        print(f"  (b) sample, cost (1, None)                       {ms(t_sample)}: {B / min(t_sample) * 1e-6:.1f} M draws / s")
        print(f"      host: states() / costs(), numpy, set_states  {ms(t_host)}: x{min(t_host) / min(t_sample):.0f}")
        # (c)
        sample()
        index = out[0].clone()
        cap = max(tab.max_cost, 1)
        plans = tab.plans(index, plan_cap=cap)
        t_tie = {}
        for tie in ("uniform", "lowest"):
            t_tie[tie] = timed(lambda: tab.plans(index, tie=tie, seed=2, plan_cap=cap, out=plans), rep)
            print(f"  (c) plans, tie {tie:<8} plan_cap {cap:<3}             {ms(t_tie[tie])}: "
                  f"{min(t_tie[tie]) / B * 1e9:.2f} ns / plan")
        hpos = vec.pos[:64, :pz.num_movables].cpu().numpy()
        starts = [tuple(tuple(int(v) for v in xy) for xy in s) for s in hpos]
        t_loop = timed(lambda: [tab.optimal_plan(s) for s in starts], rep)
        print(f"      host: optimal_plan loop on 64 states         {ms(t_loop)}: {min(t_loop) / 64 * 1e3:.2f} ms / plan; "
              f"{B} plans at that rate {min(t_loop) / 64 * B:.0f} s against {min(t_tie['lowest']) * 1e3:.3f} ms (tie lowest)")
        # (d)
        rows = tab.demonstration_rows(plans, pos=vec.pos)
        t_emit = timed(lambda: tab.demonstration_rows(plans, pos=vec.pos, out=rows), rep)
        print(f"  (d) emit of {rows.num_rows} rows (cumsum and launch)       {ms(t_emit)}: "
              f"{rows.num_rows / min(t_emit) * 1e-6:.1f} M rows / s")
        # (e)
        for obs in (None, "own"):
            t_demo = timed(lambda: vec.optimal_push_demonstrations([tab], observation=obs), rep)
            print(f"  (e) optimal_push_demonstrations, observation {str(obs):<5} {ms(t_demo)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    print(f"# tools/bench_push_table_sample.py --repeats {args.repeats}")
    print(f"# {torch.cuda.get_device_name(0)}; host clock around synchronised calls, best of {args.repeats} after a warm-up")
    measure("room3", deep_puzzles.room3(), args.repeats)
    measure("big", deep_puzzles.big(), args.repeats)


if __name__ == "__main__":
    main()

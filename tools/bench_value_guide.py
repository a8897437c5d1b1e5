"""Measures the cost-to-go guidance inside the step (pw_guide_step, guide.ValueGuide, VecPushWorld.set_guide) and
prints the figures kept in profiles/value_guide.txt.

    python tools/bench_value_guide.py [--envs 65536] [--steps 50] [--repeats 7] [--policy-steps 300] > profiles/value_guide.txt

The set is K26's benchmark set (tools/bench_start_pool.py part 3): 200 of generate_level0_set(2000, random_seed=21) within 4 096
canonical states, one move-level SolutionTableBatch over them; max_steps 100, autoreset, state only.

  (1) the step loop, four environments with the same seeds, interleaved in one process (every loop once per round, round 0 is
      the warm-up; device synchronise around each window of --steps steps), medians and ranges over --repeats rounds:
        (a) `step` without a guide -- the parent's path;
        (b) `step` with the fused guide (ONE pw_guide_step launch behind the step);
        (c) today's composition for the same outputs: `step`, then vec.cost_to_go([batch]) and the torch ops that make the dead
            flags, the cut, the shaped reward, the counts and the seen flags;
        (d) `step` with the applied form (the batch's own query launch, then pw_guide_step).
      Accepted when (b) - (a) is below (c) - (a) in every round and the two ranges do not overlap.
  (2) one exact count: a uniform random policy for --policy-steps steps without and with end_dead -- env-steps and ended episodes
      from pw_counters, the dead ends entered from the guide's counts, and the env-steps spent in dead states (the sum of the
      guide's dead flags behind every step, accumulated on the device).
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pushworld_amd.vec_env import VecPushWorld  # noqa: E402

GAMMA, SCALE = 0.99, 0.1


def level0_set(B):
    """K26's set (tools/bench_start_pool.py part 3), the environments grouped by puzzle."""
    from pushworld_amd import generate
    from pushworld_amd.search import TABLE_SUMMARY_ONLY, PushSolutionTableBatch

    pset, _, _ = generate.generate_level0_set(2000, random_seed=21)
    probe = VecPushWorld(pset, 1, observation=None, max_steps=None)
    with PushSolutionTableBatch(probe, max_states_each=4096, states=0, rows=0) as dry:
        built = np.flatnonzero(dry.status.cpu().numpy() == TABLE_SUMMARY_ONLY)
    qp = [int(i) for i in built[:: max(1, len(built) // 200)][:200]]
    ids = np.asarray(qp, dtype=np.int64)[(np.arange(B) * len(qp)) // B]  # grouped by puzzle, as a bound batch is
    return pset, qp, ids


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def composition(vec, batch, dead_cost, counts, state):
    """What a user composes today behind every step for the guide's outputs."""
    P = counts.shape[0]
    pid = vec.puzzle_id.long()

    def run():
        _, c, a = vec.cost_to_go([batch])
        c_prev, seen = state["cost"], state["seen"]
        done = (vec.terminated | vec.truncated) != 0
        refused = vec.terminated == 0xFF
        dead = c == -1
        cut = dead & ~done & ~seen
        vec.truncated.masked_fill_(cut, 1)
        known = (c != -2) & (c_prev != -2)
        flat = seen | refused | ~known
        dc = dead_cost[pid]
        phi = -(SCALE * torch.where(dead, dc, c).double())
        phi_prev = -(SCALE * torch.where(c_prev == -1, dc, c_prev).double())
        state["shaped"] = vec.reward + torch.where(flat, 0.0, GAMMA * phi - phi_prev)
        live = ~seen & ~refused
        guided = live & known
        cols = torch.stack([guided, guided & (c_prev > 0) & (c == c_prev - 1), guided & dead & (c_prev >= 0), live & (c == -2)], 1)
        counts.index_add_(0, pid, cols.long())
        state["cost"], state["acts"], state["dead"], state["seen"] = c, a, dead, done | cut
    assert P == len(dead_cost)
    return run


def step_loops(args, pset, qp, ids):
    B, T = args.envs, args.steps
    kw = dict(puzzle_ids=ids, observation=None, max_steps=100, autoreset=True)
    vecs = [VecPushWorld(pset, B, **kw) for _ in range(4)]
    dev = vecs[0].device
    batches = [v.solution_tables(qp) for v in vecs[1:]]
    built = int((batches[0].status == 0).sum())
    print(f"(1) {len(pset)} generated puzzles, {len(qp)} in the move-level batch ({built} stored, "
          f"{int(batches[0].num_states[batches[0].status == 0].sum())} rows); {B} environments, max_steps 100, {T} steps per window")
    fused = vecs[1].set_guide(batches[0], gamma=GAMMA, scale=SCALE, end_dead=True)
    applied = vecs[3].set_guide([batches[2]], gamma=GAMMA, scale=SCALE, end_dead=True)
    counts = torch.zeros_like(fused.counts)
    for v in vecs:
        v.reset()
    state = dict(cost=vecs[2].cost_to_go([batches[1]])[1], seen=torch.zeros((B,), dtype=torch.bool, device=dev))
    compose = composition(vecs[2], batches[1], fused.dead_cost, counts, state)
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    acts = torch.randint(0, 4, (T, B), dtype=torch.uint8, device=dev, generator=gen)

    def loop(v, behind=None):
        def run():
            for t in range(T):
                v.step(acts[t])
                if behind is not None:
                    behind()
        return run

    loops = [loop(vecs[0]), loop(vecs[1]), loop(vecs[2], compose), loop(vecs[3])]
    times = [[] for _ in loops]
    for k in range(args.repeats + 1):
        for ts, fn in zip(times, loops):
            t = clock(fn) / T * 1e6
            if k:
                ts.append(t)
    # the four environments did the same thing
    same = all(torch.equal(vecs[1].pos, v.pos) and torch.equal(vecs[1].truncated, v.truncated) for v in vecs[2:])
    same = same and torch.equal(fused.cost, state["cost"]) and torch.equal(fused.cost, applied.cost) \
        and torch.equal(fused.counts, counts) and torch.equal(fused.counts, applied.counts) \
        and torch.equal(fused.shaped.view(torch.int64), applied.shaped.view(torch.int64))
    print(f"  the fused guide, the composition and the applied form left the same states, costs and counts: {same}")

    def line(name, ts):
        return f"  {name}: median {np.median(ts):.2f} us per step, range {min(ts):.2f} .. {max(ts):.2f}  (" + \
            ", ".join(f"{t:.2f}" for t in ts) + ")"

    for name, ts in zip(("(a) step, no guide            ", "(b) step + fused guide        ", "(c) step + composition        ",
                         "(d) step + applied guide      "), times):
        print(line(name, ts))
    a, b, c, d = (np.asarray(ts) for ts in times)
    for name, x in (("(b) - (a)", b - a), ("(c) - (a)", c - a), ("(d) - (a)", d - a)):
        print(f"  {name}, round by round: median {np.median(x):+.2f} us, range {x.min():+.2f} .. {x.max():+.2f}")
    ok = (b - a).max() < (c - a).min()
    print(f"  accepted ((b) - (a) below (c) - (a), ranges apart): {ok}; the composition costs x{np.median(c - a) / np.median(b - a):.1f} "
          f"the fused guide")
    for bt in batches:
        bt.close()


def policy_count(args, pset, qp, ids):
    B, T = args.envs, args.policy_steps
    print(f"(2) a uniform random policy, {B} environments, max_steps 100, {T} steps")
    for end_dead in (False, True):
        vec = VecPushWorld(pset, B, puzzle_ids=ids, observation=None, max_steps=100, autoreset=True)
        batch = vec.solution_tables(qp)
        guide = vec.set_guide(batch, end_dead=end_dead)
        vec.reset()
        vec.counters_reset()
        gen = torch.Generator(device=vec.device).manual_seed(args.seed)
        dead_steps = torch.zeros((), dtype=torch.int64, device=vec.device)
        known_steps = torch.zeros((), dtype=torch.int64, device=vec.device)
        # the environments whose puzzle can be solved from its initial state at all (the generator does not promise that)
        alive = torch.zeros((len(pset),), dtype=torch.bool, device=vec.device)
        alive[torch.as_tensor(qp, device=vec.device)] = (batch.status == 0) & (batch.start_cost >= 0)
        alive = alive[vec.puzzle_id.long()]
        alive_dead, alive_known = torch.zeros_like(dead_steps), torch.zeros_like(dead_steps)
        for _ in range(T):
            vec.step(torch.randint(0, 4, (B,), dtype=torch.uint8, device=vec.device, generator=gen))
            dead_steps += guide.dead.sum()
            known_steps += (guide.cost != -2).sum()
            alive_dead += (guide.dead.bool() & alive).sum()
            alive_known += ((guide.cost != -2) & alive).sum()
        c, st = vec.counters(), guide.stats()
        dead, known = int(dead_steps), int(known_steps)
        print(f"  end_dead={end_dead}: env_steps {c['env_steps']}, episodes_ended {c['episodes_ended']}, episodes_solved "
              f"{c['episodes_solved']}; guided steps {int(st.guided.sum())}, optimal {int(st.optimal.sum())}, dead ends entered "
              f"{int(st.dead_entered.sum())}, unknown {int(st.unknown.sum())}; env-steps that ended in a dead state {dead} of "
              f"{known} with a known cost = {dead / max(known, 1):.4f}")
        print(f"      of them in the {int(alive.sum())} environments whose puzzle is solvable from its initial state: "
              f"{int(alive_dead)} of {int(alive_known)} = {int(alive_dead) / max(int(alive_known), 1):.4f}")
        batch.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--seed", type=int, default=23)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--policy-steps", type=int, default=300)
    ap.add_argument("--only", default="1,2", help="the parts to run")
    args = ap.parse_args()
    print(f"# tools/bench_value_guide.py --envs {args.envs} --steps {args.steps} --seed {args.seed} --repeats {args.repeats} "
          f"--policy-steps {args.policy_steps}")
    print(f"# {torch.cuda.get_device_name(0)}; host clock around synchronised windows, one process, loops interleaved, round 0 dropped")
    pset, qp, ids = level0_set(args.envs)
    parts = args.only.split(",")
    if "1" in parts:
        step_loops(args, pset, qp, ids)
    if "2" in parts:
        policy_count(args, pset, qp, ids)


if __name__ == "__main__":
    main()

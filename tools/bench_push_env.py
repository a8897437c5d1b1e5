"""Measures stepping by pushes with the mask kept (pw_step_push_mask) and prints the figures kept in
profiles/push_env.txt.

    python tools/bench_push_env.py [--envs 65536] [--pushes 3] [--repeats 3] > profiles/push_env.txt

--envs live environments of the C3 set (the 68 Level-1 puzzles, environments grouped by puzzle) after --pushes drawn pushes from
the reset; every environment then draws one of its push rows uniformly.  On those states, in the same process, interleaved repeat
by repeat (the states and the views are put back before every timed call):
  (a) pw_step_push followed by pw_push_mask   the existing entry points, which this change does not touch: two floods
  (b) pw_step_push_mask with current views    the choice is looked up in the view; one flood, of the state that is left
  (c) pw_step_push_mask with every view invalidated   a flood of the state on entry, then (b)
and pw_walk_regions (no maps) on the same states, the cost of one full flood.  Then PushWorldPushVectorEnv loops -- valid choices
made from info["action_mask"] on the device (a uniform draw; the first push move), uint8 observations rendered every step -- in
pushes/s and primitive moves/s.

Timing: the host clock around synchronised calls, best of --repeats after one warm-up round, every repeat listed.
"""
import argparse
import glob
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pushworld_amd import _capi  # noqa: E402
from pushworld_amd.puzzle import PushWorldPuzzle  # noqa: E402
from pushworld_amd.search import PUSH_NONE, walk_regions  # noqa: E402
from pushworld_amd.vec_env import VecPushWorld  # noqa: E402
from pushworld_amd.vector_env import PushWorldPushVectorEnv  # noqa: E402

LEVEL1 = os.path.join(ROOT, "pushworld_amd", "data", "puzzles", "level1")


def ms(ts):
    return f"best {min(ts) * 1e3:.3f} ms (" + ", ".join(f"{t * 1e3:.3f}" for t in ts) + ")"


def draw_rows(vec, gen):
    """(push_from, push_action, WalkRegions, PushMoves): one uniformly drawn push row per environment, PUSH_NONE without one."""
    B, dev = vec.num_envs, vec.device
    reg = walk_regions(vec, vec.puzzle_id, vec.pos)
    rows = reg.pushes()
    count = reg.offset[1:] - reg.offset[:-1]
    u = torch.rand(B, generator=gen, dtype=torch.float64).to(dev)
    pick = (reg.offset[:-1] + (u * count).long().clamp(max=(count - 1).clamp(min=0))).clamp(max=max(rows.num_rows - 1, 0))
    has = count > 0
    frm = torch.where(has[:, None], rows.frm[pick], torch.zeros_like(rows.frm[pick])).contiguous()
    act = torch.where(has, rows.action[pick], torch.full_like(rows.action[pick], PUSH_NONE)).contiguous()
    return frm, act, reg, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--seed", type=int, default=23)
    ap.add_argument("--pushes", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--loop-envs", type=int, default=65536)
    ap.add_argument("--loop-steps", type=int, default=30)
    args = ap.parse_args()
    print(f"# tools/bench_push_env.py --envs {args.envs} --seed {args.seed} --pushes {args.pushes} --repeats {args.repeats} "
          f"--loop-envs {args.loop_envs} --loop-steps {args.loop_steps}")
    print(f"# {torch.cuda.get_device_name(0)}; host clock around synchronised calls, best of {args.repeats} after a warm-up")

    B = args.envs
    paths = sorted(glob.glob(os.path.join(LEVEL1, "*.pwp")))
    puzzles = [PushWorldPuzzle(p) for p in paths]
    ids = [i * len(paths) // B for i in range(B)]
    vec = VecPushWorld(puzzles, B, puzzle_ids=ids, observation=None, max_steps=None)
    vec.reset()
    gen = torch.Generator().manual_seed(args.seed)
    for _ in range(args.pushes):
        frm, act, _, _ = draw_rows(vec, gen)
        vec.step_push(frm, act)
    eng = vec.engine
    frm, act, reg, rows = draw_rows(vec, gen)
    vec.observe_pushes()  # the views of the states the timings start from
    state = (vec.pos, vec.steps, vec.terminated, vec.truncated)
    views = (vec.push_view_mask, vec.push_view_count, vec.push_walk_map, vec.push_region_size, vec._push_view_pos,
             vec._push_view_id)
    saved = [t.clone() for t in state + views]
    vec.step_push(frm, act)  # (allocates moves / status)

    def restore(invalidate=False):
        for dst, src in zip(state + views, saved):
            dst.copy_(src)
        if invalidate:
            vec._push_view_id.fill_(-1)

    mask = torch.empty_like(vec.push_view_mask)
    num = torch.empty_like(vec.push_view_count)

    def two_calls():
        eng.step_push(vec.puzzle_id, frm, act, vec.pos, vec.steps, vec.reward, vec.dgoals, vec.terminated, vec.truncated,
                      vec.push_moves_taken, vec.push_status, 0)
        eng.push_mask(vec.puzzle_id, vec.pos, None, mask, num)

    def one_call():
        eng.step_push_mask(vec.puzzle_id, frm, act, vec.pos, vec.steps, vec.reward, vec.dgoals, vec.terminated, vec.truncated,
                           vec.push_moves_taken, vec.push_status, *views, 0)

    def regions():
        eng.walk_regions(vec.puzzle_id, vec.pos, None, reg.region_size, reg.canon, reg.offset)

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    t_a, t_b, t_c, t_r = [], [], [], []
    for k in range(args.repeats + 1):  # interleaved: (a), (b), (c) and the flood in every round; round 0 is the warm-up
        restore()
        a = clock(two_calls)
        if k == 0:  # both paths leave the same states, masks and counts behind
            want = [t.clone() for t in state] + [mask.clone(), num.clone(), vec.push_moves_taken.clone(), vec.push_status.clone()]
        restore()
        b = clock(one_call)
        if k == 0:
            got = list(state) + [vec.push_view_mask, vec.push_view_count, vec.push_moves_taken, vec.push_status]
            assert all(torch.equal(x, y) for x, y in zip(got, want)), "pw_step_push_mask differs from pw_step_push + pw_push_mask"
        restore(invalidate=True)
        c = clock(one_call)
        restore()
        r = clock(regions)
        if k:
            t_a.append(a)
            t_b.append(b)
            t_c.append(c)
            t_r.append(r)
    restore()
    one_call()
    moves, status = vec.push_moves_taken.clone(), vec.push_status.clone()
    size = reg.region_size.double()
    print(f"C3 set, live states after {args.pushes} drawn pushes: {B} environments, N_pad {vec.num_objects_padded}, maps of "
          f"{mask.shape[1]} x {mask.shape[2]}; regions of {size.mean().item():.1f} positions on average (largest "
          f"{int(size.max().item())}), {rows.num_rows / B:.2f} push rows per state")
    print(f"  one drawn row per environment: {int((status == _capi.PUSH_DONE).sum())} pushed, "
          f"{int((status == _capi.PUSH_CUT).sum())} cut, {int((status == _capi.PUSH_REFUSED).sum())} refused; moves "
          f"{moves[moves > 0].double().mean().item():.2f} on average, {int(moves.max())} at the most")
    print(f"  (a) pw_step_push + pw_push_mask:            {ms(t_a)}")
    print(f"  (b) pw_step_push_mask, views current:       {ms(t_b)} = {B / min(t_b):.3e} pushes/s; (b) / (a) = "
          f"{min(t_b) / min(t_a):.2f}")
    print(f"  (c) pw_step_push_mask, views invalidated:   {ms(t_c)}; (c) / (a) = {min(t_c) / min(t_a):.2f}")
    print(f"  pw_walk_regions (no maps), one full flood:  {ms(t_r)}; (b) / flood = {min(t_b) / min(t_r):.2f}, (c) / flood = "
          f"{min(t_c) / min(t_r):.2f}")
    del vec

    # the facade, with the choice made on the device from info["action_mask"]
    E, T = args.loop_envs, args.loop_steps
    env = PushWorldPushVectorEnv(puzzles, E, max_steps=100, observation="uint8", seed=args.seed)
    _, info = env.reset()
    dgen = torch.Generator(device=env.vec.device).manual_seed(args.seed)

    def draw(am):
        flat = am.to(torch.float32)
        has = flat.sum(1, keepdim=True) > 0
        return torch.multinomial(torch.where(has, flat, torch.ones_like(flat)), 1, generator=dgen).squeeze(1)

    def first(am):
        return am.to(torch.uint8).argmax(1)

    print(f"PushWorldPushVectorEnv, {E} environments x {T} steps, uint8 observations, max_steps 100; the choice is made on the "
          f"device from info[\"action_mask\"], inside the timed loop:")
    for name, choose in (("a uniform draw over the push moves (torch.multinomial)", draw), ("the first push move (argmax)", first)):
        loops = []
        for k in range(args.repeats + 1):
            env.vec.counters_reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(T):
                _, _, _, _, info = env.step(choose(info["action_mask"]))
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            c = env.vec.counters()
            if k:
                loops.append((dt, c["env_steps"], c["episodes_ended"]))
        env.check_actions()
        dt, prim, ended = min(loops)
        print(f"  {name}: {ms([x[0] for x in loops])} per loop = {dt / T * 1e3:.3f} ms per step; {E * T / dt:.3e} pushes/s, "
              f"{prim / dt:.3e} primitive moves/s ({prim / (E * T):.2f} per push, resets included; {ended} episodes ended)")


if __name__ == "__main__":
    main()

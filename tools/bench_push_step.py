"""Measures stepping by pushes (pw_step_push / pw_push_mask) and prints the figures kept in
profiles/push_step.txt.

    python tools/bench_push_step.py [--envs 65536] [--repeats 3] > profiles/push_step.txt

--envs live environments of the C3 set (the 68 Level-1 puzzles, environments grouped by puzzle, 20 random steps from the reset);
every environment draws one of its push rows uniformly.  On those states, in the same run:
  pw_step_push     one macro step of every environment on its drawn row (the states are put back before every repeat)
  pw_walk_regions  the full flood of every region (no maps), what profiles/walk.txt records
  pw_push_mask     that flood with its push boards written out
  the loop         what a caller had to do before: pw_walk_regions with the walk maps and their copy to the host (timed), following
                   the paths there (not timed), then max(moves) single pw_step launches, each environment with its own length
                   (timed: the launches alone, with random actions)

Timing: the host clock around synchronised calls, best of --repeats after one warm-up run, every repeat listed.
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

LEVEL1 = os.path.join(ROOT, "pushworld_amd", "data", "puzzles", "level1")


def timed(fn, repeats, setup=None):
    """Seconds of every repeat of fn() between two synchronisations, after one warm-up; setup() runs before each, untimed."""
    out = []
    for k in range(repeats + 1):
        if setup:
            setup()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if k:
            out.append(time.perf_counter() - t0)
    return out


def ms(ts):
    return f"best {min(ts) * 1e3:.3f} ms (" + ", ".join(f"{t * 1e3:.3f}" for t in ts) + ")"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--seed", type=int, default=21)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    print(f"# tools/bench_push_step.py --envs {args.envs} --seed {args.seed} --repeats {args.repeats}")
    print(f"# {torch.cuda.get_device_name(0)}; host clock around synchronised calls, best of {args.repeats} after a warm-up")

    B = args.envs
    paths = sorted(glob.glob(os.path.join(LEVEL1, "*.pwp")))
    ids = [i * len(paths) // B for i in range(B)]
    vec = VecPushWorld([PushWorldPuzzle(p) for p in paths], B, puzzle_ids=ids, observation=None, max_steps=None)
    vec.reset()
    dev = vec.device
    gen = torch.Generator().manual_seed(args.seed)
    for _ in range(20):
        vec.step(torch.randint(0, 4, (B,), generator=gen, dtype=torch.uint8).to(dev))
    eng = vec.engine

    # one uniformly drawn push row per environment (PUSH_NONE where a state has none)
    reg = walk_regions(vec, vec.puzzle_id, vec.pos)
    rows = reg.pushes()
    count = reg.offset[1:] - reg.offset[:-1]
    u = torch.rand(B, generator=gen, dtype=torch.float64).to(dev)
    pick = (reg.offset[:-1] + (u * count).long().clamp(max=(count - 1).clamp(min=0))).clamp(max=max(rows.num_rows - 1, 0))
    has = count > 0
    frm = torch.where(has[:, None], rows.frm[pick], torch.zeros_like(rows.frm[pick])).contiguous()
    act = torch.where(has, rows.action[pick], torch.full_like(rows.action[pick], PUSH_NONE)).contiguous()
    saved = [t.clone() for t in (vec.pos, vec.steps, vec.terminated, vec.truncated)]

    def restore():
        for dst, src in zip((vec.pos, vec.steps, vec.terminated, vec.truncated), saved):
            dst.copy_(src)

    _, _, _, _, moves, status = vec.step_push(frm, act)
    moves, status = moves.clone(), status.clone()
    done = int((status == _capi.PUSH_DONE).sum())
    refused = int((status == _capi.PUSH_REFUSED).sum())
    cut = int((status == _capi.PUSH_CUT).sum())
    stepped = moves[moves > 0].double()
    longest = int(moves.max())
    size = reg.region_size.double()
    print(f"C3 set, live states after 20 random steps: {B} environments, N_pad {vec.num_objects_padded}; regions of "
          f"{size.mean().item():.1f} positions on average (largest {int(size.max().item())}), {rows.num_rows} push rows "
          f"({rows.num_rows / B:.2f} per state)")
    print(f"  one drawn row per environment: {done} pushed, {cut} cut, {refused} without a push move (refused); moves "
          f"{stepped.mean().item():.2f} on average, {longest} at the most")

    def step_push():
        eng.step_push(vec.puzzle_id, frm, act, vec.pos, vec.steps, vec.reward, vec.dgoals, vec.terminated, vec.truncated,
                      vec.push_moves_taken, vec.push_status, 0)

    def regions():
        eng.walk_regions(vec.puzzle_id, vec.pos, None, reg.region_size, reg.canon, reg.offset)

    mask = torch.empty((B, vec.pset.max_height, vec.pset.max_width), dtype=torch.uint8, device=dev)
    num = torch.empty((B,), dtype=torch.int32, device=dev)

    def push_mask():
        eng.push_mask(vec.puzzle_id, vec.pos, None, mask, num)

    actions = torch.randint(0, 4, (longest, B), generator=gen, dtype=torch.uint8).to(dev)

    def loop():
        for t in range(longest):
            vec.step(actions[t])

    maps = walk_regions(vec, vec.puzzle_id, vec.pos, maps=True)
    host_maps = torch.empty(maps.walk_map.shape, dtype=maps.walk_map.dtype, pin_memory=True)

    def maps_to_host():
        eng.walk_regions(vec.puzzle_id, vec.pos, None, maps.region_size, maps.canon, maps.offset, maps.walk_map)
        host_maps.copy_(maps.walk_map, non_blocking=True)

    t_s = timed(step_push, args.repeats, restore)
    restore()
    t_r = timed(regions, args.repeats)
    t_m = timed(push_mask, args.repeats)
    t_l = timed(loop, args.repeats, restore)
    print(f"  pw_step_push:              {ms(t_s)} = {B / min(t_s):.3e} macro steps/s, "
          f"{float(moves.sum()) / min(t_s):.3e} primitive steps/s")
    print(f"  pw_walk_regions (no maps): {ms(t_r)}; pw_step_push / pw_walk_regions = {min(t_s) / min(t_r):.2f}")
    print(f"  pw_push_mask ({mask.shape[1]} x {mask.shape[2]} bytes per state): {ms(t_m)}; pw_push_mask / pw_walk_regions = "
          f"{min(t_m) / min(t_r):.2f}")
    restore()
    t_h = timed(maps_to_host, args.repeats)
    print(f"  the loop of {longest} pw_step launches: {ms(t_l)} = {min(t_l) / longest * 1e6:.1f} us per launch")
    print(f"  pw_walk_regions with maps and their copy to the host ({maps.walk_map.numel() * 2 / 2**20:.0f} MiB), which the loop "
          f"needs first: {ms(t_h)}")
    print(f"  (maps to the host + the loop) / pw_step_push = {(min(t_h) + min(t_l)) / min(t_s):.2f}, the paths on the host not counted")


if __name__ == "__main__":
    main()

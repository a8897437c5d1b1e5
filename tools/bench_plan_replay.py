"""Measures plan replay (pw_plan_replay_check / pw_plan_replay_emit) on the 223 human solutions and on
that set tiled to 4 096 and 65 536 items, against the host loop it replaces (pw_plan_states + the is_valid_plan test, one
call per plan), and writes the figures to profiles/plan_replay.txt.

    python tools/bench_plan_replay.py [--out profiles/plan_replay.txt] [--repeats 20]

Timing: HIP events around each launch sequence on the current stream, after 3 warm-up runs; the median of --repeats runs.
"""
import argparse
import glob
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pushworld_amd import _capi  # noqa: E402
from pushworld_amd.puzzle import PushWorldPuzzle  # noqa: E402
from pushworld_amd.search import REPLAY_VALID, replay_plans  # noqa: E402
from pushworld_amd.vec_env import VecPushWorld  # noqa: E402

DATA = os.path.join(ROOT, "pushworld_amd", "data")
PEAK_BYTES_PER_S = 8e12


def human():
    out = []
    for k in (1, 2, 3, 4):
        for p in sorted(glob.glob(os.path.join(DATA, "puzzles", f"level{k}", "*.pwp"))):
            name = os.path.splitext(os.path.basename(p))[0]
            with open(os.path.join(DATA, "solutions", f"level{k}", name + ".yaml")) as f:
                plan = [ln.split(":", 1)[1].strip() for ln in f if ln.startswith("plan:")][0]
            out.append((p, ["LRUD".index(c) for c in plan]))
    return out


def timed(fn, repeats):
    """Median milliseconds of fn() between two events on the current stream."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plan_replay.txt"))
    ap.add_argument("--repeats", type=int, default=20)
    args = ap.parse_args()
    hs = human()
    paths, plans = [p for p, _ in hs], [pl for _, pl in hs]
    puzzles = [PushWorldPuzzle(p) for p in paths]
    vec = VecPushWorld(puzzles, len(paths), observation=None, max_steps=None)
    eng, dev, npad = vec.engine, vec.device, vec.num_objects_padded
    cap = 512
    base_plans = np.zeros((len(plans), cap), np.uint8)
    for i, p in enumerate(plans):
        base_plans[i, :len(p)] = p
    base_len = np.array([len(p) for p in plans], np.int32)
    lines = [f"plan replay, {torch.cuda.get_device_name(dev)}, N_pad {npad}, {len(plans)} human plans, "
             f"{int(base_len.sum())} actions (6 .. {int(base_len.max())} per plan); median (min) of {args.repeats} runs, HIP events"]

    # the host loop this replaces: one pw_plan_states call + the is_valid_plan test per plan
    def host_loop():
        ok = 0
        for i, p in enumerate(plans):
            _, goals = eng.plan_states(i, bytes(p))
            ok += bool(goals[-1] == 1 and not goals[:-1].any())
        return ok

    host_loop()
    host = []
    for _ in range(5):
        t0 = time.perf_counter()
        assert host_loop() == len(plans)
        host.append((time.perf_counter() - t0) * 1e3)
    host_ms = statistics.median(host)
    lines.append(f"host loop of pw_plan_states + is_valid_plan over the 223 plans: {host_ms:.2f} ms wall clock "
                 f"({host_ms / len(plans) * 1e3:.1f} us per plan; states only, no rows are kept)")

    row_bytes = 4 + 4 + 4 + 2 * npad + 1 + 8 + 1  # item, t, puzzle id, pos, action, reward, done
    for n in (len(plans), 4096, 65536):
        idx = np.arange(n) % len(plans)
        ids = torch.as_tensor(idx.astype(np.int32), device=dev)
        t_plans = torch.as_tensor(base_plans[idx], device=dev)
        t_len = torch.as_tensor(base_len[idx], device=dev)
        out = replay_plans(eng, ids, t_plans, t_len)
        T = out.num_rows
        assert T == int(base_len[idx].sum()) and bool((out.verdict == REPLAY_VALID).all())
        inc = _capi.REPLAY_INCLUDE_VALID

        def check():
            eng.plan_replay_check(ids, None, t_plans, t_len, None, inc, out.verdict, out.first_goal, out.final_pos, out.offset)

        def emit():
            eng.plan_replay_emit(ids, None, t_plans, t_len, None, inc, out.verdict, out.offset, T, out.item, out.t,
                                 out.puzzle_id, out.pos, out.action, out.reward, out.done)

        def both():
            check()
            emit()

        c_ms, c_min = timed(check, args.repeats)
        e_ms, e_min = timed(emit, args.repeats)
        b_ms, b_min = timed(both, args.repeats)
        t0 = time.perf_counter()
        replay_plans(eng, ids, t_plans, t_len)
        torch.cuda.synchronize()
        wall_ms = (time.perf_counter() - t0) * 1e3
        host_n = host_ms * n / len(plans)
        lines.append(f"n = {n:6d} items, {T:8d} rows: check {c_ms:.3f} ({c_min:.3f}) ms, emit {e_ms:.3f} ({e_min:.3f}) ms, "
                     f"check + emit {b_ms:.3f} ({b_min:.3f}) ms; replay_plans() wall clock incl. allocation and the one read-back "
                     f"{wall_ms:.2f} ms")
        lines.append(f"             host loop {'(measured)' if n == len(plans) else '(223-plan time scaled by n / 223)'} "
                     f"{host_n:.1f} ms -> ratio {host_n / b_ms:.0f}x against check + emit")
        lines.append(f"             emit: {T / (e_ms * 1e-3):.3e} rows/s, {row_bytes} bytes per row -> "
                     f"{T * row_bytes / (e_ms * 1e-3) / 1e9:.2f} GB/s written = "
                     f"{100 * T * row_bytes / (e_ms * 1e-3) / PEAK_BYTES_PER_S:.3f} % of the 8 TB/s peak")

    # the longest item alone: a replay is one dependent chain of steps, so this bounds every launch that holds it
    k = int(base_len.argmax())
    ids1 = torch.as_tensor(np.array([k], np.int32), device=dev)
    p1 = torch.as_tensor(base_plans[k:k + 1], device=dev)
    l1 = torch.as_tensor(base_len[k:k + 1], device=dev)
    o1 = replay_plans(eng, ids1, p1, l1)

    def emit1():
        eng.plan_replay_emit(ids1, None, p1, l1, None, 0, o1.verdict, o1.offset, o1.num_rows, o1.item, o1.t, o1.puzzle_id,
                             o1.pos, o1.action, o1.reward, o1.done)

    m1, m1min = timed(emit1, args.repeats)
    lines.append(f"longest item alone ({int(base_len[k])} actions, {os.path.basename(paths[k])}): emit {m1:.3f} ({m1min:.3f}) ms = "
                 f"{m1 * 1e3 / int(base_len[k]):.2f} us per step; the launch of the 223 plans cannot be shorter than this chain")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

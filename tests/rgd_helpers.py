"""What the RGD device tests share (tests/test_gpu_rgd.py, tests/test_gpu_rgd_deep.py): the restatement's call limit and the
helpers that encode states, read a shipped plan and compare the kernel with the restatement bit for bit."""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rgd_restatement as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_CALLS = 4000  # the restatement gives up past this many recursion frames (below the kernel's default budget, 4 096)


def enc(state):
    return [x * 10000 + y for x, y in state]


def dev(states, h):
    return torch.tensor([enc(s) for s in states], dtype=torch.int32, device=h.device)


def solution_plan(level, name):
    with open(os.path.join(ROOT, "pushworld_amd", "data", "solutions", level, name + ".yaml")) as f:
        for line in f:
            if line.startswith("plan:"):
                return ["LRUD".index(c) for c in line.split(":", 1)[1].strip()]
    raise ValueError(name)


def same(a, b):
    return (a == b) or (math.isnan(a) and math.isnan(b))


def compare(h_gpu, h_ref, states):
    """(compared, skipped): every state the restatement finishes must match bit for bit."""
    got = h_gpu.evaluate(dev(states, h_gpu)).cpu().numpy()
    compared = skipped = 0
    for s, g in zip(states, got):
        try:
            want = h_ref.estimate(s)
        except R.GiveUp:
            skipped += 1
            continue
        assert same(float(g), want), (s, float(g), want)
        compared += 1
    return compared, skipped

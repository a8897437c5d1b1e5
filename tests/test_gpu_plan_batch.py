"""Batched best-first search (pw_plan_batch_*, search.PlanBatch / solve_many) against the one-puzzle planner
(search.BestFirstSearch, itself held to the plain-Python restatement by test_gpu_planner.py): every item's info[0..7] and
plan must equal the planner's, in batches that mix puzzles of every level, sizes and outcomes; plus the time limit, the
bucket range, cancellation and the CLI."""
import glob
import os
import subprocess
import sys
import time

import pytest
import torch

from oracle import pw_oracle
from pushworld_amd.puzzle import PushWorldPuzzle
from pushworld_amd.search import BestFirstSearch, PlanBatch, RecursiveGraphDistance, action_groups, solve_many

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import planner_restatement as P  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_CPP = sorted(glob.glob(os.path.join(ROOT, "tests", "puzzles", "ref_cpp", "*.pwp")))
LEVEL = {k: sorted(glob.glob(os.path.join(ROOT, "pushworld_amd", "data", "puzzles", f"level{k}", "*.pwp"))) for k in (1, 2, 3, 4)}


def _mixed(per_level=4):
    """Puzzles of every level (different sizes and numbers of movables) and the C++ test puzzles, in one list."""
    out = list(REF_CPP)
    for k in (4, 2, 3, 1):
        out += LEVEL[k][:per_level]
    return out


def _single(path, mode, k, order, max_states, max_rounds, rgd_budget=None):
    bfs = BestFirstSearch(PushWorldPuzzle(path, order="cpp"), heuristic=mode, batch=k, max_states=max_states,
                          action_order=order, rgd_budget=rgd_budget)
    try:
        bfs.begin()
        info = bfs.run(max_rounds)
        return tuple(info), bfs.plan()
    finally:
        bfs.close()


def _batch(paths, mode, k, order, max_states, max_rounds=None, time_limit=None, rgd_budget=None, cost_range=None):
    pb = PlanBatch([PushWorldPuzzle(p, order="cpp") for p in paths], heuristic=mode, batch=k, max_states=max_states,
                   action_order=order, rgd_budget=rgd_budget, cost_range=cost_range)
    try:
        pb.run(max_rounds=max_rounds, time_limit=time_limit)
        return pb.results()
    finally:
        pb.close()


def _check_equal(paths, mode, k, order, max_states, max_rounds, rgd_budget=None):
    got = _batch(paths, mode, k, order, max_states, max_rounds, rgd_budget=rgd_budget)
    for path, (plan, info, seconds) in zip(paths, got):
        want_info, want_plan = _single(path, mode, k, order, max_states, max_rounds, rgd_budget)
        tag = (os.path.basename(path), mode, k, order, max_states, max_rounds)
        assert tuple(info) == want_info, tag
        assert plan == want_plan, tag
        assert seconds >= 0.0
    return got


@pytest.mark.parametrize("order", ["reference", "fixed"])
@pytest.mark.parametrize("mode", ["RGD", "N+RGD"])
@pytest.mark.parametrize("k", [1, 3, 64])
def test_mixed_batch_equals_planner_capped(k, mode, order):
    rounds = {1: 60, 3: 40, 64: 8}[k]
    _check_equal(_mixed(), mode, k, order, max_states=max(6000, 4 * k + 1), max_rounds=rounds)


@pytest.mark.parametrize("mode", ["RGD", "N+RGD"])
def test_level1_whole_searches_equal_planner(mode):
    # every Level-1 puzzle searched to its end at K = 1 (the reference's order) and at K = 8
    for k in (1, 8):
        got = _check_equal(LEVEL[1], mode, k, "reference", max_states=1 << 15, max_rounds=None)
        assert any(info.status == "solved" for _, info, _ in got), (mode, k)


def test_plans_are_valid_and_the_restatement_agrees():
    paths = REF_CPP + LEVEL[1][:8]
    got = _batch(paths, "N+RGD", 1, "reference", 20000, max_rounds=200)
    g = action_groups()
    for path, (plan, info, _) in zip(paths, got):
        with open(path) as f:
            oz = pw_oracle.OraclePuzzle(f.read(), "cpp")
        ref = P.PlannerRestatement(oz, "N+RGD", batch=1, max_states=20000, groups=g)
        ref.begin()
        want = ref.run(200)
        assert info.status == want["status"], path
        assert (info.rounds, info.expanded, info.visited, info.open) == \
            (want["rounds"], want["expanded"], want["visited"], want["open"]), path
        assert plan == ref.plan(), path
        if plan is not None:
            assert oz.is_valid_plan(plan, reject_early_goal=False), path


def test_limits_repeats_and_a_second_run():
    # a tiny store: every unsolved item ends with status limit, exactly where the planner does; an item listed twice gets
    # the same answer twice, and a second launch of the same handle (new closed-set tags) the same answers again
    paths = [LEVEL[1][5], LEVEL[2][0], LEVEL[1][5], REF_CPP[0]]
    for k in (1, 8):
        max_states = 4 * k + 41
        got = _check_equal(paths, "RGD", k, "reference", max_states=max_states, max_rounds=None)
        assert got[0][1] == got[2][1]
        assert any(info.status == "limit" for _, info, _ in got)
    pb = PlanBatch([PushWorldPuzzle(p, order="cpp") for p in paths], heuristic="N+RGD", batch=3, max_states=5000)
    try:
        pb.run(max_rounds=50)
        first = [(plan, tuple(info)) for plan, info, _ in pb.results()]
        pb.run(max_rounds=50)
        second = [(plan, tuple(info)) for plan, info, _ in pb.results()]
    finally:
        pb.close()
    assert first == second


def test_small_rgd_budget_equals_planner():
    _check_equal(LEVEL[1][:12], "N+RGD", 8, "reference", max_states=1 << 16, max_rounds=300, rgd_budget=1)


def test_time_limit():
    paths = LEVEL[4][:6] + LEVEL[1][:6]
    # a limit of a nanosecond: every item that is not solved at its start times out before its first round
    got = _batch(paths, "N+RGD", 1, "reference", 1 << 16, time_limit=1e-9)
    for plan, info, _ in got:
        assert info.status == "timeout" and info.rounds == 0 and plan is None
        assert info.open == 1 and info.stored == 1
    # a generous limit changes nothing
    capped = _batch(paths, "N+RGD", 4, "reference", 1 << 16, max_rounds=100, time_limit=600.0)
    free = _batch(paths, "N+RGD", 4, "reference", 1 << 16, max_rounds=100)
    assert [(p, tuple(i)) for p, i, _ in capped] == [(p, tuple(i)) for p, i, _ in free]
    # a limit in between: items stop by their own clock, each after some rounds
    t0 = time.perf_counter()
    mid = _batch(LEVEL[4], "N+RGD", 1, "reference", 1 << 20, time_limit=0.05)
    assert time.perf_counter() - t0 < 60
    for plan, info, seconds in mid:
        assert info.status in ("solved", "timeout", "exhausted", "limit")
        if info.status == "timeout":
            assert info.rounds > 0 and seconds >= 0.05


def test_cost_range():
    paths = LEVEL[1][:10]
    got = _batch(paths, "RGD", 1, "reference", 1 << 16, max_rounds=20, cost_range=4)
    full = _batch(paths, "RGD", 1, "reference", 1 << 16, max_rounds=20)
    for path, (plan, info, _), (_, want, _) in zip(paths, got, full):
        pz = PushWorldPuzzle(path, order="cpp")
        rgd = RecursiveGraphDistance(pz)
        start = torch.tensor([[x * 10000 + y for x, y in pz.initial_state]], dtype=torch.int32, device=rgd.device)
        c0 = float(rgd.evaluate(start)[0])
        rgd.close()
        if c0 == c0 and c0 != float("inf") and c0 >= 4:
            assert info.status == "range" and info.rounds == 0, path
        if info.status != "range":  # nothing reached the range: the same search
            assert tuple(info) == tuple(want), path


def test_cancel():
    pb = PlanBatch([PushWorldPuzzle(p, order="cpp") for p in LEVEL[4] * 2], heuristic="RGD", batch=1, max_states=1 << 22)
    try:
        t0 = time.perf_counter()
        pb.run(time_limit=30.0)
        time.sleep(0.2)
        pb.cancel()
        got = pb.results()
        elapsed = time.perf_counter() - t0
    finally:
        pb.close()
    assert elapsed < 10.0
    statuses = [info.status for _, info, _ in got]
    assert "running" in statuses and "timeout" not in statuses
    for plan, info, _ in got:
        assert (plan is not None) == (info.status == "solved")


def test_solve_many_and_the_cli(tmp_path):
    paths = LEVEL[1][:5]
    res = solve_many([PushWorldPuzzle(p, order="cpp") for p in paths], mode="N+RGD", max_states=1 << 18, time_limit=60.0)
    for path, (plan, info, _) in zip(paths, res):
        if plan is not None:
            assert PushWorldPuzzle(path).is_valid_plan(plan)
    pdir = tmp_path / "puzzles" / "sub"
    pdir.mkdir(parents=True)
    for p in paths + [os.path.join(ROOT, "tests", "puzzles", "ref_cpp", "no_solution.pwp")]:
        with open(p) as f:
            (pdir / os.path.basename(p)).write_text(f.read())
    out_dir = tmp_path / "results"
    out = subprocess.run([sys.executable, "-m", "pushworld_amd.benchmark_rgd", "--puzzles-path", str(tmp_path / "puzzles"),
                          "--results-path", str(out_dir), "--time-limit", "60", "--max-states", "262144"],
                         cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    files = sorted(os.listdir(out_dir / "sub"))
    assert files == sorted(os.path.splitext(os.path.basename(p))[0] + ".yaml" for p in os.listdir(pdir))
    text = (out_dir / "sub" / "no_solution.yaml").read_text()
    assert "failure_reason: no solution exists\n" in text and "plan: null\n" in text
    solved = 0
    for path, (plan, _, _) in zip(paths, res):
        text = (out_dir / "sub" / (os.path.splitext(os.path.basename(path))[0] + ".yaml")).read_text()
        assert "planner: Novelty+RGD\n" in text
        if plan is not None:
            solved += 1
            assert f"plan: {''.join('LRUD'[a] for a in plan)}\n" in text
    assert solved >= 1

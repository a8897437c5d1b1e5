"""Host side of the batched planner: the YAML writer of ``python -m pushworld_amd.benchmark_rgd`` (the reference's result
files without PyYAML), the result mapping of every planner status, the CLI's usage and the argument checks of
``pw_plan_batch_create``."""
import ctypes
import os
import subprocess
import sys

import pytest

from pushworld_amd import _capi
from pushworld_amd.benchmark_rgd import planning_result, yaml_dump, yaml_scalar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TRICKY = ["2 Obstacle", "A Perfect Fit", "LRUDDRUL", "", " lead", "trail ", "yes", "No", "null", "~", "123", "0x1F", "1.5",
          "1e5", ".inf", "- dash", "a: b", "a #b", "#hash", "it's", '"quoted"', "[x]", "{y}", "colon:", "50%", "@at", "ünï",
          "tab\tin", "2001-01-01", "Novelty+RGD", "time limit reached", "a,b", "x?", "-x", ":x", "a'b", "1_000", "+1",
          "1:30", "e5", "back\\slash"]


def test_yaml_literals():
    assert yaml_dump({"puzzle": "2 Obstacle", "plan": None, "planner": "RGD", "planning_time": 0.4,
                      "failure_reason": "time limit reached"}) == (
        "failure_reason: time limit reached\nplan: null\nplanner: RGD\nplanning_time: 0.4\npuzzle: 2 Obstacle\n")
    assert yaml_scalar(1800) == "1800"
    assert yaml_scalar(1e-05) == "1.0e-05"
    assert yaml_scalar(float("inf")) == ".inf"
    assert yaml_scalar("yes") == "'yes'"
    assert yaml_scalar("it's") == "it's"
    assert yaml_scalar("'q'") == "'''q'''"
    assert yaml_scalar("tab\tin") == '"tab\\tin"'
    assert yaml_scalar("LRUD") == "LRUD"


def test_yaml_reads_back():
    try:  # (PyYAML is optional: the files are written without it; where it is installed, it must read them back)
        import yaml
    except ImportError:
        yaml = None
    for s in TRICKY:
        m = {"puzzle": s, "plan": "LR", "planning_time": 0.125, "planner": "Novelty+RGD"}
        text = yaml_dump(m)
        if yaml is not None:
            assert yaml.safe_load(text) == m, s
            assert text == yaml.dump(m), s


def test_planning_results():
    r = planning_result("RGD", "p", "solved", "LRU", 0.5, 10.0)
    assert r == {"planner": "RGD", "puzzle": "p", "planning_time": 0.5, "plan": "LRU"}
    r = planning_result("RGD", "p", "solved", "LRU", 0.5, 10.0, valid=False)
    assert r["plan"] is None and r["failure_reason"] == "invalid plan"
    r = planning_result("RGD", "p", "timeout", None, 12.5, 10.0)
    assert r["plan"] is None and r["failure_reason"] == "time limit reached" and r["planning_time"] == 10.0
    assert planning_result("RGD", "p", "exhausted", None, 1.0, 10.0)["failure_reason"] == "no solution exists"
    assert planning_result("RGD", "p", "limit", None, 1.0, 10.0)["failure_reason"] == "memory error"
    assert planning_result("RGD", "p", "range", None, 1.0, 10.0)["failure_reason"] == "unknown"


def test_cli_usage():
    out = subprocess.run([sys.executable, "-m", "pushworld_amd.benchmark_rgd", "--help"], cwd=ROOT, capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    for opt in ("--results-path", "--puzzles-path", "--heuristic", "--time-limit", "--memory-limit", "--batch"):
        assert opt in out.stdout
    out = subprocess.run([sys.executable, "-m", "pushworld_amd.benchmark_rgd", "--heuristic", "BFS"], cwd=ROOT,
                         capture_output=True, text=True, timeout=120)
    assert out.returncode != 0


@pytest.mark.parametrize("mode, k, max_states, flags, cost_range, words", [
    (2, 1, 100, 0, 0, "mode"),
    (0, 0, 100, 0, 0, "batch"),
    (0, 65, 1000, 0, 0, "batch"),
    (0, 1, 100, 2, 0, "flags"),
    (0, 1, 100, 0, 65537, "cost_range"),
    (0, 1, 100, 0, -1, "cost_range"),
    (1, 8, 32, 0, 0, "max_states"),
    (1, 1, (1 << 28) + 1, 0, 0, "max_states"),
])
def test_create_argument_checks(mode, k, max_states, flags, cost_range, words):
    h = ctypes.c_void_p()
    rc = _capi.lib.pw_plan_batch_create(None, None, 1, mode, max_states, k, flags, 0, cost_range, ctypes.byref(h))
    assert rc == _capi.PW_EINVAL and not h.value
    assert words in _capi.last_error()
    assert _capi.lib.pw_plan_batch_cancel(None) == _capi.PW_EINVAL
    _capi.lib.pw_plan_batch_destroy(None)

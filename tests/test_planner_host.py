"""Best-first planner, host half: the restatement (tests/planner_restatement.py) against the literals of the reference's
C++ search test (cpp/test/search/test_best_first_search.cc), the reference action groups, and pw_planner_create's
argument checks (they fail before any device work)."""
import ctypes
import os
import sys

import pytest

from oracle import pw_oracle
from pushworld_amd import _capi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import planner_restatement as P  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_CPP = os.path.join(ROOT, "tests", "puzzles", "ref_cpp")


def _groups():
    buf = (ctypes.c_uint8 * 4000)()
    assert _capi.lib.pw_planner_action_groups(buf) == 1000
    return [tuple(buf[4 * g: 4 * g + 4]) for g in range(1000)]


def _load(name, order="cpp"):
    with open(os.path.join(REF_CPP, name)) as f:
        return pw_oracle.OraclePuzzle(f.read(), order)


def _manhattan(pz, sign=1):
    def h(state, moved):
        return float(sign * sum(abs(state[k + 1][0] - g[0]) + abs(state[k + 1][1] - g[1]) for k, g in enumerate(pz.goal_state)))
    return h


def test_action_groups():
    g = _groups()
    assert len(g) == 1000 and all(sorted(x) == [0, 1, 2, 3] for x in g)
    assert ["".join(map(str, x)) for x in g[:6]] == ["1230", "2103", "2031", "0231", "2103", "1320"]
    assert "".join(map(str, g[999])) == "0312"


@pytest.mark.parametrize("order", ["reference", "fixed"])
def test_restatement_matches_reference_search_test(order):
    groups = _groups() if order == "reference" else None
    pz = _load("easy_search.pwp")
    r = P.PlannerRestatement(pz, _manhattan(pz), groups=groups)
    r.begin()
    info = r.run()
    assert info["status"] == "solved" and len(r.plan()) == 3
    assert 9 <= info["visited"] <= 12 and info["open"] > 0
    assert pz.is_valid_plan(r.plan(), reject_early_goal=False)
    assert info["visited"] == (12 if order == "reference" else 10)

    r = P.PlannerRestatement(pz, _manhattan(pz, -1), groups=groups)
    r.begin()
    info = r.run()
    assert info["status"] == "solved" and info["visited"] > 100 and info["open"] > 0
    assert pz.is_valid_plan(r.plan(), reject_early_goal=False)

    pz = _load("no_solution.pwp")
    r = P.PlannerRestatement(pz, lambda s, m: 0.0, groups=groups)
    r.begin()
    info = r.run()
    assert info["status"] == "exhausted" and r.plan() is None and info["visited"] == 9 and info["open"] == 0

    pz = _load("trivial.pwp")
    r = P.PlannerRestatement(pz, lambda s, m: 0.0, groups=groups)
    r.begin()
    r.run()
    assert "".join("LRUD"[a] for a in r.plan()) == "RDRU"


@pytest.mark.parametrize("mode,k,max_states,words", [
    (2, 1, 100, "mode"), (-1, 1, 100, "mode"), (0, 0, 100, "batch"), (1, -3, 100, "batch"),
    (0, 4, 16, "max_states"), (1, 1, 4, "max_states"), (0, 1, 5, "null argument")])
def test_create_argument_checks(mode, k, max_states, words):
    # the argument checks need no engine: a NULL one is reported only once they pass
    h = ctypes.c_void_p()
    assert _capi.lib.pw_planner_create(None, 0, mode, max_states, k, 0, 0, ctypes.byref(h)) == _capi.PW_EINVAL
    assert words in _capi.last_error()
    assert not h.value

"""Host side of plan replay: the argument checks of ``pw_plan_replay_check`` / ``pw_plan_replay_emit`` that return before any
launch (all but the last need no engine or device memory), the verdict constants, and the shape / dtype / device checks of
``search.replay_plans``."""
import ctypes

import pytest
import torch

from pushworld_amd import _capi
from pushworld_amd.search import (REPLAY_CUT, REPLAY_EARLY, REPLAY_INCLUDE, REPLAY_NONE, REPLAY_NOT_GOAL, REPLAY_SKIPPED,
                                  REPLAY_VALID, REPLAY_VERDICT, PlanReplay, _replay_inputs, replay_plans)

# stand-ins for device pointers (and for the engine): every check below returns before anything is read through them
P = ctypes.c_void_p(4096)


def _check(e=P, ids=P, pos=None, npad=8, plans=P, plan_len=P, plan_cap=64, mask=None, n=4, include=0, verdict=P,
           first_goal=P, final_pos=None, offset=P):
    return _capi.lib.pw_plan_replay_check(e, ids, pos, npad, plans, plan_len, plan_cap, mask, n, include, verdict, first_goal,
                                          final_pos, offset, None)


def _emit(e=P, ids=P, pos=None, npad=8, plans=P, plan_len=P, plan_cap=64, mask=None, n=4, include=0, verdict=P, offset=P,
          cap=16):
    return _capi.lib.pw_plan_replay_emit(e, ids, pos, npad, plans, plan_len, plan_cap, mask, n, include, verdict, offset, cap,
                                         None, None, None, None, None, None, None, None, None, None)


CASES = [
    (dict(e=None), "null engine"),
    (dict(ids=None), "null puzzle_id"),
    (dict(plans=None), "null plans"),
    (dict(plan_len=None), "null plan_len"),
    (dict(verdict=None), "null verdict"),
    (dict(offset=None), "null offset"),
    (dict(n=0), "n must be"),
    (dict(n=-3), "n must be"),
    (dict(npad=0), "npad"),
    (dict(npad=12), "npad"),
    (dict(npad=64), "npad"),
    (dict(plan_cap=0), "plan_cap"),
    (dict(plan_cap=-1), "plan_cap"),
    (dict(plan_cap=65537), "plan_cap"),
    (dict(include=2), "include"),
    (dict(include=-1), "include"),
]


@pytest.mark.parametrize("kw, words", CASES)
def test_check_argument_checks(kw, words):
    assert _check(**kw) == _capi.PW_EINVAL
    msg = _capi.last_error()
    assert words in msg and "pw_plan_replay_check" in msg


@pytest.mark.parametrize("kw, words", CASES + [(dict(cap=-1), "cap must be")])
def test_emit_argument_checks(kw, words):
    assert _emit(**kw) == _capi.PW_EINVAL
    msg = _capi.last_error()
    assert words in msg and "pw_plan_replay_emit" in msg


def test_verdict_constants():
    assert (REPLAY_VALID, REPLAY_NOT_GOAL, REPLAY_EARLY, REPLAY_NONE, REPLAY_CUT, REPLAY_SKIPPED) == (1, 0, 2, -1, -2, -3)
    assert (_capi.REPLAY_VALID, _capi.REPLAY_NOT_GOAL, _capi.REPLAY_EARLY) == (1, 0, 2)
    assert (_capi.REPLAY_NONE, _capi.REPLAY_CUT, _capi.REPLAY_SKIPPED) == (-1, -2, -3)
    assert REPLAY_INCLUDE == {"valid": 0, "replayed": 1}
    assert (_capi.REPLAY_INCLUDE_VALID, _capi.REPLAY_INCLUDE_REPLAYED) == (0, 1)
    assert sorted(REPLAY_VERDICT.values()) == ["cut", "early", "none", "not_goal", "skipped", "valid"]
    assert _capi.PLAN_MAX_ACTIONS == 65536
    assert PlanReplay().verdict is None and PlanReplay().obs is None


def test_replay_plans_arguments():
    with pytest.raises(ValueError, match="engine_or_vec"):
        replay_plans(object(), None, None, None)
    with pytest.raises(ValueError, match="engine_or_vec"):
        replay_plans(None, None, None, None)


def test_replay_input_checks():
    cpu = torch.device("cpu")
    ids = torch.zeros(5, dtype=torch.int32)
    plans = torch.zeros((5, 16), dtype=torch.uint8)
    lens = torch.zeros(5, dtype=torch.int32)
    pos = torch.zeros((5, 8, 2), dtype=torch.int8)
    assert _replay_inputs(ids, plans, lens, None, None, 8, cpu) == 5
    assert _replay_inputs(ids, plans, lens, pos, torch.ones(5, dtype=torch.uint8), 8, cpu) == 5
    assert _replay_inputs(ids, plans, lens, pos, torch.ones(5, dtype=torch.bool), 8, cpu) == 5
    bad = [
        (ids.long(), plans, lens, pos, None, "puzzle_id"),
        (ids.view(5, 1), plans, lens, pos, None, "puzzle_id"),
        (torch.zeros(0, dtype=torch.int32), plans[:0], lens[:0], None, None, "items"),
        (ids, plans.to(torch.int8), lens, pos, None, "plans"),
        (ids, plans[:4], lens, pos, None, "plans"),
        (ids, plans.view(-1), lens, pos, None, "plans"),
        (ids, plans[:, :0], lens, pos, None, "plan_cap"),
        (ids, torch.zeros((5, 65537), dtype=torch.uint8), lens, pos, None, "plan_cap"),
        (ids, plans, lens.long(), pos, None, "plan_len"),
        (ids, plans, lens[:4], pos, None, "plan_len"),
        (ids, plans, lens, pos.to(torch.uint8), None, "pos"),
        (ids, plans, lens, pos[:, :4], None, "pos"),
        (ids, plans, lens, pos.view(5, 16), None, "pos"),
        (ids, plans, lens, pos, torch.ones(5, dtype=torch.int32), "mask"),
        (ids, plans, lens, pos, torch.ones(4, dtype=torch.uint8), "mask"),
        (ids, torch.zeros((16, 5), dtype=torch.uint8).t(), lens, pos, None, "contiguous"),
        (ids, plans, torch.zeros(10, dtype=torch.int32)[::2], pos, None, "contiguous"),
        (ids, plans, lens, pos.transpose(1, 2).contiguous().transpose(1, 2), None, "contiguous"),
    ]
    for a, b, c, d, m, words in bad:
        with pytest.raises(ValueError, match=words):
            _replay_inputs(a, b, c, d, m, 8, cpu)
    with pytest.raises(ValueError, match="live on"):
        _replay_inputs(ids, plans, lens, None, None, 8, torch.device("cuda", 0))

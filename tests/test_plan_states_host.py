"""Host side of planning from given states: the argument checks of ``pw_plan_batch_run_states`` that return before any
launch (no handle or device memory is needed for them), and the shape / dtype / device checks of ``StatePlanner.plan``."""
import ctypes

import pytest
import torch

from pushworld_amd import _capi
from pushworld_amd.search import PLAN_STATUS, StatePlanner, _state_inputs

# stand-ins for device pointers: every check below returns before anything is read through them
P = ctypes.c_void_p(4096)


def _run(b=None, ids=P, pos=P, npad=8, mask=None, n=4, info=P, plans=None, plan_len=None, plan_cap=0, time_limit=0.0):
    return _capi.lib.pw_plan_batch_run_states(b, ids, pos, npad, mask, n, 0, time_limit, info, plans, plan_len, plan_cap,
                                              None, None)


@pytest.mark.parametrize("kw, words", [
    (dict(n=0), "n must be"),
    (dict(n=-5), "n must be"),
    (dict(npad=0), "npad"),
    (dict(npad=12), "npad"),
    (dict(npad=64), "npad"),
    (dict(ids=None), "null argument"),
    (dict(pos=None), "null argument"),
    (dict(info=None), "null argument"),
    (dict(plans=P, plan_cap=16), "plan_len"),
    (dict(plans=P, plan_len=P, plan_cap=0), "plan_cap"),
    (dict(time_limit=-1.0), "time_limit"),
    (dict(time_limit=float("nan")), "time_limit"),
    (dict(), "null handle"),
])
def test_run_states_argument_checks(kw, words):
    assert _run(**kw) == _capi.PW_EINVAL
    assert words in _capi.last_error()


def test_skipped_status_name():
    assert PLAN_STATUS[6] == "skipped"


def test_state_planner_arguments():
    with pytest.raises(ValueError, match="heuristic"):
        StatePlanner(None, heuristic="BFS")
    with pytest.raises(ValueError, match="action_order"):
        StatePlanner(None, action_order="random")
    with pytest.raises(ValueError, match="source"):
        StatePlanner(object())


def test_plan_input_checks():
    cpu = torch.device("cpu")
    ids = torch.zeros(5, dtype=torch.int32)
    pos = torch.zeros((5, 8, 2), dtype=torch.int8)
    assert _state_inputs(ids, pos, None, 8, cpu) == 5
    assert _state_inputs(ids, pos, torch.ones(5, dtype=torch.uint8), 8, cpu) == 5
    assert _state_inputs(ids, pos, torch.ones(5, dtype=torch.bool), 8, cpu) == 5
    bad = [
        (ids.long(), pos, None, "puzzle_id"),
        (ids.view(5, 1), pos, None, "puzzle_id"),
        (torch.zeros(0, dtype=torch.int32), pos[:0], None, "items"),
        (ids, pos.to(torch.uint8), None, "pos"),
        (ids, pos[:, :4], None, "pos"),
        (ids, pos[:4], None, "pos"),
        (ids, pos.view(5, 16), None, "pos"),
        (ids, pos, torch.ones(5, dtype=torch.int32), "mask"),
        (ids, pos, torch.ones(4, dtype=torch.uint8), "mask"),
        (ids, pos.transpose(1, 2).contiguous().transpose(1, 2), None, "contiguous"),
        (torch.zeros(10, dtype=torch.int32)[::2], pos, None, "contiguous"),
    ]
    for a, b, m, words in bad:
        with pytest.raises(ValueError, match=words):
            _state_inputs(a, b, m, 8, cpu)
    with pytest.raises(ValueError, match="live on"):
        _state_inputs(ids, pos, None, 8, torch.device("cuda", 0))

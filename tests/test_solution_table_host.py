"""Host side of the cost-to-go tables: the argument checks of ``pw_search_solve`` / ``pw_search_table_read`` /
``pw_search_table_query`` that return before any launch (no search, no device memory), the shape / dtype / device /
contiguity checks of ``search.SolutionTable.query``, and the exported names."""
import ctypes

import pytest
import torch

import pushworld_amd
from pushworld_amd import _capi, search
from pushworld_amd.search import SolutionTable

# stand-ins for device pointers (and for the search): every check below returns before anything is read through them
P = ctypes.c_void_p(4096)
INFO = (ctypes.c_int64 * 4)()


def _query(s=P, ids=None, pos=P, npad=8, mask=None, n=4):
    return _capi.lib.pw_search_table_query(s, ids, pos, npad, mask, n, None, None, None, None)


@pytest.mark.parametrize("kw, words", [
    (dict(s=None), "null search"),
    (dict(n=0), "n must be"),
    (dict(n=-3), "n must be"),
    (dict(pos=None), "null pos"),
    (dict(npad=0), "npad"),
    (dict(npad=12), "npad"),
    (dict(npad=64), "npad"),
])
def test_query_argument_checks(kw, words):
    assert _query(**kw) == _capi.PW_EINVAL
    msg = _capi.last_error()
    assert words in msg and "pw_search_table_query" in msg


def test_solve_and_read_argument_checks():
    assert _capi.lib.pw_search_solve(None, INFO, None) == _capi.PW_EINVAL
    assert "pw_search_solve" in _capi.last_error() and "null search" in _capi.last_error()
    assert _capi.lib.pw_search_solve(P, None, None) == _capi.PW_EINVAL
    assert "pw_search_solve" in _capi.last_error() and "null info" in _capi.last_error()
    assert _capi.lib.pw_search_table_read(None, 0, 1, None, None, None, None) == _capi.PW_EINVAL
    assert "pw_search_table_read" in _capi.last_error() and "null search" in _capi.last_error()
    assert _capi.lib.pw_search_solve_stats(None, (ctypes.c_double * 5)()) == _capi.PW_EINVAL
    assert _capi.lib.pw_search_solve_stats(P, None) == _capi.PW_EINVAL
    assert "pw_search_solve_stats" in _capi.last_error()
    for first, count in ((-1, 1), (0, -1)):
        assert _capi.lib.pw_search_table_read(P, first, count, None, None, None, None) == _capi.PW_EINVAL
        assert "pw_search_table_read" in _capi.last_error() and "range" in _capi.last_error()


def _bare_table(npad=8):
    """A SolutionTable that never searched: ``query`` checks its inputs before it touches the library."""
    tab = SolutionTable.__new__(SolutionTable)
    tab.search, tab.npad, tab.device, tab.puzzle_index = None, npad, torch.device("cpu"), 0
    return tab


def test_query_input_checks():
    tab = _bare_table()
    ids = torch.zeros(5, dtype=torch.int32)
    pos = torch.zeros((5, 8, 2), dtype=torch.int8)
    bad = [
        (ids.long(), pos, None, "puzzle_id"),
        (ids.view(5, 1), pos, None, "puzzle_id"),
        (torch.zeros(0, dtype=torch.int32), pos[:0], None, "items"),
        (None, pos.view(5, 16), None, "pos"),
        (None, pos[:0], None, "pos"),
        (None, pos, torch.ones(4, dtype=torch.uint8), "mask"),
        (None, pos.transpose(1, 2).contiguous().transpose(1, 2), None, "contiguous"),
        (None, pos.to(torch.uint8), None, "pos"),
        (ids, pos.to(torch.uint8), None, "pos"),
        (ids, pos[:, :4], None, "pos"),
        (ids, pos[:4], None, "pos"),
        (ids, pos, torch.ones(5, dtype=torch.int32), "mask"),
        (ids, pos, torch.ones(4, dtype=torch.uint8), "mask"),
        (torch.zeros(10, dtype=torch.int32)[::2], pos, None, "contiguous"),
        (ids, pos.transpose(1, 2).contiguous().transpose(1, 2), None, "contiguous"),
    ]
    for a, b, m, words in bad:
        with pytest.raises(ValueError, match=words):
            tab.query(a, b, mask=m)
    tab.device = torch.device("cuda", 0)
    with pytest.raises(ValueError, match="live on"):
        tab.query(ids, pos)


def test_query_out_checks():
    tab = _bare_table()
    ids = torch.zeros(5, dtype=torch.int32)
    pos = torch.zeros((5, 8, 2), dtype=torch.int8)
    index, cost, acts = torch.zeros(5, dtype=torch.int32), torch.zeros(5, dtype=torch.int32), torch.zeros(5, dtype=torch.uint8)
    bad = [
        ((index, cost), "triple"),
        (index, "triple"),
        ((index.long(), cost, acts), "index"),
        ((index, cost[:4], acts), "cost"),
        ((index, cost, acts.to(torch.int8)), "acts"),
        ((index, torch.zeros(10, dtype=torch.int32)[::2], acts), "cost"),
        ((index, cost, None), "acts"),
    ]
    for out, words in bad:
        with pytest.raises(ValueError, match=words):
            tab.query(ids, pos, out=out)


def test_exported_names():
    from pushworld_amd.vec_env import VecPushWorld

    assert pushworld_amd.SolutionTable is search.SolutionTable
    assert "__all__" not in vars(pushworld_amd)  # (a star import must not pull in the built library)
    with pytest.raises(AttributeError):
        pushworld_amd.no_such_name
    assert (search.COST_DEAD_END, search.COST_UNKNOWN, search.TABLE_DEAD_END) == (-1, -2, 0xFFFF)
    for name in ("successors", "costs", "actions", "states", "plan", "optimal_plan", "query", "close"):
        assert callable(getattr(SolutionTable, name))
    assert callable(VecPushWorld.solution_table) and callable(VecPushWorld.cost_to_go)
    for name in ("pw_search_solve", "pw_search_solve_stats", "pw_search_table_read", "pw_search_table_query"):
        assert name in _capi.SIGNATURES and hasattr(_capi.lib, name)
    assert _capi.ABI_VERSION == 4

"""Host side of the batched cost-to-go tables: the argument checks of the ``pw_solve_batch_*`` entry points that return
before any launch (no handle is dereferenced further than its "no run yet" word, no device memory), the input checks of
``search.SolutionTableBatch.query``, and the exported names."""
import ctypes

import pytest
import torch

import pushworld_amd
from pushworld_amd import _capi, generate, search
from pushworld_amd.search import SolutionTableBatch

P = ctypes.c_void_p(4096)  # a stand-in for a device pointer: every check below returns before anything is read through it
lib = _capi.lib


def _einval(rc, *words):
    assert rc == _capi.PW_EINVAL
    msg = _capi.last_error()
    for w in words:
        assert w in msg, (w, msg)


def test_null_handle_is_refused_by_every_entry_point():
    out = ctypes.c_void_p()
    _einval(lib.pw_solve_batch_create(None, 16, ctypes.byref(out)), "pw_solve_batch_create", "null engine")
    _einval(lib.pw_solve_batch_create(P, 16, None), "pw_solve_batch_create", "null out")
    _einval(lib.pw_solve_batch_run(None, None, 4, 1 << 16, None), "pw_solve_batch_run", "null handle")
    _einval(lib.pw_solve_batch_results(None, None, None, None), "pw_solve_batch_results", "null handle")
    _einval(lib.pw_solve_batch_copy_results(None, None, None, None, None), "pw_solve_batch_copy_results", "null handle")
    _einval(lib.pw_solve_batch_totals(None, (ctypes.c_int64 * 3)(), None), "pw_solve_batch_totals", "null handle")
    _einval(lib.pw_solve_batch_read(None, 0, 0, 1, None, None, None, None, None), "pw_solve_batch_read", "null handle")
    _einval(lib.pw_solve_batch_query(None, P, P, 8, None, 4, None, None, None, None), "pw_solve_batch_query", "null handle")
    lib.pw_solve_batch_destroy(None)  # a no-op


def test_rows_cap_below_zero_is_refused_before_the_engine_is_touched():
    out = ctypes.c_void_p()
    _einval(lib.pw_solve_batch_create(P, -1, ctypes.byref(out)), "pw_solve_batch_create", "rows_cap")
    assert not out.value


class _Handle(ctypes.Structure):
    """The head of a PwSolveBatch that never ran: an engine pointer, the caps and the item counts -- all zero."""
    _fields_ = [("eng", ctypes.c_void_p), ("rows_cap", ctypes.c_int64), ("slots_cap", ctypes.c_int64),
                ("n_cap", ctypes.c_int32), ("n", ctypes.c_int32), ("rest", ctypes.c_uint8 * 512)]


@pytest.fixture()
def fresh():
    h = _Handle()
    return ctypes.cast(ctypes.pointer(h), ctypes.c_void_p), h


@pytest.mark.parametrize("kw, words", [
    (dict(n=0), "n must be"),
    (dict(n=-3), "n must be"),
    (dict(ids=None), "null puzzle_id"),
    (dict(pos=None), "null pos"),
    (dict(npad=0), "npad"),
    (dict(npad=12), "npad"),
    (dict(npad=64), "npad"),
    (dict(), "no run yet"),
])
def test_query_argument_checks(fresh, kw, words):
    args = dict(ids=P, pos=P, npad=8, n=4)
    args.update(kw)
    rc = lib.pw_solve_batch_query(fresh[0], args["ids"], args["pos"], args["npad"], None, args["n"], None, None, None, None)
    _einval(rc, "pw_solve_batch_query", words)


def test_run_and_read_argument_checks(fresh):
    h = fresh[0]
    for n in (0, -1):
        _einval(lib.pw_solve_batch_run(h, None, n, 1 << 16, None), "pw_solve_batch_run", "n must be")
    for cap in (0, -5, (1 << 28) + 1):
        _einval(lib.pw_solve_batch_run(h, None, 4, cap, None), "pw_solve_batch_run", "max_states_each")
    _einval(lib.pw_solve_batch_results(h, None, None, None), "pw_solve_batch_results", "no run yet")
    _einval(lib.pw_solve_batch_copy_results(h, None, None, None, None), "pw_solve_batch_copy_results", "no run yet")
    _einval(lib.pw_solve_batch_totals(h, None, None), "pw_solve_batch_totals", "null totals")
    _einval(lib.pw_solve_batch_totals(h, (ctypes.c_int64 * 3)(), None), "pw_solve_batch_totals", "no run yet")
    _einval(lib.pw_solve_batch_read(h, 0, 0, 1, None, None, None, None, None), "pw_solve_batch_read", "no run yet")


def _bare_batch(npad=8):
    """A SolutionTableBatch that never ran: ``query`` checks its inputs before it touches the library."""
    tab = SolutionTableBatch.__new__(SolutionTableBatch)
    tab.handle, tab.npad, tab.device = None, npad, torch.device("cpu")
    return tab


def test_query_input_checks():
    tab = _bare_batch()
    ids = torch.zeros(5, dtype=torch.int32)
    pos = torch.zeros((5, 8, 2), dtype=torch.int8)
    good = (torch.zeros(5, dtype=torch.int32), torch.zeros(5, dtype=torch.int32), torch.zeros(5, dtype=torch.uint8))
    bad = [
        (None, pos, None, None, "puzzle_id"),
        (ids.long(), pos, None, None, "puzzle_id"),
        (torch.zeros(0, dtype=torch.int32), pos[:0], None, None, "items"),
        (ids, pos.to(torch.uint8), None, None, "pos"),
        (ids, pos[:, :4], None, None, "pos"),
        (ids, pos, torch.ones(4, dtype=torch.uint8), None, "mask"),
        (ids, pos.transpose(1, 2).contiguous().transpose(1, 2), None, None, "contiguous"),
        (ids, pos, None, good[:2], "triple"),
        (ids, pos, None, (good[0].long(), good[1], good[2]), "index"),
        (ids, pos, None, (good[0], good[1][:4], good[2]), "cost"),
    ]
    for a, b, m, out, words in bad:
        with pytest.raises(ValueError, match=words):
            tab.query(a, b, mask=m, out=out)
    with pytest.raises(ValueError, match="source"):
        SolutionTableBatch(object())


def test_exported_names():
    from pushworld_amd.vec_env import VecPushWorld

    assert pushworld_amd.SolutionTableBatch is search.SolutionTableBatch
    assert pushworld_amd.SolutionTable is search.SolutionTable
    for name in ("keys", "states", "successors", "costs", "actions", "optimal_plan", "query", "close"):
        assert callable(getattr(SolutionTableBatch, name))
    assert callable(VecPushWorld.solution_tables) and callable(VecPushWorld.cost_to_go) and callable(generate.difficulty)
    assert (search.TABLE_BUILT, search.TABLE_TOO_MANY, search.TABLE_NOT_SEARCHED, search.TABLE_SUMMARY_ONLY,
            search.TABLE_COST_RANGE, search.TABLE_INTERNAL) == (0, 2, 3, 4, 5, 6)
    for name in ("pw_solve_batch_create", "pw_solve_batch_destroy", "pw_solve_batch_run", "pw_solve_batch_results",
                 "pw_solve_batch_copy_results", "pw_solve_batch_totals", "pw_solve_batch_read", "pw_solve_batch_query"):
        assert name in _capi.SIGNATURES and hasattr(_capi.lib, name)
    assert _capi.ABI_VERSION == 4

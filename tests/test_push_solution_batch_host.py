"""Host side of the batched cost-to-go tables over pushes: the header against ``_capi.SIGNATURES``, the include
order and ``build.HEADERS``, the argument checks of the ``pw_push_solve_batch_*`` entry points that return before any launch (no
handle is dereferenced further than its "no run yet" word, no device memory), the input checks of the Python wrappers, and the
key packing of tests/push_solution_batch_restatement.py on hand values."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import push_solution_batch_restatement as BR
from pushworld_amd import _capi, build, generate, search
from pushworld_amd.search import PushSolutionTableBatch
from pushworld_amd.vec_env import VecPushWorld

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p(4096)  # a stand-in for a device pointer: every check below returns before anything is read through it
lib = _capi.lib

NAMES = ("pw_push_solve_batch_create", "pw_push_solve_batch_destroy", "pw_push_solve_batch_run", "pw_push_solve_batch_results",
         "pw_push_solve_batch_copy_results", "pw_push_solve_batch_totals", "pw_push_solve_batch_read_states",
         "pw_push_solve_batch_read_rows", "pw_push_solve_batch_query")


def _einval(rc, *words):
    assert rc == _capi.PW_EINVAL
    msg = _capi.last_error()
    for w in words:
        assert w in msg, (w, msg)


def test_header_signatures_and_the_unit():
    with open(os.path.join(ROOT, "include", "pushworld_amd.h")) as f:
        src = f.read()
    assert _capi.lib.pw_abi_version() == 4 and _capi.ABI_VERSION == 4 and re.search(r"#define PW_ABI_VERSION 4\b", src)
    for name in NAMES:
        decl = re.search(r"\b(int|void) %s\((.*?)\);" % name, src, re.S)
        assert decl, name
        params = [p for p in re.sub(r"/\*.*?\*/", "", decl.group(2), flags=re.S).split(",") if p.strip()]
        restype, argtypes = _capi.SIGNATURES[name]
        assert restype is (ctypes.c_int if decl.group(1) == "int" else None) and len(argtypes) == len(params), name
        for p, t in zip(params, argtypes):
            if "**" in p:
                want = ctypes.POINTER(ctypes.c_void_p)
            elif "totals[" in p:
                want = ctypes.POINTER(ctypes.c_int64)
            elif "*" in p:
                want = ctypes.c_void_p
            else:
                want = ctypes.c_int64 if "int64_t" in p else ctypes.c_int32
            assert t is want, (name, p)
        assert hasattr(_capi.lib, name)
    with open(os.path.join(ROOT, "pushworld_amd", "csrc", "pw_kernels.hip")) as f:
        unit = f.read()
    mine = unit.index('#include "pw_push_solution_batch.inc"')
    assert unit.index('#include "pw_push_table.inc"') < mine and unit.index('#include "pw_solution_batch.inc"') < mine
    assert "pw_push_solution_batch.inc" in build.HEADERS
    with open(os.path.join(ROOT, "pushworld_amd", "csrc", "pw_push_solution_batch.inc")) as f:
        inc = f.read()
    code = "\n".join(line.split("//")[0] for line in inc.splitlines())  # (the comments may name what the code must not call)
    assert "pw_walk_kernel" not in code and "walk_launch" not in code and "lane_step<8>" in code
    assert "printf" not in code and "assert(" not in code


def test_null_handle_is_refused_by_every_entry_point():
    out = ctypes.c_void_p()
    _einval(lib.pw_push_solve_batch_create(None, 16, 16, ctypes.byref(out)), "pw_push_solve_batch_create", "null engine")
    _einval(lib.pw_push_solve_batch_create(P, 16, 16, None), "pw_push_solve_batch_create", "null out")
    _einval(lib.pw_push_solve_batch_run(None, None, None, 8, 4, 1 << 12, None), "pw_push_solve_batch_run", "null handle")
    _einval(lib.pw_push_solve_batch_results(None, None, None, None, None), "pw_push_solve_batch_results", "null handle")
    _einval(lib.pw_push_solve_batch_copy_results(None, None, None, None, None, None), "pw_push_solve_batch_copy_results",
            "null handle")
    _einval(lib.pw_push_solve_batch_totals(None, (ctypes.c_int64 * 4)(), None), "pw_push_solve_batch_totals", "null handle")
    _einval(lib.pw_push_solve_batch_read_states(None, 0, 0, 1, None, None, None, None, None), "pw_push_solve_batch_read_states",
            "null handle")
    _einval(lib.pw_push_solve_batch_read_rows(None, 0, 0, 1, None, None, None, None, None), "pw_push_solve_batch_read_rows",
            "null handle")
    _einval(lib.pw_push_solve_batch_query(None, P, P, 8, None, 4, None, None, None, None, None, None, None),
            "pw_push_solve_batch_query", "null handle")
    lib.pw_push_solve_batch_destroy(None)  # a no-op


@pytest.mark.parametrize("caps, words", [((-1, 0), "states_cap"), ((0, -1), "rows_cap"), ((-5, -5), "states_cap")])
def test_negative_caps_are_refused_before_the_engine_is_touched(caps, words):
    out = ctypes.c_void_p()
    _einval(lib.pw_push_solve_batch_create(P, caps[0], caps[1], ctypes.byref(out)), "pw_push_solve_batch_create", words)
    assert not out.value


class _Handle(ctypes.Structure):
    """The head of a PwPushSolveBatch that never ran: an engine pointer, the caps and the item counts -- all zero."""
    _fields_ = [("eng", ctypes.c_void_p), ("states_cap", ctypes.c_int64), ("rows_cap", ctypes.c_int64),
                ("slots_cap", ctypes.c_int64), ("n_cap", ctypes.c_int32), ("n", ctypes.c_int32), ("rest", ctypes.c_uint8 * 512)]


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
    rc = lib.pw_push_solve_batch_query(fresh[0], args["ids"], args["pos"], args["npad"], None, args["n"], None, None, None, None,
                                       None, None, None)
    _einval(rc, "pw_push_solve_batch_query", words)


def test_run_and_read_argument_checks(fresh):
    h = fresh[0]
    for n in (0, -1):
        _einval(lib.pw_push_solve_batch_run(h, None, None, 8, n, 1 << 12, None), "pw_push_solve_batch_run", "n must be")
    for cap in (0, -5, (1 << 26) + 1):
        _einval(lib.pw_push_solve_batch_run(h, None, None, 8, 4, cap, None), "pw_push_solve_batch_run", "max_states_each")
    for npad in (0, 12, 64):  # (only read with starts)
        _einval(lib.pw_push_solve_batch_run(h, None, P, npad, 4, 1 << 12, None), "pw_push_solve_batch_run", "npad")
    _einval(lib.pw_push_solve_batch_results(h, None, None, None, None), "pw_push_solve_batch_results", "no run yet")
    _einval(lib.pw_push_solve_batch_copy_results(h, None, None, None, None, None), "pw_push_solve_batch_copy_results", "no run yet")
    _einval(lib.pw_push_solve_batch_totals(h, None, None), "pw_push_solve_batch_totals", "null totals")
    _einval(lib.pw_push_solve_batch_totals(h, (ctypes.c_int64 * 4)(), None), "pw_push_solve_batch_totals", "no run yet")
    _einval(lib.pw_push_solve_batch_read_states(h, 0, 0, 1, None, None, None, None, None), "pw_push_solve_batch_read_states",
            "no run yet")
    _einval(lib.pw_push_solve_batch_read_rows(h, 0, 0, 1, None, None, None, None, None), "pw_push_solve_batch_read_rows",
            "no run yet")


def _bare_batch(npad=8):
    """A PushSolutionTableBatch that never ran: ``query`` checks its inputs before it touches the library."""
    tab = PushSolutionTableBatch.__new__(PushSolutionTableBatch)
    tab.handle, tab.npad, tab.device = None, npad, torch.device("cpu")
    return tab


def _engine(count=3):
    """An engine object without a device behind it: the wrapper's checks come before anything of the engine is used."""
    e = _capi.Engine.__new__(_capi.Engine)
    e.device, e.np, e.handle = torch.device("cpu"), 4, None
    e.pset = [None] * count
    return e


def test_wrapper_input_checks():
    tab = _bare_batch()
    ids = torch.zeros(5, dtype=torch.int32)
    pos = torch.zeros((5, 8, 2), dtype=torch.int8)
    good = search._push_query_outputs(None, 5, torch.device("cpu"))
    bad = [
        (None, pos, None, None, "puzzle_id"),
        (ids.long(), pos, None, None, "puzzle_id"),
        (torch.zeros(0, dtype=torch.int32), pos[:0], None, None, "items"),
        (ids, pos.to(torch.uint8), None, None, "pos"),
        (ids, pos[:, :4], None, None, "pos"),
        (ids, pos, torch.ones(4, dtype=torch.uint8), None, "mask"),
        (ids, pos.transpose(1, 2).contiguous().transpose(1, 2), None, None, "contiguous"),
        (ids, pos, None, tuple(good)[:5], "PushQuery of an earlier query"),
        (ids, pos, None, (good.index.long(),) + tuple(good)[1:], "index"),
        (ids, pos, None, tuple(good)[:1] + (good.cost[:4],) + tuple(good)[2:], "cost"),
    ]
    for a, b, m, out, words in bad:
        with pytest.raises(ValueError, match=words):
            tab.query(a, b, mask=m, out=out)
    with pytest.raises(ValueError, match="closed"):
        tab.query(ids, pos)
    with pytest.raises(ValueError, match="source"):
        PushSolutionTableBatch(object())
    e = _engine()
    for kw, words in [(dict(puzzles=[]), "must not be empty"), (dict(puzzles=[3]), "indices into the set"),
                      (dict(puzzles=[-1]), "indices into the set"), (dict(states=4), "both"), (dict(rows=4), "both"),
                      (dict(states=-1, rows=0), ">= 0"), (dict(states=0, rows=-1), ">= 0"), (dict(max_states_each=0), "max_states_each"),
                      (dict(puzzles=[0, 1], starts=[None]), "one entry")]:
        with pytest.raises(ValueError, match=words):
            PushSolutionTableBatch(e, **kw)


def test_entry_points_that_do_not_take_a_batch_yet():
    vec = VecPushWorld.__new__(VecPushWorld)  # the check comes before anything of the engine is used
    batch = _bare_batch()
    for call in (lambda: vec.reset_from_push_tables([batch]), lambda: vec.optimal_push_demonstrations([batch]),
                 lambda: vec.fewest_push_plans([batch])):
        with pytest.raises(ValueError, match="PushSolutionTableBatch is not supported here yet"):
            call()
    other = _bare_batch()
    other.engine, vec.engine = object(), object()
    with pytest.raises(ValueError, match="made on this environment"):
        vec.push_cost_to_go([other])
    assert callable(VecPushWorld.push_tables) and callable(generate.push_difficulty)
    for name in ("keys", "states", "offsets", "costs", "best", "rows", "query", "close", "__enter__", "__exit__"):
        assert callable(getattr(PushSolutionTableBatch, name))


def test_key_packing_by_hand():
    # movable j at bits 8 j: x in the low nibble, y in the high one; the agent's pair is canon, not where the state left it
    state = ((5, 7), (1, 2), (15, 0))
    assert BR.pack_key((3, 4), state) == 0x43 | (0x21 << 8) | (0x0F << 16)
    assert BR.pack_key((0, 0), ((9, 9),)) == 0 and BR.pack_key((15, 15), ((0, 0),)) == 0xFF
    eight = tuple((j, 15 - j) for j in range(8))
    want = sum(((j | ((15 - j) << 4)) << (8 * j)) for j in range(8))
    assert BR.pack_key(eight[0], eight) == want and want >> 63 == 1  # the top bit is in use: keys are unsigned
    assert search.pack_push_key((3, 4), state) == BR.pack_key((3, 4), state)
    with pytest.raises(ValueError):
        search.pack_push_key((16, 0), state)
    # the vectorised form, and the unpacking PushSolutionTableBatch.states does
    at = np.array([[(3, 4), (1, 2), (15, 0)], [(0, 0), (2, 1), (0, 15)]])
    keys = BR.keys_of(at)
    assert keys.dtype == np.uint64 and keys.tolist() == [BR.pack_key(s[0], s) for s in map(lambda a: tuple(map(tuple, a)), at.tolist())]
    shifts = (np.arange(3, dtype=np.uint64) * np.uint64(8))[None, :]
    byte = (keys[:, None] >> shifts) & np.uint64(0xFF)
    assert (np.stack([byte & np.uint64(15), byte >> np.uint64(4)], axis=-1).astype(np.int64) == at).all()

"""Host side of the batched best-first search over pushes: the header against ``_capi.SIGNATURES``, the include
order and ``build.HEADERS``, the argument checks of the ``pw_push_plan_batch_*`` entry points that return before any launch (no
handle is read further than its head, no device memory), the input checks of the Python wrappers on bare objects, and the names
on ``VecPushWorld``."""
import ctypes
import os
import re

import pytest
import torch

from pushworld_amd import _capi, build, search
from pushworld_amd.search import PushPlanBatch, PushPlanQuery, PushStatePlanner
from pushworld_amd.vec_env import VecPushWorld

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p(4096)  # a stand-in for a pointer: every check below returns before anything is read through it
lib = _capi.lib

NAMES = ("pw_push_plan_batch_create", "pw_push_plan_batch_run", "pw_push_plan_batch_run_states", "pw_push_plan_batch_read_states",
         "pw_push_plan_batch_read_links", "pw_push_plan_batch_cancel", "pw_push_plan_batch_destroy")


def _einval(rc, *words):
    assert rc == _capi.PW_EINVAL
    msg = _capi.last_error()
    for w in words:
        assert w in msg, (w, msg)


def test_header_signatures_and_the_unit():
    with open(os.path.join(ROOT, "include", "pushworld_amd.h")) as f:
        src = f.read()
    assert _capi.lib.pw_abi_version() == 4 and _capi.ABI_VERSION == 4 and re.search(r"#define PW_ABI_VERSION 4\b", src)
    assert re.search(r"#define PW_PUSH_PLAN_BATCH_INFO 11\b", src) and search.PUSH_PLAN_BATCH_INFO == 11
    assert re.search(r"#define PW_PUSH_NONE 0xFF\b", src) and search.PUSH_NONE == 0xFF
    for name in NAMES:
        decl = re.search(r"\b(int|void) %s\((.*?)\);" % name, src, re.S)
        assert decl, name
        params = [p for p in re.sub(r"/\*.*?\*/", "", decl.group(2), flags=re.S).split(",") if p.strip()]
        restype, argtypes = _capi.SIGNATURES[name]
        assert restype is (ctypes.c_int if decl.group(1) == "int" else None) and len(argtypes) == len(params), name
        for p, t in zip(params, argtypes):
            if "**" in p:
                want = ctypes.POINTER(ctypes.c_void_p)
            elif "*" in p:
                want = ctypes.c_void_p
            elif "double" in p:
                want = ctypes.c_double
            else:
                want = ctypes.c_int64 if "int64_t" in p else ctypes.c_int32
            assert t is want, (name, p)
        assert hasattr(_capi.lib, name)
    with open(os.path.join(ROOT, "pushworld_amd", "csrc", "pw_kernels.hip")) as f:
        unit = f.read()
    mine = unit.index('#include "pw_push_plan_batch.inc"')
    assert unit.index('#include "pw_plan_batch.inc"') < mine and unit.index('#include "pw_push_solution_batch.inc"') < mine
    assert "pw_push_plan_batch.inc" in build.HEADERS
    with open(os.path.join(ROOT, "pushworld_amd", "csrc", "pw_push_plan_batch.inc")) as f:
        inc = f.read()
    code = "\n".join(line.split("//")[0] for line in inc.splitlines())  # (the comments may name what the code must not call)
    # the flood and the queue are the existing ones, not copies; nothing of K15's flood launches
    for used in ("pw_psb_step(", "pw_psb_region_lanes<true", "pw_psb_region_lanes<false", "pw_psb_in_grid(", "pw_bs_pack(",
                 "pb_next_bucket(", "rgd_eval_pos("):
        assert used in code, used
    assert "pw_walk_kernel" not in code and "walk_launch" not in code and "lane_step" not in code
    assert "printf" not in code and "assert(" not in code


def test_create_argument_checks():
    out = ctypes.c_void_p()
    fn = "pw_push_plan_batch_create"
    _einval(lib.pw_push_plan_batch_create(None, None, 1, 1 << 12, 1, 0, 0, ctypes.byref(out)), fn, "null engine")
    _einval(lib.pw_push_plan_batch_create(P, None, 1, 1 << 12, 1, 0, 0, None), fn, "null out")
    for n in (0, -2):
        _einval(lib.pw_push_plan_batch_create(P, None, n, 1 << 12, 1, 0, 0, ctypes.byref(out)), fn, "n must be")
    for batch in (0, -1, 65):
        _einval(lib.pw_push_plan_batch_create(P, None, 1, 1 << 12, batch, 0, 0, ctypes.byref(out)), fn, "batch")
    for ms in (0, -1, (1 << 28) + 1):
        _einval(lib.pw_push_plan_batch_create(P, None, 1, ms, 1, 0, 0, ctypes.byref(out)), fn, "max_states")
    _einval(lib.pw_push_plan_batch_create(P, None, 1, 1 << 12, 1, -1, 0, ctypes.byref(out)), fn, "rgd_budget")
    for cr in (-1, 65537):
        _einval(lib.pw_push_plan_batch_create(P, None, 1, 1 << 12, 1, 0, cr, ctypes.byref(out)), fn, "cost_range")
    assert not out.value


class _Handle(ctypes.Structure):
    """The head of a PwPushPlanBatch that never ran: an engine pointer, the items, K and the largest number of movables."""
    _fields_ = [("eng", ctypes.c_void_p), ("n", ctypes.c_int32), ("K", ctypes.c_int32), ("max_n", ctypes.c_int32),
                ("rest", ctypes.c_uint8 * 2044)]


@pytest.fixture()
def fresh():
    h = _Handle()
    h.max_n = 5
    return ctypes.cast(ctypes.pointer(h), ctypes.c_void_p), h


RUN_BAD = [
    (dict(b=None), "null handle"),
    (dict(info=None), "null info"),
    (dict(limit=-1.0), "time_limit"),
    (dict(limit=float("nan")), "time_limit"),
    (dict(cap=-1), "push_cap"),
    (dict(plan_len=None, plan_from=P), "need plan_len"),
    (dict(plan_len=None, plan_action=P), "need plan_len"),
    (dict(plan_len=None, plan_pos=P), "need plan_len"),
    (dict(npad=0), "npad"),
    (dict(npad=12), "npad"),
    (dict(npad=64), "npad"),
    (dict(npad=4), "smaller than the largest prepared"),
]


@pytest.mark.parametrize("kw, words", RUN_BAD)
def test_run_argument_checks(fresh, kw, words):
    a = dict(b=fresh[0], limit=0.0, info=P, plan_len=P, plan_from=None, plan_action=None, plan_pos=None, cap=8, npad=8)
    a.update(kw)
    rc = lib.pw_push_plan_batch_run(a["b"], 0, a["limit"], a["info"], a["plan_len"], a["plan_from"], a["plan_action"], a["plan_pos"],
                                    a["cap"], a["npad"], None)
    _einval(rc, "pw_push_plan_batch_run", words)


@pytest.mark.parametrize("kw, words", RUN_BAD + [(dict(n=0), "n must be"), (dict(n=-4), "n must be"),
                                                 (dict(ids=None), "null puzzle_id"), (dict(pos=None), "null pos")])
def test_run_states_argument_checks(fresh, kw, words):
    a = dict(b=fresh[0], ids=P, pos=P, n=4, limit=0.0, info=P, plan_len=P, plan_from=None, plan_action=None, plan_pos=None, cap=8,
             npad=8)
    a.update(kw)
    rc = lib.pw_push_plan_batch_run_states(a["b"], a["ids"], a["pos"], a["npad"], None, a["n"], 0, a["limit"], a["info"],
                                           a["plan_len"], a["plan_from"], a["plan_action"], a["plan_pos"], a["cap"], None, None, None)
    _einval(rc, "pw_push_plan_batch_run_states", words)


def test_read_cancel_and_destroy_argument_checks(fresh):
    h = fresh[0]
    for fn, call in (("pw_push_plan_batch_read_states", lambda b, i, f, c: lib.pw_push_plan_batch_read_states(b, i, f, c, None, 8, None, None)),
                     ("pw_push_plan_batch_read_links", lambda b, i, f, c: lib.pw_push_plan_batch_read_links(b, i, f, c, None, None, None, None, None))):
        _einval(call(None, 0, 0, 1), fn, "null handle")
        _einval(call(h, -1, 0, 1), fn, "item")
        _einval(call(h, 0, -1, 1), fn, "range")
        _einval(call(h, 0, 0, -1), fn, "range")
        _einval(call(h, 0, 0, 1), fn, "no run yet")
    for npad in (0, 12, 64):
        _einval(lib.pw_push_plan_batch_read_states(h, 0, 0, 1, P, npad, None, None), "pw_push_plan_batch_read_states", "npad")
    _einval(lib.pw_push_plan_batch_cancel(None), "pw_push_plan_batch_cancel", "null handle")
    lib.pw_push_plan_batch_destroy(None)  # a no-op


def _engine(count=3):
    """An engine object without a device behind it: the wrappers' checks come before anything of the engine is used."""
    e = _capi.Engine.__new__(_capi.Engine)
    e.device, e.np, e.handle = torch.device("cpu"), 8, None
    e.pset = [None] * count
    return e


def test_wrapper_input_checks():
    for kw, words in [(dict(batch=0), "batch"), (dict(batch=65), "batch"), (dict(max_states=0), "max_states"),
                      (dict(max_states=(1 << 28) + 1), "max_states"), (dict(rgd_budget=0), "rgd_budget"),
                      (dict(cost_range=0), "cost_range"), (dict(cost_range=65537), "cost_range")]:
        with pytest.raises(ValueError, match=words):
            PushPlanBatch([object()], **kw)
        with pytest.raises(ValueError, match=words):
            PushStatePlanner(_engine(), **kw)
    with pytest.raises(ValueError, match="must not be empty"):
        PushPlanBatch([])
    with pytest.raises(ValueError, match="source"):
        PushStatePlanner(object())
    for puzzles, words in [([], "must not be empty"), ([3], "indices into the set"), ([-1], "indices into the set")]:
        with pytest.raises(ValueError, match=words):
            PushStatePlanner(_engine(), puzzles=puzzles)
    with pytest.raises(ValueError, match="must not be empty"):
        search.solve_many_pushes([])

    sp = PushStatePlanner.__new__(PushStatePlanner)  # a planner that is closed: plan checks its inputs before the library
    sp.handle, sp.npad, sp.device, sp._out = None, 8, torch.device("cpu"), None
    ids = torch.zeros(5, dtype=torch.int32)
    pos = torch.zeros((5, 8, 2), dtype=torch.int8)
    for a, b, kw, words in [
        (None, pos, {}, "puzzle_id"),
        (ids.long(), pos, {}, "puzzle_id"),
        (ids[:0], pos[:0], {}, "items"),
        (ids, pos.to(torch.uint8), {}, "pos"),
        (ids, pos[:, :4], {}, "pos"),
        (ids, pos, dict(mask=torch.ones(4, dtype=torch.uint8)), "mask"),
        (ids, pos.transpose(1, 2).contiguous().transpose(1, 2), {}, "contiguous"),
        (ids, pos, dict(max_rounds=0), "max_rounds"),
        (ids, pos, dict(time_limit=0.0), "time_limit"),
        (ids, pos, dict(push_cap=-1), "push_cap"),
        (ids, pos, {}, "closed"),
    ]:
        with pytest.raises(ValueError, match=words):
            sp.plan(a, b, **kw)
    for call in (sp.results, sp.primitive_plans, sp.validate, sp.info):
        with pytest.raises(RuntimeError, match="plan\\(\\) has not been called"):
            call()

    pb = PushPlanBatch.__new__(PushPlanBatch)
    pb.handle, pb.npad, pb.device, pb._out, pb.n = None, 8, torch.device("cpu"), None, 2
    for kw, words in [(dict(max_rounds=0), "max_rounds"), (dict(time_limit=-1.0), "time_limit"), (dict(push_cap=-1), "push_cap"),
                      ({}, "closed")]:
        with pytest.raises(ValueError, match=words):
            pb.run(**kw)
    for call in (pb.results, pb.primitive_plans, pb.validate):
        with pytest.raises(RuntimeError, match="run\\(\\) has not been called"):
            call()
    with pytest.raises(ValueError, match="item out of bounds"):
        pb.states(2)
    for closed in (pb, sp):  # cancel on a closed object says so, as run and plan do
        with pytest.raises(ValueError, match="closed"):
            closed.cancel()
    pb.close()
    sp.close()


def test_names_on_the_vector_environment():
    vec = VecPushWorld.__new__(VecPushWorld)  # the check comes before anything of the engine is used
    vec.engine = object()
    other = PushStatePlanner.__new__(PushStatePlanner)
    other.handle, other.engine = None, object()
    with pytest.raises(ValueError, match="made on this environment"):
        vec.planned_pushes(other)
    assert callable(VecPushWorld.push_planner) and callable(VecPushWorld.planned_pushes)
    assert callable(VecPushWorld.planner) and callable(VecPushWorld.expert_actions)  # (the move-by-move pair stays)
    assert PushPlanQuery._fields == ("push_from", "push_action", "pushes", "status")
    for cls, names in ((PushPlanBatch, ("run", "results", "primitive_plans", "validate", "states", "links", "cancel", "close",
                                        "__enter__", "__exit__")),
                       (PushStatePlanner, ("plan", "results", "primitive_plans", "validate", "info", "cancel", "close",
                                           "__enter__", "__exit__"))):
        for name in names:
            assert callable(getattr(cls, name)), (cls, name)
    assert callable(search.solve_many_pushes)
    assert search.PLAN_STATUS[search.PLAN_SKIPPED] == "skipped" and search.PUSH_PLAN_CUT == -2

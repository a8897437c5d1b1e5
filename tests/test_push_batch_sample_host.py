"""Host side of drawing from the batched cost-to-go tables over pushes (csrc/pw_push_batch_sample.inc): the
key-ordered cost index of tests/push_batch_sample_restatement.py against values worked out by hand, the header against
``_capi.SIGNATURES``, the argument checks that return before any launch (through the loaded library, stand-in pointers and the
head of a handle built by hand: no device), the wrappers' input checks and what ``VecPushWorld`` asks of a batch."""
import ctypes
import os
import re

import pytest
import torch

import push_batch_sample_restatement as XR
import push_table_restatement as TR
import push_table_sample_restatement as SR
from pushworld_amd import _capi, build
from pushworld_amd.search import PushPlans, PushSolutionTableBatch
from pushworld_amd.vec_env import VecPushWorld

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p(4096)  # a stand-in for a device pointer: every check below returns before anything is read through it
lib = _capi.lib
NAMES = ("pw_push_solve_batch_index", "pw_push_solve_batch_index_read", "pw_push_solve_batch_sample",
         "pw_push_solve_batch_plans", "pw_push_solve_batch_emit")


def _index(name):
    t = TR.case(name)[3]
    keys = XR.keys_of_table(t)
    return t, keys, XR.cost_index(t, keys)


# ---- hand values -----------------------------------------------------------------------------------------------------------------
def test_corridor_by_hand():
    """`corridor 7`: three states in a chain, costs 2, 1, 0 -- one state per bucket, so the order inside a bucket cannot matter."""
    t, keys, (sbc, cs) = _index("corridor 7")
    assert t.cost == [2, 1, 0] and sbc == [2, 1, 0] and cs == [0, 1, 2, 3, 3]
    assert (sbc, cs) == SR.cost_index(t)
    # the agent at canon (1, 1) in every state, the box one cell further each time: movable j at bits 8 j, x | y << 4
    assert [k & 0xFF for k in keys] == [0x11] * 3 and keys[0] < keys[1] < keys[2]
    assert [XR.canonical(t, i)[0] for i in range(3)] == [(1, 1)] * 3
    for env in range(4):
        assert XR.draw_state(7, env, 1, 0, 0, sbc, cs) == 2 and XR.draw_state(7, env, 1, 2, 9, sbc, cs) == 0


def test_overshoot_by_hand():
    """`serpentine 14x13 overshoot`: one goal state, one dead end, the start one push from the goal."""
    t, keys, (sbc, cs) = _index("serpentine 14x13 overshoot")
    goal, dead = t.cost.index(0), t.cost.index(-1)
    assert sbc == [goal, 0, dead] and cs == [0, 1, 2, 3]
    for env in range(6):  # the dead end is never in a band, however wide
        assert XR.draw_state(3, env, 1, 0, 1 << 30, sbc, cs) in (goal, 0)
        assert XR.draw_state(3, env, 1, 1, 1 << 30, sbc, cs) == 0


def test_all_dead_by_hand():
    """`shape (3, 12, 9) search start 3`: 261 states, all dead -- two words of cost_start, one bucket in ascending key."""
    t, keys, (sbc, cs) = _index("shape (3, 12, 9) search start 3")
    assert t.info[4] == -1 and cs == [0, 261] and sorted(sbc) == list(range(261))
    assert [keys[i] for i in sbc] == sorted(keys) and len(set(keys)) == 261
    assert sbc != list(range(261))  # (the store's order is the search's, not the keys')
    for lo, hi in ((0, 0), (1, 1 << 30), (-5, 50)):
        assert XR.draw_state(7, 0, 1, lo, hi, sbc, cs) is None


def test_empty_buckets():
    """A table whose store holds no state of cost 0 or 1 (every goal row leaves the grid, and so on): the buckets are empty, the
    words repeat, and a band over them alone draws nothing."""
    t = TR.case("corridor 7")[3]
    t = t._replace(cost=[2, 2, -1], info=t.info[:3] + (1, 2))
    keys = [30, 10, 20]
    sbc, cs = XR.cost_index(t, keys)
    assert sbc == [1, 0, 2] and cs == [0, 0, 0, 2, 3]
    assert XR.draw_state(7, 0, 1, 0, 1, sbc, cs) is None and XR.draw_state(7, 0, 1, 0, 2, sbc, cs) in (0, 1)
    assert {XR.draw_state(7, env, 1, 2, 2, sbc, cs) for env in range(32)} == {0, 1}
    # the same costs with the keys the other way round: the same buckets, the other order inside
    assert XR.cost_index(t, [10, 30, 20]) == ([0, 1, 2], cs)


def test_key_order_is_not_store_order_on_big():
    t, keys, (sbc, cs) = _index("big")
    by_store, cs_store = SR.cost_index(t)
    assert cs == cs_store and len(cs) == t.info[4] + 3 and cs[-1] == t.info[0] == 1260
    differ = 0
    for b in range(t.info[4] + 2):
        part = sbc[cs[b]:cs[b + 1]]
        assert sorted(part) == by_store[cs[b]:cs[b + 1]]  # the same states ...
        assert [keys[i] for i in part] == sorted(keys[i] for i in part)  # ... in ascending key
        assert all(t.cost[i] == (b if b <= t.info[4] else -1) for i in part)
        differ += part != by_store[cs[b]:cs[b + 1]]
    assert differ >= 1  # a test of the batch cannot pass by store order


@pytest.mark.parametrize("name", ["big", "corridor 7", "serpentine 14x14", "serpentine 14x13 overshoot",
                                  "shape (3, 12, 9) deep goal start", "shape (3, 12, 9) search start 3"])
def test_rows_start_from_the_canonical_state(name):
    """With ``pos`` NULL row 0 is the unpacked key: the agent at canon -- a cell of the stored state's own walk region, so the
    oracle's walk from there reaches every push of the node."""
    cp, t = TR.case(name)[1], TR.case(name)[3]
    for i in range(0, t.info[0], max(1, t.info[0] // 40)):
        steps = XR.plan(t, i, 1, 9, i)
        if not steps:
            continue
        got = XR.rows(cp, t, i, None, steps)
        assert got[0].pos == XR.canonical(t, i) and [r.cost for r in got] == list(range(len(steps), 0, -1))
        same = SR.rows(cp, t, i, None, steps)  # from the state as reached: the rows after the first are the same states
        assert [r.pos for r in got[1:]] == [r.pos for r in same[1:]]


# ---- the header ------------------------------------------------------------------------------------------------------------------
def test_header_signatures_and_the_unit():
    with open(os.path.join(ROOT, "include", "pushworld_amd.h")) as f:
        src = f.read()
    assert _capi.lib.pw_abi_version() == 4 and _capi.ABI_VERSION == 4 and re.search(r"#define PW_ABI_VERSION 4\b", src)
    for name in NAMES:
        decl = re.search(r"\bint %s\((.*?)\);" % name, src, re.S)
        assert decl, name
        params = [p for p in decl.group(1).split(",") if p.strip()]
        restype, argtypes = _capi.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == len(params), name
        for p, t in zip(params, argtypes):
            if "*" in p:
                want = ctypes.c_void_p
            elif "uint64_t" in p:
                want = ctypes.c_uint64
            else:
                want = ctypes.c_int64 if "int64_t" in p else ctypes.c_int32
            assert t is want, (name, p)
        assert hasattr(_capi.lib, name)
    # the three draws take the arguments of the one-puzzle table's
    for mine, theirs in (("sample", "sample"), ("plans", "plans"), ("emit", "emit")):
        assert _capi.SIGNATURES["pw_push_solve_batch_" + mine] == _capi.SIGNATURES["pw_push_search_table_" + theirs]
    for words in ("ASCENDING", "64-BIT KEY", "ENTIRELY untouched", "pw_push_solve_batch_index_read"):
        assert words in src, words
    with open(os.path.join(ROOT, "pushworld_amd", "csrc", "pw_kernels.hip")) as f:
        unit = f.read()
    mine = unit.index('#include "pw_push_batch_sample.inc"')
    draw = unit.index('#include "pw_push_draw.inc"')
    assert unit.index('#include "pw_push_solution_batch.inc"') < mine and unit.index('#include "pw_push_table_sample.inc"') < mine
    # the draws both push tables share: after the helpers and the scan of the move-level draws, before its two users
    assert unit.index('#include "pw_table_sample.inc"') < unit.index('#include "pw_push_table.inc"') < draw
    assert draw < unit.index('#include "pw_push_table_sample.inc"')
    # the one scan, sample, plans and emit are in the shared files; key and keep stay here, K20's key kernel there
    kernels = {"pw_table_sample.inc": 5, "pw_push_draw.inc": 3, "pw_push_table_sample.inc": 1, "pw_push_batch_sample.inc": 2}
    names = []
    for name, count in kernels.items():
        assert name in build.HEADERS
        with open(os.path.join(ROOT, "pushworld_amd", "csrc", name)) as f:
            inc = f.read()
        code = "\n".join(line.split("//")[0] for line in inc.splitlines())
        assert "printf" not in code and "assert(" not in code and "asm" not in code, name
        assert code.count("__global__") == count, name
        names += re.findall(r"__global__ __launch_bounds__\(256\) void (\w+)\(", code)
    assert sorted(names) == sorted([
        "pw_table_index_count_kernel", "pw_table_index_scan_kernel", "pw_table_index_scatter_kernel", "pw_table_sample_kernel",
        "pw_table_plans_kernel", "pw_push_sample_kernel", "pw_push_plans_kernel", "pw_push_emit_kernel",
        "pw_push_table_index_key_kernel", "pw_push_batch_index_key_kernel", "pw_push_batch_index_keep_kernel"])


# ---- the C ABI: checks that return before any launch -----------------------------------------------------------------------------
def _einval(rc, *words):
    assert rc == _capi.PW_EINVAL
    msg = _capi.last_error()
    for w in words:
        assert w in msg, (w, msg)


class _Handle(ctypes.Structure):
    """The head of a PwPushSolveBatch built by hand: no engine behind it, the caps, the item counts and the key pool's pointer;
    everything after it -- the index among it -- is zero."""
    _fields_ = [("eng", ctypes.c_void_p), ("states_cap", ctypes.c_int64), ("rows_cap", ctypes.c_int64),
                ("slots_cap", ctypes.c_int64), ("n_cap", ctypes.c_int32), ("n", ctypes.c_int32), ("d_key", ctypes.c_void_p),
                ("rest", ctypes.c_uint8 * 1024)]


def _handle(n=0, states=0, rows=0, key=None):
    h = _Handle()
    h.n, h.n_cap, h.states_cap, h.rows_cap, h.d_key = n, n, states, rows, key
    return ctypes.cast(ctypes.pointer(h), ctypes.c_void_p), h


RAN = dict(n=3, states=64, rows=64, key=4096)  # a handle that ran and has pools (and no index)


def _sample(b=None, ids=P, mask=None, n=4, npad=8, counter=P, lo=1, hi=3, lo_n=None, hi_n=None, pos=P, steps=P, state=P, cost=P,
            handle=RAN):
    keep = _handle(**handle)
    return lib.pw_push_solve_batch_sample(keep[0] if b is None else b[0], ids, mask, n, npad, 7, counter, lo, hi, lo_n, hi_n, pos,
                                          steps, None, None, state, cost, None)


def _plans(null=False, index=P, ids=P, n=4, tie=0, frm=P, action=P, state=P, plan_cap=16, plan_len=P, handle=RAN):
    keep = _handle(**handle)
    return lib.pw_push_solve_batch_plans(None if null else keep[0], index, ids, None, n, tie, 7, frm, action, state, plan_cap,
                                         plan_len, None)


def _emit(null=False, ids=P, n=4, npad=8, frm=P, action=P, state=P, plan_cap=16, plan_len=P, pos=None, offset=P, rows_cap=10, row=P,
          dropped=P, handle=RAN):
    keep = _handle(**handle)
    return lib.pw_push_solve_batch_emit(None if null else keep[0], ids, None, n, npad, frm, action, state, plan_cap, plan_len, pos,
                                        offset, rows_cap, row, P, P, P, P, P, P, dropped, None)


@pytest.mark.parametrize("kw, words", [
    (dict(b=(None,)), "null handle"),
    (dict(ids=None), "null puzzle_id"),
    (dict(n=0), "n must be"),
    (dict(n=-2), "n must be"),
    (dict(pos=None), "null pos"),
    (dict(steps=None), "null steps"),
    (dict(counter=None), "null counter"),
    (dict(state=None), "null out_state / out_cost"),
    (dict(cost=None), "null out_state / out_cost"),
    (dict(npad=0), "npad must be 4, 8, 16 or 32"),
    (dict(npad=12), "npad must be 4, 8, 16 or 32"),
    (dict(npad=64), "npad must be 4, 8, 16 or 32"),
    (dict(lo=4, hi=3), "lo <= hi"),
    (dict(lo=-1, hi=3), "0 <= lo"),
    (dict(lo_n=P), "come together"),
    (dict(hi_n=P), "come together"),
    (dict(handle=dict()), "no run yet"),
    (dict(handle=dict(n=3)), "nothing stored"),
    (dict(handle=dict(n=3, states=64, rows=64)), "nothing stored"),
    (dict(), "no index yet"),
])
def test_sample_argument_checks(kw, words):
    _einval(_sample(**kw), "pw_push_solve_batch_sample: ", words)


@pytest.mark.parametrize("kw, words", [
    (dict(null=True), "null handle"),
    (dict(n=0), "n must be"),
    (dict(index=None), "null index"),
    (dict(ids=None), "null puzzle_id"),
    (dict(frm=None), "null plan_from"),
    (dict(action=None), "plan_action"),
    (dict(plan_len=None), "plan_len"),
    (dict(plan_cap=0), "plan_cap"),
    (dict(plan_cap=-4), "plan_cap"),
    (dict(tie=2), "tie"),
    (dict(tie=-1), "tie"),
    (dict(handle=dict()), "no run yet"),
    (dict(handle=dict(n=3)), "nothing stored"),
])
def test_plans_argument_checks(kw, words):
    _einval(_plans(**kw), "pw_push_solve_batch_plans: ", words)


@pytest.mark.parametrize("kw, words", [
    (dict(null=True), "null handle"),
    (dict(n=0), "n must be"),
    (dict(ids=None), "null puzzle_id"),
    (dict(npad=5), "npad must be 4, 8, 16 or 32"),
    (dict(npad=64), "npad must be 4, 8, 16 or 32"),
    (dict(frm=None), "null plan_from"),
    (dict(action=None), "plan_action"),
    (dict(state=None), "plan_state"),
    (dict(plan_len=None), "plan_len"),
    (dict(plan_cap=0), "plan_cap"),
    (dict(offset=None), "null offset"),
    (dict(rows_cap=-1), "rows_cap"),
    (dict(row=None), "null row output"),
    (dict(dropped=None), "null dropped"),
    (dict(n=1 << 30, plan_cap=1 << 12), "beyond one launch"),
    (dict(handle=dict()), "no run yet"),
    (dict(handle=dict(n=3)), "nothing stored"),
])
def test_emit_argument_checks(kw, words):
    _einval(_emit(**kw), "pw_push_solve_batch_emit: ", words)


def test_index_argument_checks():
    _einval(lib.pw_push_solve_batch_index(None, None), "pw_push_solve_batch_index: ", "null handle")
    _einval(lib.pw_push_solve_batch_index_read(None, 0, P, P, None), "pw_push_solve_batch_index_read: ", "null handle")
    for kw, words in ((dict(), "no run yet"), (dict(n=3), "nothing stored")):
        keep = _handle(**kw)
        _einval(lib.pw_push_solve_batch_index(keep[0], None), "pw_push_solve_batch_index: ", words)
        _einval(lib.pw_push_solve_batch_index_read(keep[0], 0, P, P, None), "pw_push_solve_batch_index_read: ", words)
    keep = _handle(**RAN)
    _einval(lib.pw_push_solve_batch_index_read(keep[0], 0, P, P, None), "pw_push_solve_batch_index_read: ", "no index yet")


# ---- the wrappers ------------------------------------------------------------------------------------------------------------------
def _bare_batch(npad=8):
    """A PushSolutionTableBatch that never ran: every check comes before the library is touched ("closed" comes last)."""
    tab = PushSolutionTableBatch.__new__(PushSolutionTableBatch)
    tab.handle, tab.npad, tab.device = None, npad, torch.device("cpu")
    return tab


def test_python_input_checks():
    tab = _bare_batch()
    assert tab.indexed is False
    n = 5
    ids, pos = torch.zeros(n, dtype=torch.int32), torch.zeros((n, 8, 2), dtype=torch.int8)
    steps, flag = torch.zeros(n, dtype=torch.int32), torch.zeros(n, dtype=torch.uint8)
    ctr, i32 = torch.zeros(n, dtype=torch.int32), torch.zeros(n, dtype=torch.int32)
    for kw, words in [
        (dict(puzzle_id=None), "puzzle_id"),
        (dict(puzzle_id=ids.long()), "puzzle_id"),
        (dict(pos=pos[:, :4]), "pos"),
        (dict(steps=steps.long()), "steps"),
        (dict(terminated=flag.to(torch.int32)), "terminated"),
        (dict(mask=flag[:4]), "mask"),
        (dict(cost=3), "cost"),
        (dict(cost=(3, 1)), "lo <= hi"),
        (dict(cost=(i32, 4)), "cost: hi"),
        (dict(counter=ctr.long()), "counter"),
        (dict(out=(i32,)), "pair"),
        (dict(), "closed"),
    ]:
        args = dict(puzzle_id=ids, pos=pos, steps=steps, terminated=flag, truncated=flag, counter=ctr)
        args.update(kw)
        with pytest.raises(ValueError, match=words):
            tab.sample(**args)
    good = PushPlans(torch.zeros((n, 16, 2), dtype=torch.int8), torch.zeros((n, 16), dtype=torch.uint8),
                     torch.zeros((n, 16), dtype=torch.int32), i32)
    for kw, words in [
        (dict(index=ids.long()), "index"),
        (dict(index=ids[:0]), "items"),
        (dict(puzzle_id=None), "puzzle_id"),
        (dict(puzzle_id=ids[:4]), "puzzle_id"),
        (dict(mask=flag.to(torch.int32)), "mask"),
        (dict(tie="random"), "tie"),
        (dict(plan_cap=0), "plan_cap"),
        (dict(out=good[:3]), "PushPlans of an earlier call"),
        (dict(out=good._replace(state=good.state.long())), "out: state"),
        (dict(out=good), "closed"),
    ]:
        args = dict(index=ids, puzzle_id=ids, plan_cap=16)
        args.update(kw)
        with pytest.raises(ValueError, match=words):
            tab.plans(**args)
    for kw, words in [
        (dict(plans=good[:2]), "PushPlans of a plans call"),
        (dict(puzzle_id=None), "puzzle_id"),
        (dict(pos=pos[:, :4]), "pos"),
        (dict(mask=flag[:2]), "mask"),
        (dict(offset=torch.zeros(n, dtype=torch.int64)), "offset"),
        (dict(rows_cap=-1, offset=torch.zeros(n + 1, dtype=torch.int64)), "rows_cap"),
        (dict(rows_cap=3, offset=torch.zeros(n + 1, dtype=torch.int64)), "closed"),
    ]:
        args = dict(plans=good, pos=pos, puzzle_id=ids)
        args.update(kw)
        with pytest.raises(ValueError, match=words):
            tab.demonstration_rows(**args)
    for call in (tab.build_index, lambda: tab.cost_index(0)):
        with pytest.raises(ValueError, match="closed"):
            call()
    for name in ("build_index", "cost_index", "sample", "plans", "demonstration_rows", "covers"):
        assert callable(getattr(PushSolutionTableBatch, name))


def test_what_the_environment_asks_of_a_batch():
    vec = VecPushWorld.__new__(VecPushWorld)  # the checks come before anything of the engine is used
    vec.engine = object()
    calls = (vec.reset_from_push_tables, vec.optimal_push_demonstrations, vec.fewest_push_plans)
    # without an index: refused in the old words, whoever made it
    bare = _bare_batch()
    bare.engine = vec.engine
    for call in calls:
        with pytest.raises(ValueError, match="PushSolutionTableBatch is not supported here yet .*need a cost index on the batch"):
            call([bare])
    # indexed, of another engine
    other = _bare_batch()
    other.indexed, other.engine = True, object()
    for call in calls:
        with pytest.raises(ValueError, match=r"made on this environment \(VecPushWorld.push_tables\)"):
            call([other])
    # indexed and its own: the check passes (in a list with one that does not, the other is named)
    own = _bare_batch()
    own.indexed, own.engine = True, vec.engine
    assert vec._own_push_tables([own]) == [own] and vec._own_push_tables([]) == []
    with pytest.raises(ValueError, match="made on this environment"):
        vec._own_push_tables([own, other])
    with pytest.raises(ValueError, match="not supported here yet"):
        vec._own_push_tables([own, bare])

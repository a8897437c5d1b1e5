"""Host side of pushes unrolled into primitive actions: the restatement (tests/push_unroll_restatement.py)
against values worked out by hand on ``deep_puzzles.corridor(7)``, against the C oracle's step on every optimal row of the ten
table cases, the argument checks of ``pw_push_unroll_count`` / ``_write`` / ``_plans`` that return before any launch, the header
against ``_capi.SIGNATURES`` and the input checks of the Python wrappers."""
import ctypes
import os
import re

import pytest
import torch

import deep_puzzles
import push_step_restatement as SR
import push_table_restatement as TR
import push_unroll_restatement as UR
import walk_restatement as WR
from oracle import c_oracle
from pushworld_amd import _capi, build
from pushworld_amd.search import PUSH_NONE, PushRows, push_rows_to_plans, unroll_pushes
from pushworld_amd.vec_env import VecPushWorld

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# stand-ins for device pointers (and for the engine): every check below returns before anything is read through them
P = ctypes.c_void_p(4096)
L, R, U, D = 0, 1, 2, 3


def _corridor():
    """corridor(7) is `A . . . M0 . G0`; with its border the board is 9 x 3 and the agent starts at (1, 1)."""
    cp = c_oracle.COraclePuzzle(deep_puzzles.corridor(7))
    assert (cp.width, cp.height, cp.num_movables, cp.num_goals) == (9, 3, 2, 1)
    assert cp.initial_state == ((1, 1), (5, 1)) and tuple(cp.py.goal_state[0]) == (7, 1)
    return cp


def test_restatement_by_hand():
    cp = _corridor()
    s0 = cp.initial_state
    assert UR.unroll(cp, s0, (4, 1), R) == [R, R, R, R]  # three cells right to the cell left of M0, then the push
    s1 = ((5, 1), (6, 1))
    assert UR.unroll(cp, s1, (5, 1), R) == [R]           # dist 0: the push alone
    assert UR.unroll(cp, ((3, 1), (6, 1)), (5, 1), R) == [R, R, R]
    # the agent right of the box: it walks left to nothing, and pushes the box LEFT from its right-hand side
    s2 = ((7, 1), (5, 1))
    assert UR.unroll(cp, s2, (6, 1), L) == [L, L]
    seqs = [UR.unroll(cp, s0, (4, 1), R), None, UR.unroll(cp, s1, (5, 1), R), UR.unroll(cp, s2, (6, 1), L), None]
    assert UR.flatten(seqs) == ([4, -1, 1, 2, -1], [0, 4, 4, 5, 7, 7], [R, R, R, R, R, L, L])
    # plans: rows 0..0 refused by row 1; rows 2..3; no rows; a plan cut at plan_cap keeps its length
    assert UR.plans([0, 2, 4, 4, 5], seqs, 2) == ([[], [R, L], [], []], [-1, 3, 0, -1])
    assert UR.plans([0, 1], seqs, 3) == ([[R, R, R]], [4])


REFUSALS = [
    ("outside the grid", dict(frm=(9, 1))),
    ("negative position", dict(frm=(-1, 1))),
    ("outside the region", dict(frm=(6, 1))),     # behind the box
    ("a walk move", dict(frm=(3, 1))),
    ("a move that displaces nothing", dict(frm=(1, 1), action=L)),  # LEFT into the border
    ("action 4", dict(action=4)),
    ("PUSH_NONE", dict(action=PUSH_NONE)),
    ("a masked item", dict(masked=True)),
    ("puzzle id outside the set", dict(no_puzzle=True)),
    ("a movable outside its grid", dict(state=((1, 1), (9, 1)))),
]


@pytest.mark.parametrize("kind, kw", REFUSALS, ids=[k for k, _ in REFUSALS])
def test_restatement_refusals(kind, kw):
    cp = _corridor()
    state = kw.get("state", cp.initial_state)
    assert UR.unroll(None if kw.get("no_puzzle") else cp, state, kw.get("frm", (4, 1)), kw.get("action", R),
                     masked=kw.get("masked", False)) is None
    # pw_step_push's rule, unchanged (a mask is not part of it)
    if not kw.get("masked"):
        res = SR.macro_step(None if kw.get("no_puzzle") else cp, SR.Env(state, 0, 0, 0), kw.get("frm", (4, 1)), kw.get("action", R))
        assert res.status == SR.REFUSED


@pytest.mark.parametrize("name", list(TR.EXPECT))
def test_oracle_identity_on_optimal_rows(name):
    """Stepping the C oracle through L from a row's state ends in the macro step's state, with len(L) moves."""
    _, cp, _, t = TR.case(name)
    assert TR.summary(cp, t) == TR.EXPECT[name]
    rows = 0
    for i, state in enumerate(t.store.states):
        opt = [r for r in range(t.row_off[i], t.row_off[i + 1]) if t.flags[r] & TR.OPTIMAL]
        if not opt:
            continue
        reg = WR.region(cp, state)
        for r in opt:
            seq = UR.unroll(cp, state, t.frm[r], t.action[r], reg=reg)
            assert seq is not None and 1 <= len(seq) <= 4096
            s = tuple(tuple(xy) for xy in state)
            for k, a in enumerate(seq):
                s, moved = cp.get_next_state_moved(s, a)
                assert (list(moved) == [0]) == (k < len(seq) - 1)  # walk moves, then the one push move
            want = SR.macro_step(cp, SR.Env(state, 0, 0, 0), t.frm[r], t.action[r], reg=reg)
            assert want.status == SR.DONE and want.moves == len(seq) and tuple(map(tuple, s)) == want.state
            rows += 1
    assert (rows > 0) == (t.info[4] > 0)


def _count(e=P, ids=P, npad=8, frm=P, act=P, n=4, length=P, offset=P):
    return _capi.lib.pw_push_unroll_count(e, ids, None, npad, frm, act, None, n, length, offset, None)


def _write(e=P, ids=P, npad=8, frm=P, act=P, n=4, offset=P, cap=16, actions=P):
    return _capi.lib.pw_push_unroll_write(e, ids, None, npad, frm, act, None, n, offset, cap, actions, None, None)


def _plans(e=P, item_offset=P, length=P, offset=P, actions=P, rows=8, cap=16, m=4, plan_cap=32, plans=P, plan_len=P):
    return _capi.lib.pw_push_unroll_plans(e, item_offset, length, offset, actions, rows, cap, m, plan_cap, plans, plan_len, None)


COMMON = [
    (dict(e=None), "null engine"),
    (dict(ids=None), "null puzzle_id"),
    (dict(frm=None), "null push_from"),
    (dict(act=None), "null push_action"),
    (dict(offset=None), "null offset"),
    (dict(n=0), "n must be"),
    (dict(n=-3), "n must be"),
    (dict(npad=0), "npad"),
    (dict(npad=12), "npad"),
    (dict(npad=64), "npad"),
]


@pytest.mark.parametrize("kw, words", COMMON + [(dict(length=None), "null length")])
def test_count_argument_checks(kw, words):
    assert _count(**kw) == _capi.PW_EINVAL
    msg = _capi.last_error()
    assert words in msg and "pw_push_unroll_count" in msg


@pytest.mark.parametrize("kw, words", COMMON + [(dict(actions=None), "null actions"), (dict(cap=-1), "cap must be")])
def test_write_argument_checks(kw, words):
    assert _write(**kw) == _capi.PW_EINVAL
    msg = _capi.last_error()
    assert words in msg and "pw_push_unroll_write" in msg


@pytest.mark.parametrize("kw, words", [
    (dict(e=None), "null engine"),
    (dict(item_offset=None), "null item_offset"),
    (dict(length=None), "null length"),
    (dict(offset=None), "null offset"),
    (dict(actions=None), "null actions"),
    (dict(plans=None), "null plans"),
    (dict(plan_len=None), "null plan_len"),
    (dict(m=0), "m must be"),
    (dict(m=-1), "m must be"),
    (dict(rows=-1), "rows must be"),
    (dict(cap=-1), "cap must be"),
    (dict(plan_cap=0), "plan_cap"),
    (dict(plan_cap=65537), "plan_cap"),
])
def test_plans_argument_checks(kw, words):
    assert _plans(**kw) == _capi.PW_EINVAL
    msg = _capi.last_error()
    assert words in msg and "pw_push_unroll_plans" in msg


def test_header_signatures_and_the_unit():
    with open(os.path.join(ROOT, "include", "pushworld_amd.h")) as f:
        src = f.read()
    assert _capi.lib.pw_abi_version() == 4 and re.search(r"#define PW_ABI_VERSION 4\b", src)
    for name in ("pw_push_unroll_count", "pw_push_unroll_write", "pw_push_unroll_plans"):
        decl = re.search(r"\bint %s\((.*?)\);" % name, src, re.S)
        assert decl, name
        params = [p for p in re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",") if p.strip()]
        restype, argtypes = _capi.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == len(params), name
        for p, t in zip(params, argtypes):
            want = ctypes.c_void_p if "*" in p else (ctypes.c_int64 if "int64_t" in p else ctypes.c_int32)
            assert t is want, (name, p)
        assert hasattr(_capi.lib, name)
    with open(os.path.join(ROOT, "pushworld_amd", "csrc", "pw_kernels.hip")) as f:
        unit = f.read()
    assert unit.index('#include "pw_push_step.inc"') < unit.index('#include "pw_push_unroll.inc"')
    assert "pw_push_unroll.inc" in build.HEADERS


def _engine():
    """An engine object without a device behind it: the wrappers' checks come before anything of the engine is used."""
    e = _capi.Engine.__new__(_capi.Engine)
    e.device, e.np = torch.device("cpu"), 4
    return e


def test_wrapper_input_checks():
    ids = torch.zeros(3, dtype=torch.int32)
    frm, act = torch.zeros((3, 2), dtype=torch.int8), torch.zeros(3, dtype=torch.uint8)
    for bad in (object(), None):
        with pytest.raises(ValueError, match="engine_or_vec"):
            unroll_pushes(bad, ids, frm, act)
        with pytest.raises(ValueError, match="engine_or_vec"):
            push_rows_to_plans(bad, ids, None, None)
    e = _engine()
    bad = [
        (dict(puzzle_id=ids.to(torch.int64)), "puzzle_id"),
        (dict(puzzle_id=torch.zeros(0, dtype=torch.int32)), "puzzle_id"),
        (dict(push_from=frm.to(torch.uint8)), "push_from"),
        (dict(push_from=torch.zeros((3, 3), dtype=torch.int8)), "push_from"),
        (dict(push_from=torch.zeros((2, 3), dtype=torch.int8).t()), "push_from"),
        (dict(push_action=act.to(torch.int8)), "push_action"),
        (dict(push_action=torch.zeros(4, dtype=torch.uint8)), "push_action"),
        (dict(push_action=torch.zeros(6, dtype=torch.uint8)[::2]), "push_action"),
        (dict(pos=torch.zeros((3, 8, 2), dtype=torch.int8)), "pos"),
        (dict(mask=torch.zeros(3, dtype=torch.int32)), "mask"),
    ]
    for kw, words in bad:
        args = dict(puzzle_id=ids, push_from=frm, push_action=act)
        args.update(kw)
        with pytest.raises(ValueError, match=words):
            unroll_pushes(e, **args)
    rows = PushRows(torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.int32),
                    torch.zeros((0, 2), dtype=torch.int8), torch.zeros(0, dtype=torch.uint8), torch.zeros(0, dtype=torch.int32),
                    torch.zeros((0, 4, 2), dtype=torch.int8), torch.zeros(1, dtype=torch.int32), 0)
    none = torch.zeros(0, dtype=torch.int32)
    off = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(ValueError, match="rows"):
        push_rows_to_plans(e, none, (1, 2), off)
    with pytest.raises(ValueError, match="plan_cap"):
        push_rows_to_plans(e, none, rows, off, plan_cap=0)
    with pytest.raises(ValueError, match="plan_cap"):
        push_rows_to_plans(e, none, rows, off, plan_cap=65537)
    with pytest.raises(ValueError, match="item_offset"):
        push_rows_to_plans(e, none, rows, off.to(torch.int32))
    with pytest.raises(ValueError, match="item_offset"):
        push_rows_to_plans(e, none, rows, torch.zeros(1, dtype=torch.int64))
    with pytest.raises(ValueError, match="puzzle_id_rows"):
        push_rows_to_plans(e, ids, rows, off)
    # plans without rows: every plan is empty, nothing is launched
    plans, plan_len, pushes = push_rows_to_plans(e, none, rows, off, plan_cap=5)
    assert plans.shape == (3, 5) and plans.dtype == torch.uint8 and plan_len.tolist() == [0, 0, 0] and pushes.tolist() == [0, 0, 0]
    assert plan_len.dtype == torch.int32 and pushes.dtype == torch.int32


def test_fewest_push_plans_input_checks():
    vec = VecPushWorld.__new__(VecPushWorld)  # the checks come before anything of the engine is used
    for kw, words in [(dict(tie="first"), "tie"), (dict(plan_cap=0), "plan_cap"), (dict(plan_cap=65537), "plan_cap"),
                      (dict(push_cap=0), "push_cap")]:
        with pytest.raises(ValueError, match=words):
            vec.fewest_push_plans([], **kw)

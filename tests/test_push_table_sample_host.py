"""Host side of drawing from the cost-to-go tables over pushes (csrc/pw_push_table_sample.inc): the restatement
of tests/push_table_sample_restatement.py against values worked out by hand, the identity the emit kernel relies on -- asserted
from the C oracle's step on every optimal row of all ten cases of ``push_table_restatement.EXPECT`` --, the argument checks
that return before anything touches a device, the header against ``_capi.SIGNATURES`` and the wrappers' input checks."""
import ctypes
import os

import pytest
import torch

import push_table_restatement as TR
import push_table_sample_restatement as SR
import walk_restatement as WR
from pushworld_amd import _capi, search
from pushworld_amd.search import PushPlans, PushRows, PushSolutionTable, decode_push_choice, encode_push_choice
from table_sample_restatement import K_PLAN, K_SAMPLE, hash64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p(4096)  # a stand-in for a handle or a device array: every check below returns before anything is read through it
lib = _capi.lib
NAMES = {"index": 2, "index_read": 4, "sample": 18, "plans": 13, "emit": 22}  # entry point -> number of arguments
D = WR.DISPLACEMENTS


def _mix_by_hand(seed, a, b):
    """pw_mix64 in plain Python integers: the splitmix64 finaliser over seed + c1 (a + 1) + c2 b."""
    m = (1 << 64) - 1
    z = (seed + 0x9E3779B97F4A7C15 * (a + 1) + 0xD1B54A32D192ED03 * b) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


# ---- hand values ------------------------------------------------------------------------------------------------------------------
def test_corridor_by_hand():
    """`corridor 7`: three states in a chain, costs 2, 1, 0 -- one state per bucket and no dead end."""
    _, cp, _, t = TR.case("corridor 7")
    assert t.cost == [2, 1, 0] and t.info[4] == 2
    sbc, cs = SR.cost_index(t)
    assert sbc == [2, 1, 0] and cs == [0, 1, 2, 3, 3]
    # one state per cost: whatever the hash, a band of one cost draws that state
    for env in range(4):
        assert SR.draw_state(7, env, 1, 0, 0, sbc, cs) == 2
        assert SR.draw_state(7, env, 1, 1, 1, sbc, cs) == 1
        assert SR.draw_state(7, env, 1, 2, 9, sbc, cs) == 0 == SR.draw_state(7, env, 1, 40, 50, sbc, cs)
    # the band 1 .. 2 holds states_by_cost[1 : 3] = 1, 0: u = floor(r * 2 / 2^64) is the top bit of the hash
    for env, counter in ((0, 1), (0, 2), (1, 1), (2, 1), (3, 5)):
        r = _mix_by_hand(7 ^ K_SAMPLE, env, counter)
        assert r == hash64(7 ^ K_SAMPLE, env, counter)
        assert SR.draw_state(7, env, counter, 1, 1 << 30, sbc, cs) == (1, 0)[r >> 63]
    assert _mix_by_hand(7 ^ K_SAMPLE, 0, 1) == 0x717A53E9E02ECF93  # top bit 0: environment 0 draws state 1 first
    assert SR.draw_state(7, 0, 1, 1, 2, sbc, cs) == 1
    # the plans: one row per state, both tie rules the same; the emitted states from the oracle
    p0 = SR.plan(t, 0, 0, 7, 0)
    assert [s.node for s in p0] == [0, 1] and p0 == SR.plan(t, 0, 1, 7, 3)
    assert [(s.frm, s.action) for s in p0] == [(t.frm[0], t.action[0]), (t.frm[1], t.action[1])]
    assert SR.plan(t, 2, 0, 7, 0) == [] and SR.plan(t, 3, 0, 7, 0) is None and SR.plan(t, -1, 0, 7, 0) is None
    rows = SR.rows(cp, t, 5, None, p0)
    assert [(r.item, r.t, r.node, r.cost) for r in rows] == [(5, 0, 0, 2), (5, 1, 1, 1)]
    assert rows[0].pos == t.store.states[0]
    a = p0[0]
    assert rows[1].pos == ((a.frm[0] + D[a.action][0], a.frm[1] + D[a.action][1]),) + tuple(t.store.states[1][1:])


def test_overshoot_by_hand():
    """`serpentine 14x13 overshoot`: one goal state, one dead end, the start one push from the goal."""
    _, cp, _, t = TR.case("serpentine 14x13 overshoot")
    assert sorted(t.cost) == [-1, 0, 1] and t.cost[0] == 1 and t.info[4] == 1
    goal, dead = t.cost.index(0), t.cost.index(-1)
    sbc, cs = SR.cost_index(t)
    assert sbc == [goal, 0, dead] and cs == [0, 1, 2, 3]
    for env in range(6):  # the dead end is never in a band, however wide
        assert SR.draw_state(3, env, 1, 0, 1 << 30, sbc, cs) in (goal, 0)
        assert SR.draw_state(3, env, 1, 1, 1 << 30, sbc, cs) == 0
        assert SR.draw_state(3, env, 1, -5, 0, sbc, cs) == goal
    assert {SR.draw_state(3, env, 1, 0, 1, sbc, cs) for env in range(16)} == {goal, 0}
    assert SR.plan(t, dead, 0, 0, 0) is None and SR.plan(t, goal, 1, 0, 0) == []
    assert [s.node for s in SR.plan(t, 0, 0, 0, 0)] == [0]


def test_all_dead_by_hand():
    """`shape (3, 12, 9) search start 3`: 261 states, all dead -- two words of cost_start, every draw and plan -1."""
    _, cp, _, t = TR.case("shape (3, 12, 9) search start 3")
    assert t.info[4] == -1 and set(t.cost) == {-1}
    sbc, cs = SR.cost_index(t)
    assert cs == [0, 261] and sbc == list(range(261))
    for lo, hi in ((0, 0), (1, 1 << 30), (-5, 50)):
        assert SR.draw_state(7, 0, 1, lo, hi, sbc, cs) is None
    assert all(SR.plan(t, i, tie, 7, 0) is None for i in (0, 130, 260) for tie in (0, 1))


def test_band_without_a_state():
    """Listed state 29: every goal row leaves the grid, so the store has no state of cost 0 and bucket 0 is empty."""
    _, cp, _, t = TR.case("shape (8, 16, 2) listed 29")
    sbc, cs = SR.cost_index(t)
    assert cs[:2] == [0, 0] and cs[2] == 99 - 67 and cs[3] == 99 and len(cs) == 4
    assert SR.draw_state(7, 0, 1, 0, 0, sbc, cs) is None and SR.draw_state(7, 0, 1, 0, 1, sbc, cs) in sbc[:32]
    assert sbc[:32] == sorted(sbc[:32]) and sbc[32:] == sorted(sbc[32:])


@pytest.mark.parametrize("name", list(TR.EXPECT))
def test_index_of_every_case(name):
    _, cp, _, t = TR.case(name)
    sbc, cs = SR.cost_index(t)
    S, mc = t.info[0], t.info[4]
    assert sorted(sbc) == list(range(S)) and len(cs) == mc + 3 and cs[0] == 0 and cs[-1] == S
    for b in range(mc + 2):
        part = sbc[cs[b]:cs[b + 1]]
        assert part == sorted(part) and all(t.cost[i] == (b if b <= mc else -1) for i in part)
    assert cs[-1] - cs[-2] == t.info[3]


def test_tie_rules_on_big():
    _, cp, _, t = TR.case("big")
    ties = [i for i in range(t.info[0]) if sum(1 for r in range(t.row_off[i], t.row_off[i + 1]) if t.flags[r] & TR.OPTIMAL) > 1]
    assert len(ties) > 50
    i = ties[0]
    optimal = [r for r in range(t.row_off[i], t.row_off[i + 1]) if t.flags[r] & TR.OPTIMAL]
    assert optimal[0] == t.row_off[i] + t.best[i]  # best is the lowest optimal row
    for item in range(8):
        j = (_mix_by_hand(11 ^ K_PLAN, item, 0) * len(optimal)) >> 64
        first = SR.plan(t, i, 1, 11, item)[0]
        assert (first.frm, first.action) == (t.frm[optimal[j]], t.action[optimal[j]])
    assert len({(s.frm, s.action) for item in range(32) for s in SR.plan(t, i, 1, 11, item)[:1]}) == len(
        {(t.frm[r], t.action[r]) for r in optimal})
    for i in range(0, t.info[0], 7):  # every plan is as long as its start's cost, whatever the rule
        for tie in (0, 1):
            p = SR.plan(t, i, tie, 5, i)
            assert (p is None) == (t.cost[i] < 0) and (p is None or len(p) == t.cost[i])


# ---- the identity the emit relies on ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TR.EXPECT))
def test_identity_on_every_optimal_row(name):
    """For every optimal row: the oracle's successor has the agent at from + the action's displacement, and -- inside the grid
    -- the other movables of the store's state succ.  (The rows of node i are the rows of its stored state.)"""
    _, cp, _, t = TR.case(name)
    seen = 0
    for i in range(t.info[0]):
        if t.cost[i] <= 0:
            continue
        pushes = WR.region(cp, t.store.states[i]).pushes
        assert len(pushes) == t.row_off[i + 1] - t.row_off[i]
        for k, pm in enumerate(pushes):
            r = t.row_off[i] + k
            if not t.flags[r] & TR.OPTIMAL:
                continue
            seen += 1
            assert (tuple(pm.frm), pm.action) == (tuple(t.frm[r]), t.action[r])
            nxt = tuple(tuple(xy) for xy in pm.next_state)
            assert nxt[0] == (pm.frm[0] + D[pm.action][0], pm.frm[1] + D[pm.action][1])
            if t.succ[r] >= 0:
                assert nxt[1:] == tuple(tuple(xy) for xy in t.store.states[t.succ[r]][1:])
            else:  # outside its grid: a goal row, the last push of a plan -- no row is emitted after it
                assert t.flags[r] & TR.GOAL and not WR.in_grid(cp, nxt)
    assert (seen > 0) == (t.info[4] > 0)


@pytest.mark.parametrize("name", ["big", "shape (8, 16, 2) listed 30", "shape (3, 12, 9) deep goal start"])
def test_rows_from_the_oracle_satisfy_the_identity(name):
    _, cp, _, t = TR.case(name)
    n = 0
    for i in range(0, t.info[0], max(1, t.info[0] // 180)):
        for tie in (0, 1):
            steps = SR.plan(t, i, tie, 9, i)
            if not steps:
                continue
            rows = SR.rows(cp, t, i, None, steps)
            final = SR.states_along(cp, t.store.states[i], steps)[1]
            assert cp.py.is_goal_state(final)
            for k, row in enumerate(rows):
                n += 1
                assert (row.t, row.node, row.cost) == (k, steps[k].node, len(steps) - k)
                if k:
                    b = steps[k - 1]
                    assert row.pos == ((b.frm[0] + D[b.action][0], b.frm[1] + D[b.action][1]),) + tuple(
                        tuple(xy) for xy in t.store.states[row.node][1:])
    assert n >= 10


# ---- the C ABI: checks that return before any launch -----------------------------------------------------------------------------
def _einval(rc, *words):
    assert rc == _capi.PW_EINVAL
    msg = _capi.last_error()
    for w in words:
        assert w in msg, (w, msg)


def _sample(s=P, ids=P, mask=None, n=4, npad=8, counter=P, lo=1, hi=3, lo_n=None, hi_n=None, pos=P, steps=P, state=P, cost=P):
    return lib.pw_push_search_table_sample(s, ids, mask, n, npad, 7, counter, lo, hi, lo_n, hi_n, pos, steps, None, None, state, cost,
                                           None)


def _plans(s=P, index=P, ids=P, n=4, tie=0, frm=P, action=P, state=P, plan_cap=16, plan_len=P):
    return lib.pw_push_search_table_plans(s, index, ids, None, n, tie, 7, frm, action, state, plan_cap, plan_len, None)


def _emit(s=P, n=4, npad=8, frm=P, action=P, state=P, plan_cap=16, plan_len=P, pos=None, offset=P, rows_cap=10, row=P, dropped=P):
    return lib.pw_push_search_table_emit(s, None, None, n, npad, frm, action, state, plan_cap, plan_len, pos, offset, rows_cap, row,
                                         P, P, P, P, P, P, dropped, None)


@pytest.mark.parametrize("kw, words", [
    (dict(s=None), "null search"),
    (dict(n=0), "n must be"),
    (dict(n=-2), "n must be"),
    (dict(pos=None), "null pos"),
    (dict(steps=None), "null steps"),
    (dict(counter=None), "null counter"),
    (dict(state=None), "out_state"),
    (dict(cost=None), "out_cost"),
    (dict(npad=0), "npad"),
    (dict(npad=12), "npad"),
    (dict(npad=64), "npad"),
    (dict(lo=4, hi=3), "lo <= hi"),
    (dict(lo=-1, hi=3), "0 <= lo"),
    (dict(lo_n=P), "come together"),
    (dict(hi_n=P), "come together"),
])
def test_sample_argument_checks(kw, words):
    _einval(_sample(**kw), "pw_push_search_table_sample", words)


@pytest.mark.parametrize("kw, words", [
    (dict(s=None), "null search"),
    (dict(n=0), "n must be"),
    (dict(index=None), "null index"),
    (dict(frm=None), "null plan_from"),
    (dict(action=None), "plan_action"),
    (dict(plan_len=None), "plan_len"),
    (dict(plan_cap=0), "plan_cap"),
    (dict(plan_cap=-4), "plan_cap"),
    (dict(tie=2), "tie"),
    (dict(tie=-1), "tie"),
])
def test_plans_argument_checks(kw, words):
    _einval(_plans(**kw), "pw_push_search_table_plans", words)


@pytest.mark.parametrize("kw, words", [
    (dict(s=None), "null search"),
    (dict(n=0), "n must be"),
    (dict(npad=5), "npad"),
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
])
def test_emit_argument_checks(kw, words):
    _einval(_emit(**kw), "pw_push_search_table_emit", words)


def test_index_argument_checks():
    _einval(lib.pw_push_search_table_index(None, None), "pw_push_search_table_index", "null search")
    _einval(lib.pw_push_search_table_index_read(None, P, P, None), "pw_push_search_table_index_read", "null search")


def test_header_and_signatures():
    with open(os.path.join(ROOT, "include", "pushworld_amd.h")) as f:
        header = f.read()
    for name, count in NAMES.items():
        full = f"pw_push_search_table_{name}"
        assert f"int  {full}(" in header and full in _capi.SIGNATURES
        restype, argtypes = _capi.SIGNATURES[full]
        decl = header[header.index(f"int  {full}("):]
        decl = decl[:decl.index(");")]
        assert restype is ctypes.c_int and len(argtypes) == count == decl.count(",") + 1
        assert getattr(lib, full) is not None
    for words in ("IN ASCENDING STORE INDEX", "No flood", "LEFT ENTIRELY UNTOUCHED", "states_by_cost", "out_state"):
        assert words in header
    with open(os.path.join(ROOT, "pushworld_amd", "csrc", "pw_kernels.hip")) as f:
        unit = f.read()
    assert unit.index('#include "pw_push_table.inc"') < unit.index('#include "pw_push_table_sample.inc"')
    # the kernels of the draws are pw_push_draw.inc's, which needs the helpers and the scan of pw_table_sample.inc
    assert unit.index('#include "pw_table_sample.inc"') < unit.index('#include "pw_push_draw.inc"')
    assert unit.index('#include "pw_push_draw.inc"') < unit.index('#include "pw_push_table_sample.inc"')
    from pushworld_amd import build

    assert "pw_push_table_sample.inc" in build.HEADERS and "pw_push_draw.inc" in build.HEADERS
    assert _capi.ABI_VERSION == 4 and lib.pw_abi_version() == 4
    assert (search.TABLE_K_SAMPLE, search.TABLE_K_PLAN) == (K_SAMPLE, K_PLAN)


# ---- the wrappers ------------------------------------------------------------------------------------------------------------------
def _bare(npad=8):
    tab = PushSolutionTable.__new__(PushSolutionTable)
    tab.npad, tab.device, tab.puzzle_index, tab.search = npad, torch.device("cpu"), 0, None
    return tab


def test_exported_names():
    from pushworld_amd.vec_env import VecPushWorld

    for name in ("cost_index", "sample", "plans", "demonstration_rows", "covers"):
        assert callable(getattr(PushSolutionTable, name))
    assert callable(VecPushWorld.reset_from_push_tables) and callable(VecPushWorld.optimal_push_demonstrations)
    assert PushPlans._fields == ("push_from", "push_action", "state", "length")
    assert PushRows._fields == ("item", "t", "state", "push_from", "push_action", "cost", "pos", "dropped", "num_rows")
    for name in ("table_index", "table_index_read", "table_sample", "table_plans", "table_emit"):
        assert callable(getattr(_capi.PushSearchHandle, name))


def test_python_input_checks():
    """Every check raises before the library is touched: the bare table has no handle ("closed" comes last)."""
    tab = _bare()
    n = 5
    ids, pos = torch.zeros(n, dtype=torch.int32), torch.zeros((n, 8, 2), dtype=torch.int8)
    steps, flag = torch.zeros(n, dtype=torch.int32), torch.zeros(n, dtype=torch.uint8)
    ctr, i32 = torch.zeros(n, dtype=torch.int32), torch.zeros(n, dtype=torch.int32)
    for kw, words in [
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
        (dict(puzzle_id=ids[:4]), "puzzle_id"),
        (dict(mask=flag.to(torch.int32)), "mask"),
        (dict(tie="random"), "tie"),
        (dict(plan_cap=0), "plan_cap"),
        (dict(out=good[:3]), "PushPlans of an earlier call"),
        (dict(out=good._replace(push_from=good.push_from[:, :8])), "out: push_from"),
        (dict(out=good._replace(state=good.state.long())), "out: state"),
        (dict(out=good), "closed"),
    ]:
        args = dict(index=ids, puzzle_id=ids, plan_cap=16)
        args.update(kw)
        with pytest.raises(ValueError, match=words):
            tab.plans(**args)
    for kw, words in [
        (dict(plans=good[:2]), "PushPlans of a plans call"),
        (dict(plans=good._replace(length=i32.long())), "out: length"),
        (dict(pos=pos[:, :4]), "pos"),
        (dict(mask=flag[:2]), "mask"),
        (dict(offset=torch.zeros(n, dtype=torch.int64)), "offset"),
        (dict(rows_cap=-1, offset=torch.zeros(n + 1, dtype=torch.int64)), "rows_cap"),
        (dict(rows_cap=3, offset=torch.zeros(n + 1, dtype=torch.int64)), "closed"),
    ]:
        args = dict(plans=good, pos=pos)
        args.update(kw)
        with pytest.raises(ValueError, match=words):
            tab.demonstration_rows(**args)
    assert tab.covers(torch.tensor([0, 1, 0], dtype=torch.int32)).tolist() == [True, False, True]


def test_choice_is_the_inverse_of_decode():
    h, w = 5, 7
    choice = torch.arange(4 * h * w, dtype=torch.int64)
    frm, action = decode_push_choice(choice, h, w)
    assert torch.equal(encode_push_choice(frm, action, h, w), choice)
    assert frm[3 * h * w + 2 * w + 4].tolist() == [4, 2] and int(action[3 * h * w + 2 * w + 4]) == 3
    outside = encode_push_choice(torch.tensor([[7, 0], [0, 5], [-1, 0], [0, 0]], dtype=torch.int8),
                                 torch.tensor([0, 0, 0, 0xFF], dtype=torch.uint8), h, w)
    assert outside.tolist() == [-1, -1, -1, -1]

"""Host side of drawing from the cost-to-go tables (csrc/pw_table_sample.inc): the argument checks of the ``pw_solve_batch_*`` /
``pw_search_table_*`` index, sample and plans entry points that return before any launch (no device memory, no handle
dereferenced further than its "no run yet" / "no index yet" words), the input checks of the Python methods, and the numpy
restatement of the draw and of both tie rules against values worked out by hand for a 5-row toy table."""
import ctypes

import numpy as np
import pytest
import torch

from pushworld_amd import _capi, search
from pushworld_amd.search import SolutionTable, SolutionTableBatch
from table_sample_restatement import INF, K_PLAN, K_SAMPLE, clamp_band, draw_row, hash64, walk_plan

P = ctypes.c_void_p(4096)  # a stand-in for a device pointer: every check below returns before anything is read through it
lib = _capi.lib


def _einval(rc, *words):
    assert rc == _capi.PW_EINVAL
    msg = _capi.last_error()
    for w in words:
        assert w in msg, (w, msg)


class _Handle(ctypes.Structure):
    """The head of a PwSolveBatch -- an engine pointer, the caps and the item counts -- and zeros for everything behind it (the
    new members are at the END of the struct: a handle without an index)."""
    _fields_ = [("eng", ctypes.c_void_p), ("rows_cap", ctypes.c_int64), ("slots_cap", ctypes.c_int64),
                ("n_cap", ctypes.c_int32), ("n", ctypes.c_int32), ("rest", ctypes.c_uint8 * 1024)]


def _handle(n):
    h = _Handle()
    h.n = n
    return ctypes.cast(ctypes.pointer(h), ctypes.c_void_p), h


def _sample(fn, s=P, ids=P, mask=None, n=4, npad=8, counter=P, lo=1, hi=3, lo_n=None, hi_n=None, pos=P, steps=P, row=P, cost=P):
    return fn(s, ids, mask, n, npad, 7, counter, lo, hi, lo_n, hi_n, pos, steps, None, None, row, cost, None)


def _plans(fn, s=P, index=P, ids=P, n=4, tie=0, plans=P, plan_cap=16, plan_len=P):
    return fn(s, index, ids, None, n, tie, 7, plans, plan_cap, plan_len, None)


SAMPLE_CHECKS = [
    (dict(s=None), "null"),
    (dict(n=0), "n must be"),
    (dict(n=-2), "n must be"),
    (dict(pos=None), "null pos"),
    (dict(steps=None), "null steps"),
    (dict(counter=None), "null counter"),
    (dict(row=None), "out_row"),
    (dict(cost=None), "out_cost"),
    (dict(npad=0), "npad"),
    (dict(npad=12), "npad"),
    (dict(npad=64), "npad"),
    (dict(lo=4, hi=3), "lo <= hi"),
    (dict(lo=-1, hi=3), "0 <= lo"),
    (dict(lo_n=P), "come together"),
    (dict(hi_n=P), "come together"),
]


@pytest.mark.parametrize("kw, words", SAMPLE_CHECKS)
def test_sample_argument_checks(kw, words):
    # the search form: every check here comes before the search is looked at (P stands in for it)
    _einval(_sample(lib.pw_search_table_sample, **kw), "pw_search_table_sample", words)
    # the batch form, on a handle that ran but has no index: the same checks come first
    if "s" not in kw:
        kw = dict(kw, s=_handle(3)[0])
    _einval(_sample(lib.pw_solve_batch_sample, **kw), "pw_solve_batch_sample", words)


PLANS_CHECKS = [
    (dict(s=None), "null"),
    (dict(n=0), "n must be"),
    (dict(index=None), "null index"),
    (dict(plans=None), "null plans"),
    (dict(plan_len=None), "plan_len"),
    (dict(plan_cap=0), "plan_cap"),
    (dict(plan_cap=-4), "plan_cap"),
    (dict(tie=2), "tie"),
    (dict(tie=-1), "tie"),
]


@pytest.mark.parametrize("kw, words", PLANS_CHECKS)
def test_plans_argument_checks(kw, words):
    _einval(_plans(lib.pw_search_table_plans, **kw), "pw_search_table_plans", words)
    if "s" not in kw:
        kw = dict(kw, s=_handle(0)[0])
    _einval(_plans(lib.pw_solve_batch_plans, **kw), "pw_solve_batch_plans", words)


def test_batch_ids_no_run_and_no_index():
    never, ran = _handle(0)[0], _handle(3)[0]
    _einval(_sample(lib.pw_solve_batch_sample, s=ran, ids=None), "pw_solve_batch_sample", "null puzzle_id")
    _einval(_plans(lib.pw_solve_batch_plans, s=ran, ids=None), "pw_solve_batch_plans", "null puzzle_id")
    _einval(lib.pw_solve_batch_index(None, None), "pw_solve_batch_index", "null handle")
    _einval(lib.pw_solve_batch_index(never, None), "pw_solve_batch_index", "no run yet")
    _einval(lib.pw_solve_batch_index_read(None, 0, None, None, None), "pw_solve_batch_index_read", "null handle")
    _einval(lib.pw_solve_batch_index_read(never, 0, None, None, None), "pw_solve_batch_index_read", "no run yet")
    _einval(lib.pw_solve_batch_index_read(ran, 0, None, None, None), "pw_solve_batch_index_read", "no index yet")
    _einval(_sample(lib.pw_solve_batch_sample, s=never), "pw_solve_batch_sample", "no run yet")
    _einval(_sample(lib.pw_solve_batch_sample, s=ran), "pw_solve_batch_sample", "no index yet")
    _einval(_plans(lib.pw_solve_batch_plans, s=never), "pw_solve_batch_plans", "no run yet")
    _einval(lib.pw_search_table_index(None, None), "pw_search_table_index", "null search")
    _einval(lib.pw_search_table_index_read(None, None, None, None), "pw_search_table_index_read", "null search")


def _bare(cls, npad=8):
    tab = cls.__new__(cls)
    tab.npad, tab.device, tab.puzzle_index = npad, torch.device("cpu"), 0
    tab.handle = tab.search = None
    return tab


@pytest.mark.parametrize("cls", [SolutionTable, SolutionTableBatch])
def test_python_input_checks(cls):
    """Every check raises before the library is touched (the bare tables have no handle)."""
    tab = _bare(cls)
    n = 5
    ids, pos = torch.zeros(n, dtype=torch.int32), torch.zeros((n, 8, 2), dtype=torch.int8)
    steps, flag = torch.zeros(n, dtype=torch.int32), torch.zeros(n, dtype=torch.uint8)
    ctr, i32 = torch.zeros(n, dtype=torch.int32), torch.zeros(n, dtype=torch.int32)
    bad = [
        (dict(puzzle_id=ids.long()), "puzzle_id"),
        (dict(pos=pos[:, :4]), "pos"),
        (dict(pos=pos.to(torch.uint8)), "pos"),
        (dict(steps=steps.long()), "steps"),
        (dict(steps=steps[:4]), "steps"),
        (dict(terminated=flag.to(torch.int32)), "terminated"),
        (dict(truncated=flag[:3]), "truncated"),
        (dict(mask=flag[:4]), "mask"),
        (dict(cost=3), "cost"),
        (dict(cost=(3, 1)), "lo <= hi"),
        (dict(cost=(-1, 1)), "lo <= hi"),
        (dict(cost=(i32, 4)), "cost: hi"),
        (dict(cost=(i32.long(), i32)), "cost: lo"),
        (dict(cost=(i32, i32[:4])), "cost: hi"),
        (dict(counter=ctr.long()), "counter"),
        (dict(counter=torch.zeros(2 * n, dtype=torch.int32)[::2]), "contiguous"),
        (dict(out=(i32,)), "pair"),
        (dict(out=(i32, i32.long())), "out: cost"),
    ]
    for kw, words in bad:
        args = dict(puzzle_id=ids, pos=pos, steps=steps, terminated=flag, truncated=flag, counter=ctr)
        args.update(kw)
        with pytest.raises(ValueError, match=words):
            tab.sample(**args)
    bad = [
        (dict(index=ids.long()), "index"),
        (dict(index=ids[:0]), "items"),
        (dict(puzzle_id=ids[:4]), "puzzle_id"),
        (dict(mask=flag.to(torch.int32)), "mask"),
        (dict(tie="random"), "tie"),
        (dict(tie=1), "tie"),
        (dict(plan_cap=0), "plan_cap"),
        (dict(out=(torch.zeros((n, 8), dtype=torch.uint8), i32)), "out: plans"),
        (dict(out=(torch.zeros((n, 16), dtype=torch.uint8), i32.long())), "out: plan_len"),
    ]
    for kw, words in bad:
        args = dict(index=ids, puzzle_id=ids, plan_cap=16)
        args.update(kw)
        with pytest.raises(ValueError, match=words):
            tab.plans(**args)
    if cls is SolutionTableBatch:  # a mixed batch cannot do without the ids
        with pytest.raises(ValueError, match="puzzle_id"):
            tab.plans(ids, None)
        with pytest.raises(ValueError, match="puzzle_id"):
            tab.sample(None, pos, steps)
    tab.device = torch.device("cuda", 0)
    with pytest.raises(ValueError, match="live on"):
        tab.plans(ids, ids)


def test_exported_names():
    from pushworld_amd.vec_env import VecPushWorld

    for cls in (SolutionTable, SolutionTableBatch):
        for name in ("cost_index", "sample", "plans", "covers"):
            assert callable(getattr(cls, name))
    assert callable(VecPushWorld.reset_from_tables) and callable(VecPushWorld.optimal_demonstrations)
    assert (search.TABLE_K_SAMPLE, search.TABLE_K_PLAN) == (K_SAMPLE, K_PLAN) and search.TABLE_TIES == {"lowest": 0, "uniform": 1}
    assert (search.PLANS_NONE, search.PLANS_CUT) == (-1, -2)
    assert {"cost", "acts"} <= set(search.PlanReplay.__slots__)
    for form in ("pw_solve_batch", "pw_search_table"):
        for name in ("index", "index_read", "sample", "plans"):
            assert f"{form}_{name}" in _capi.SIGNATURES and hasattr(lib, f"{form}_{name}")
    assert _capi.ABI_VERSION == 4 and lib.pw_abi_version() == 4


# ---- the restatement against a toy table worked out by hand ----------------------------------------------------------------------
# rows 0 .. 4 with costs 2, 1, 0, dead, 1.  Row 0 ties: action 0 leads to row 1, action 3 to row 4; row 4 ties: actions 1 and 2
# both lead to the goal row 2; row 1 has the one optimal action 1.
COST = np.array([2, 1, 0, INF, 1], dtype=np.uint16)
SUCC = np.array([[1, 0, 0, 4], [1, 2, 1, 1], [2, 2, 2, 2], [3, 3, 3, 3], [4, 2, 2, 4]], dtype=np.int32)
ACTS = np.array([0xF0 | 0b1001, 0xF0 | 0b0010, 0xF0, 0x00, 0xF0 | 0b0110], dtype=np.uint8)
ROWS_BY_COST = np.array([2, 1, 4, 0, 3], dtype=np.int32)  # cost 0 | cost 1, cost 1 | cost 2 | dead
COST_START = np.array([0, 1, 3, 4, 5], dtype=np.uint32)   # max_cost + 3 = 5 entries


def _mix_by_hand(seed, a, b):
    """pw_mix64 in plain Python integers (no numpy): the splitmix64 finaliser over seed + c1 (a + 1) + c2 b."""
    m = (1 << 64) - 1
    z = (seed + 0x9E3779B97F4A7C15 * (a + 1) + 0xD1B54A32D192ED03 * b) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)


def test_hash_values():
    # seed 7: the hash words the cases below were worked out from
    assert _mix_by_hand(7 ^ K_SAMPLE, 0, 1) == 0x717A53E9E02ECF93 and _mix_by_hand(7 ^ K_SAMPLE, 2, 2) == 0xC847A40F2FF95144
    for a, b in ((0, 1), (0, 2), (1, 1), (2, 1), (2, 2), (3, 1)):
        assert hash64(7 ^ K_SAMPLE, a, b) == _mix_by_hand(7 ^ K_SAMPLE, a, b)
        assert hash64(7 ^ K_PLAN, a, b) == _mix_by_hand(7 ^ K_PLAN, a, b)
        assert hash64(7 ^ K_SAMPLE, a, b) == lib.pw_mix64(7 ^ K_SAMPLE, a, b)


def test_band_clamp():
    assert clamp_band(1, 2, 2) == (1, 2) and clamp_band(0, 10 ** 9, 2) == (0, 2)
    assert clamp_band(5, 9, 2) == (2, 2)      # lo > max_cost: lo = hi = max_cost
    assert clamp_band(2, 1, 2) == (2, 2)      # hi < lo reads as hi = lo
    assert clamp_band(-3, 0, 2) == (0, 0) and clamp_band(-3, -1, 2) == (0, 0)
    assert clamp_band(1, 1, 0) == (0, 0)


@pytest.mark.parametrize("env, counter, lo, hi, row", [
    # 0x717a53e9e02ecf93 * 3 >> 64 = 1: the band 1 .. 2 holds rows_by_cost[1 : 4] = 1, 4, 0
    (0, 1, 1, 2, 4),
    # 0xf36aa0dbb4643677 * 4 >> 64 = 3: the band 0 .. 2 holds rows_by_cost[0 : 4]
    (0, 2, 0, 2, 0),
    # 0x098be401b0c85239 * 4 >> 64 = 0
    (1, 1, 0, 2, 2),
    # 0x90aa2ca2dbf5d179 * 2 >> 64 = 1: cost 1 alone holds rows 1, 4
    (2, 1, 1, 1, 4),
    # beyond max_cost: lo = hi = 2, the one row of cost 2 whatever the hash
    (2, 2, 5, 9, 0),
    (3, 1, 2, 1, 0),
    (3, 1, -3, 0, 2),
    # 0x5e3c67c285fbdc88 * 4 >> 64 = 1: the dead end (row 3) is never in a band, however wide
    (3, 1, 0, 1 << 30, 1),
])
def test_draw_by_hand(env, counter, lo, hi, row):
    assert draw_row(7, env, counter, lo, hi, ROWS_BY_COST, COST_START) == row


def test_draw_without_a_finite_row():
    assert draw_row(7, 0, 1, 0, 5, np.array([0, 1, 2]), np.array([0, 0, 3], dtype=np.uint32)) is None


def test_draw_is_uniform_over_the_band():
    """4 000 environments over the band 1 .. 2 (three rows): every row about a third (chi-square, 2 degrees of freedom: 13.8
    is the 0.1 % point)."""
    rows = [draw_row(11, env, 1, 1, 2, ROWS_BY_COST, COST_START) for env in range(4000)]
    counts = np.array([rows.count(r) for r in (1, 4, 0)])
    assert counts.sum() == 4000 and (((counts - 4000 / 3) ** 2) / (4000 / 3)).sum() < 13.8


@pytest.mark.parametrize("row, tie, item, plan", [
    (0, 0, 0, [0, 1]),   # the lowest optimal action at every step
    (4, 0, 1, [1]),
    (2, 0, 0, []),       # a goal row
    (3, 0, 0, None),     # a dead end
    (3, 1, 0, None),
    (0, 1, 0, [3, 1]),   # item 0: j = 1, 0 at steps 0, 1 -- the second of actions {0, 3}, then the first of {1, 2}
    (0, 1, 2, [3, 2]),   # item 2: j = 1, 1
    (4, 1, 1, [2]),      # item 1: j = 1 at step 0
    (1, 1, 2, [1]),      # one optimal action: the hash does not matter
])
def test_walk_by_hand(row, tie, item, plan):
    assert walk_plan(ACTS, SUCC, COST, row, tie, 7, item) == plan

"""Host side of the cost-to-go guidance inside the step (``pw_guide_step`` / ``guide.ValueGuide`` / ``set_guide``, DESIGN.md
K28): the header and ``SIGNATURES``, the argument checks that return before anything touches a device, the wrappers' checks
that come before an engine is asked for, and properties of the restatement (tests/value_guide_restatement.py)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import value_guide_restatement as VR
from pushworld_amd import _capi
from pushworld_amd.guide import ValueGuide, check_guide_options
from pushworld_amd.search import PushSolutionTable, PushSolutionTableBatch, SolutionTable, SolutionTableBatch
from pushworld_amd.vec_env import VecPushWorld
from pushworld_amd.vector_env import (PushWorldDmVectorEnv, PushWorldPushDmVectorEnv, PushWorldPushVectorEnv,
                                      PushWorldVectorEnv)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p(4096)  # a stand-in for an engine or a buffer: every check below returns before anything is read through it


def test_header_and_signatures():
    with open(os.path.join(ROOT, "include", "pushworld_amd.h")) as f:
        header = f.read()
    assert "int pw_guide_step(PwEngine* e, PwSolveBatch* tables," in header
    assert "pw_guide_step" in _capi.SIGNATURES and hasattr(_capi.lib, "pw_guide_step")
    assert len(_capi.SIGNATURES["pw_guide_step"][1]) == 23
    for name, value in (("AUTORESET", "1u"), ("END_DEAD", "2u"), ("REFRESH", "4u"), ("COUNTS", "4"), ("GUIDED", "0"),
                        ("OPTIMAL", "1"), ("DEAD_ENTERED", "2"), ("UNKNOWN", "3")):
        assert f"#define PW_GUIDE_{name} {value}" in header, name
    assert (_capi.GUIDE_AUTORESET, _capi.GUIDE_END_DEAD, _capi.GUIDE_REFRESH) == (VR.AUTORESET, VR.END_DEAD, VR.REFRESH) == (1, 2, 4)
    assert _capi.GUIDE_AUTORESET == _capi.STEP_AUTORESET
    assert (_capi.GUIDE_GUIDED, _capi.GUIDE_OPTIMAL, _capi.GUIDE_DEAD_ENTERED, _capi.GUIDE_UNKNOWN) == \
        (VR.GUIDED, VR.OPTIMAL, VR.DEAD_ENTERED, VR.UNKNOWN) == (0, 1, 2, 3) and _capi.GUIDE_COUNTS == 4
    assert _capi.lib.pw_abi_version() == _capi.ABI_VERSION == 4
    with open(os.path.join(ROOT, "pushworld_amd", "csrc", "pw_kernels.hip")) as f:
        assert '#include "pw_guide.inc"' in f.read()


def _args(**kw):
    """A well-formed applied-form argument list of ``pw_guide_step`` over stand-in pointers, with replacements by name."""
    a = dict(e=P, tables=None, cost_in=P, acts_in=P, puzzle_id=P, pos=P, npad=8, reward=P, terminated=P, truncated=P, mask=None,
             n=4, cost=P, acts=P, seen=P, dead=P, shaped=P, dead_cost=P, gamma=0.99, scale=0.1, counts=P, flags=3, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return tuple(a.values())


def test_guide_step_argument_checks():
    for kw, words in ((dict(e=None), "null engine"),
                      (dict(tables=P), "exactly one"),                       # both sources
                      (dict(tables=P, acts_in=None), "exactly one"),
                      (dict(cost_in=None, acts_in=None), "no source"),       # neither
                      (dict(tables=P, cost_in=None), "acts_in goes with cost_in"),
                      (dict(puzzle_id=None), "null puzzle_id"),
                      (dict(pos=None), "null pos"),
                      (dict(npad=0), "npad"), (dict(npad=5), "npad"), (dict(npad=64), "npad"), (dict(npad=-4), "npad"),
                      (dict(terminated=None), "null terminated"),
                      (dict(truncated=None), "null truncated"),
                      (dict(n=-1), "n must be >= 0"), (dict(n=-(1 << 31)), "n must be >= 0"),
                      (dict(cost=None), "null cost"),
                      (dict(acts=None), "null acts"),
                      (dict(seen=None), "null seen"),
                      (dict(dead=None), "null dead"),
                      (dict(reward=None), "null reward"),
                      (dict(dead_cost=None), "null dead_cost"),
                      (dict(flags=8), "unknown flags"), (dict(flags=1 << 31), "unknown flags"), (dict(flags=0x107), "unknown flags")):
        assert _capi.lib.pw_guide_step(*_args(**kw)) == _capi.PW_EINVAL, kw
        msg = _capi.last_error()
        assert "pw_guide_step" in msg and words in msg, (kw, msg)


class _Set:
    def __len__(self):
        return 5


def _engine():
    """An ``Engine`` without a handle: a call that gets past the wrapper's checks fails with AttributeError."""
    e = _capi.Engine.__new__(_capi.Engine)
    e.pset, e.np = _Set(), 4
    return e


def test_engine_wrapper_checks():
    e = _engine()
    i32, u8, f64 = torch.zeros(3, dtype=torch.int32), torch.zeros(3, dtype=torch.uint8), torch.zeros(3, dtype=torch.float64)
    pos = torch.zeros((3, 4, 2), dtype=torch.int8)
    good = dict(tables=None, cost_in=i32, acts_in=u8, puzzle_id=i32, pos=pos, reward=f64, terminated=u8, truncated=u8, mask=None,
                cost=i32, acts=u8, seen=u8, dead=u8, shaped=f64, dead_cost=torch.zeros(5, dtype=torch.int32), gamma=1.0,
                scale=1.0, counts=torch.zeros((5, 4), dtype=torch.int64), flags=1)
    for kw, words in ((dict(cost_in=None, acts_in=None), "exactly one source"),
                      (dict(tables=ctypes.c_void_p(64)), "exactly one source"),
                      (dict(puzzle_id=i32.to(torch.int64)), "puzzle_id"),
                      (dict(pos=torch.zeros((3, 8, 2), dtype=torch.int8)), "pos"),
                      (dict(cost_in=torch.zeros(4, dtype=torch.int32)), "cost_in"),
                      (dict(acts_in=u8.to(torch.int8)), "acts_in"),
                      (dict(reward=f64.to(torch.float32)), "reward"),
                      (dict(reward=None), "reward"),
                      (dict(terminated=u8.to(torch.bool)), "terminated"),
                      (dict(truncated=torch.zeros(6, dtype=torch.uint8)[::2]), "truncated"),
                      (dict(mask=u8.to(torch.bool)), "mask"),
                      (dict(cost=i32.to(torch.int16)), "cost"),
                      (dict(acts=i32), "acts"),
                      (dict(seen=None), "seen"),
                      (dict(dead=torch.zeros(2, dtype=torch.uint8)), "dead"),
                      (dict(shaped=f64.to(torch.float32)), "shaped"),
                      (dict(dead_cost=torch.zeros(4, dtype=torch.int32)), "dead_cost"),
                      (dict(dead_cost=None), "dead_cost"),
                      (dict(counts=torch.zeros((5, 3), dtype=torch.int64)), "counts"),
                      (dict(flags=8), "unknown flags"), (dict(flags=-1), "unknown flags")):
        for call in (e.guide_step, e.bind_guide_step):
            with pytest.raises(ValueError, match="pw_guide_step: .*" + words):
                call(**{**good, **kw})
    with pytest.raises(AttributeError, match="handle"):  # good arguments do reach the library
        e.guide_step(**good)
    with pytest.raises(AttributeError, match="handle"):  # ... without the optional ones too
        e.guide_step(**{**good, "acts_in": None, "reward": None, "shaped": None, "dead_cost": None, "counts": None, "flags": 4})


def _vec(autoreset=False):
    vec = VecPushWorld.__new__(VecPushWorld)
    vec.flags, vec.engine = (_capi.STEP_AUTORESET if autoreset else 0), object()
    return vec


def test_value_guide_refusals_need_no_engine():
    with pytest.raises(ValueError, match="expected a VecPushWorld"):
        ValueGuide(object(), [])
    vec = _vec()
    for kw, words in ((dict(gamma=float("nan")), "gamma must be a finite number"), (dict(gamma="1"), "gamma must be"),
                      (dict(gamma=True), "gamma must be"), (dict(scale=float("inf")), "scale must be a finite number"),
                      (dict(scale=None), "scale must be"), (dict(dead_cost=-1), "dead_cost must be"),
                      (dict(dead_cost=1 << 31), "dead_cost must be"), (dict(dead_cost=2.5), "dead_cost must be"),
                      (dict(dead_cost=True), "dead_cost must be"), (dict(end_dead=True), "end_dead needs autoreset")):
        with pytest.raises(ValueError, match=words):
            ValueGuide(vec, [], **kw)
        with pytest.raises(ValueError, match=words):
            vec.set_guide([], **kw)
    check_guide_options(0.99, 0.1, None, True, True)
    check_guide_options(1, 0, 7, False, False)
    for bad in ([], (), None, "tables", 5):
        with pytest.raises(ValueError, match="tables must be one SolutionTableBatch or a non-empty list"):
            ValueGuide(_vec(True), bad, end_dead=True)
    with pytest.raises(ValueError, match="tables must be SolutionTable .* not int"):
        ValueGuide(vec, [5])
    moves = [SolutionTable.__new__(SolutionTable), SolutionTableBatch.__new__(SolutionTableBatch)]
    pushes = [PushSolutionTable.__new__(PushSolutionTable), PushSolutionTableBatch.__new__(PushSolutionTableBatch)]
    for m in moves:
        for p in pushes:
            with pytest.raises(ValueError, match="mixed levels"):
                ValueGuide(vec, [m, p])
    for batch in (moves[1], pushes[1]):  # tables of another engine: refused before anything is allocated
        batch.engine = object()
        with pytest.raises(ValueError, match="must be made on this environment"):
            ValueGuide(vec, [batch])
    with pytest.raises(ValueError, match="must be made on this environment"):
        vec.set_guide(moves[1])


def test_set_guide_refusals_need_no_engine():
    vec = _vec()
    assert vec.guide is None and vec.cost is None and vec.dead is None and vec.shaped_reward is None
    assert vec.set_guide(None) is None
    with pytest.raises(ValueError, match="takes no options"):
        vec.set_guide(None, gamma=0.9)
    other = ValueGuide.__new__(ValueGuide)
    other.vec = _vec()
    with pytest.raises(ValueError, match="must be made on this environment"):
        vec.set_guide(other)
    with pytest.raises(ValueError, match="carries its own options"):
        vec.set_guide(other, end_dead=True)
    vec.guide = object()  # a guide is set: the steps inside a rollout or a mailbox could not be looked up
    with pytest.raises(RuntimeError, match=r"rollout\(\) is not available while a guide is set"):
        vec.rollout(None)
    with pytest.raises(RuntimeError, match=r"mailbox\(\) is not available while a guide is set"):
        vec.mailbox()
    vec.guide = None
    for cls in (PushWorldVectorEnv, PushWorldDmVectorEnv, PushWorldPushVectorEnv, PushWorldPushDmVectorEnv):
        env = cls.__new__(cls)
        env.vec = _vec()
        assert env.use_shaped_reward is False
        with pytest.raises(ValueError, match="use_shaped_reward needs a guide with shaping"):
            env.set_guide(None, use_shaped_reward=True)
        with pytest.raises(ValueError, match="use_shaped_reward needs a guide with shaping"):
            env.set_guide([], use_shaped_reward=True, shaping=False)
        with pytest.raises(ValueError, match="end_dead needs autoreset"):  # the passthrough reaches VecPushWorld's checks
            env.set_guide([], end_dead=True)
        assert env.set_guide(None) is None and env.use_shaped_reward is False
        info = {"puzzle_id": 1}
        assert env._guide_info(info) == {"puzzle_id": 1} and env._reward("r") == "r"  # without a guide nothing changes
    g = ValueGuide.__new__(ValueGuide)
    g.counts = None
    with pytest.raises(RuntimeError, match="keeps no counts"):
        g.stats()
    g.counts = torch.tensor([[4, 1, 1, 0], [0, 0, 0, 3]], dtype=torch.int64)
    st = g.stats()
    assert st.guided.tolist() == [4, 0] and st.optimal.tolist() == [1, 0] and st.dead_entered.tolist() == [1, 0]
    assert st.unknown.tolist() == [0, 3] and st.optimal_rate[0] == 0.25 and np.isnan(st.optimal_rate[1])
    g.acts = torch.tensor([0x35, 0xF0, 0x0A], dtype=torch.uint8)
    assert g.optimal_actions.tolist() == [5, 0, 10] and g.safe_actions.tolist() == [3, 15, 0]


# ---- properties of the restatement ---------------------------------------------------------------------------------------------
def _one(look_cost, **kw):
    """One restated call on a batch of environments of puzzle 0 with the given looked-up costs."""
    n = len(look_cost)
    a = dict(puzzle_id=[0] * n, pos=np.zeros((n, 4, 2), np.int8), reward=[-0.01] * n, terminated=[0] * n, truncated=[0] * n,
             cost=[-2] * n, acts=[0] * n, seen=[0] * n, dead=[0] * n, dead_cost=[9], gamma=1.0, scale=0.25, flags=0)
    a.update(kw)
    return VR.guide_step(VR.ArrayLookup(look_cost), **a)


def test_shaping_telescopes_with_gamma_one():
    """With gamma = 1 the F of an uncut episode sums to phi(last) - phi(first) (scale 0.25 and integer costs: every sum is
    exact in doubles, so the comparison is too), dead ends included."""
    rng = np.random.default_rng(7)
    for trial in range(20):
        costs = [int(c) for c in rng.integers(-1, 12, size=30)]  # -1: a dead end, worth dead_cost = 9
        prev, total = _one([costs[0]], flags=VR.REFRESH), 0.0
        assert prev["shaped"][0] == 0.0 and prev["counts"].sum() == 0
        for c in costs[1:]:
            prev = _one([c], cost=prev["cost"], seen=prev["seen"], reward=[0.0])
            total += float(prev["shaped"][0])
        phi = [-(0.25 * float(9 if c == -1 else c)) for c in (costs[0], costs[-1])]
        assert total == phi[1] - phi[0], trial
    # an unknown state in the middle breaks the chain on both of its sides: F = 0 there
    r = _one([-2], cost=[5])
    assert r["shaped"][0] == -0.01 and r["counts"][0].tolist() == [0, 0, 0, 1]
    r = _one([4], cost=[-2])
    assert r["shaped"][0] == -0.01 and r["counts"][0].tolist() == [0, 0, 0, 0]
    # gamma and scale that are no binary fractions: two roundings, never one
    r = _one([3], cost=[4], gamma=0.99, scale=0.1, reward=[0.0])
    assert r["shaped"][0] == 0.99 * -(0.1 * 3.0) - -(0.1 * 4.0)


def test_counts_and_the_fresh_step():
    rng = np.random.default_rng(11)
    n = 500
    kw = dict(puzzle_id=rng.integers(-1, 4, size=n).tolist(), terminated=rng.choice([0, 0, 0, 1, 0xFF], size=n).tolist(),
              truncated=rng.choice([0, 0, 0, 1], size=n).tolist(), cost=rng.integers(-2, 6, size=n).tolist(),
              seen=rng.choice([0, 0, 1], size=n).tolist(), dead_cost=[7, 7, 7], reward=rng.normal(size=n).tolist())
    look = rng.integers(-2, 6, size=n).tolist()
    for flags in (0, VR.AUTORESET, VR.AUTORESET | VR.END_DEAD, VR.END_DEAD):
        r = _one(look, flags=flags, **kw)
        c = r["counts"]
        assert (c[:, VR.OPTIMAL] <= c[:, VR.GUIDED]).all() and (c[:, VR.DEAD_ENTERED] <= c[:, VR.GUIDED]).all()
        assert (c >= 0).all() and c[:, VR.GUIDED].sum() + c[:, VR.UNKNOWN].sum() <= n
        assert r["ended"] == (r["truncated"] != np.array(kw["truncated"])).sum() == r["branches"]["cut"]
        assert (r["cost"] == np.array(look)).all() and (r["dead"] == (np.array(look) == -1)).all()
        if not flags & VR.END_DEAD:
            assert r["ended"] == 0
    # a fresh step contributes nothing: no count, F = 0, never cut -- but the outputs are written
    r = _one([-1, 3, -2], cost=[4, 4, 4], seen=[1, 1, 1], flags=VR.AUTORESET | VR.END_DEAD, reward=[0.0, 0.0, 0.0])
    assert r["counts"].sum() == 0 and r["ended"] == 0 and r["truncated"].tolist() == [0, 0, 0]
    assert r["shaped"].tolist() == [0.0, 0.0, 0.0] and r["cost"].tolist() == [-1, 3, -2] and r["seen"].tolist() == [0, 0, 0]
    assert r["dead"].tolist() == [1, 0, 0]
    # the same inputs without autoreset are ordinary steps: the first is cut and enters a dead end
    r = _one([-1, 3, -2], cost=[4, 4, 4], seen=[1, 1, 1], flags=VR.END_DEAD, reward=[0.0, 0.0, 0.0])
    assert r["counts"][0].tolist() == [2, 1, 1, 1] and r["ended"] == 1 and r["truncated"].tolist() == [1, 0, 0]
    assert r["seen"].tolist() == [1, 0, 0]
    # a refused action (flags 0xFF): nothing counted, F = 0, not cut; the flags make it `seen`
    r = _one([-1], cost=[2], terminated=[0xFF], truncated=[0xFF], flags=VR.AUTORESET | VR.END_DEAD)
    assert r["counts"].sum() == 0 and r["ended"] == 0 and r["shaped"][0] == -0.01 and r["seen"][0] == 1
    # a masked environment gets nothing written; an id outside the set is shaped with dead_cost 0 and not counted
    r = _one([3, -1], cost=[4, 2], mask=[0, 1], puzzle_id=[0, 5], shaped=[123.0, 123.0], reward=[0.0, 0.0])
    assert r["cost"].tolist() == [4, -1] and r["shaped"].tolist() == [123.0, -(0.25 * 0.0) - -(0.25 * 2.0)]
    assert r["counts"].sum() == 0

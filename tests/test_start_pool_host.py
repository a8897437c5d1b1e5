"""Host side of the start-state pools (``pw_start_pool_arm`` / ``pw_start_pool_draw`` / ``pw_start_pool_update_bands``,
DESIGN.md K27): the header and ``SIGNATURES``, the argument checks that return before anything touches a device, the grouping
on CPU tensors against the restatement (tests/start_pool_restatement.py), the wrappers' refusals that come before an engine
is asked for, and the restatement against draws and band moves worked out by hand."""
import ctypes
import os

import numpy as np
import pytest
import torch

import start_pool_restatement as SR
from pushworld_amd import _capi
from pushworld_amd.start_pool import StartPool, check_start_options, group_entries, keep_to_q16
from pushworld_amd.vec_env import VecPushWorld
from pushworld_amd.vector_env import (PushWorldDmVectorEnv, PushWorldPushDmVectorEnv, PushWorldPushVectorEnv,
                                      PushWorldVectorEnv)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p(4096)  # a stand-in for an engine or a buffer: every check below returns before anything is read through it
NAMES = ("pw_start_pool_arm", "pw_start_pool_draw", "pw_start_pool_update_bands")


def test_header_and_signatures():
    with open(os.path.join(ROOT, "include", "pushworld_amd.h")) as f:
        header = f.read()
    for name in NAMES:
        assert f"int {name}(PwEngine* e," in header and name in _capi.SIGNATURES and hasattr(_capi.lib, name)
    assert f"#define PW_START_POOL_K_DRAW 0x{SR.K_DRAW:016X}ull\n" in header
    assert f"#define PW_START_POOL_K_KEEP 0x{SR.K_KEEP:016X}ull\n" in header
    # the two streams are new: not the table draws' (PW_TABLE_K_SAMPLE / PW_TABLE_K_PLAN)
    assert len({SR.K_DRAW, SR.K_KEEP, 0xA0761D6478BD642F, 0xE7037ED1A0B428DB}) == 4
    assert len(_capi.SIGNATURES["pw_start_pool_arm"][1]) == 6
    assert len(_capi.SIGNATURES["pw_start_pool_draw"][1]) == 27
    assert len(_capi.SIGNATURES["pw_start_pool_update_bands"][1]) == 14
    # the render of the pool path: pw_render's signature
    assert "int pw_render_retained(PwEngine* e," in header and hasattr(_capi.lib, "pw_render_retained")
    assert _capi.SIGNATURES["pw_render_retained"] == _capi.SIGNATURES["pw_render"]
    assert _capi.lib.pw_abi_version() == _capi.ABI_VERSION == 4


def _refused(name, args, words):
    assert getattr(_capi.lib, name)(*args) == _capi.PW_EINVAL, (name, words)
    msg = _capi.last_error()
    assert name in msg and words in msg, (name, words, msg)


def test_render_retained_argument_checks():
    _refused("pw_render_retained", (None, P, P, P, 64, 4, None), "null engine")
    assert _capi.lib.pw_render_retained(P, P, P, P, 64, 0, None) == 0  # an empty batch is a no-op, as for pw_render


def test_arm_argument_checks():
    for args, words in (((None, P, P, P, 4, None), "null engine"),
                        ((P, None, P, P, 4, None), "null terminated"),
                        ((P, P, None, P, 4, None), "null truncated"),
                        ((P, P, P, None, 4, None), "null pending"),
                        ((P, P, P, P, -1, None), "n must be"),
                        ((P, P, P, P, -(1 << 31), None), "n must be")):
        _refused("pw_start_pool_arm", args, words)


def _draw_args(**kw):
    a = dict(e=P, pool_pos=P, pool_level=P, order=P, start=P, start_words=9, lvl_off=P, max_level=P, num_entries=5,
             puzzle_id=P, mask=None, n=4, seed=1, counter=P, keep_q16=0, lo=0, hi=-1, band=None, lo_n=None, hi_n=None, pos=P,
             steps=P, terminated=None, truncated=None, out_entry=P, out_level=P, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return tuple(a.values())


def test_draw_argument_checks():
    for kw, words in ((dict(e=None), "null engine"), (dict(pool_pos=None), "null pool_pos"),
                      (dict(pool_level=None), "null pool_level"), (dict(order=None), "null order"),
                      (dict(start=None), "null start"), (dict(start_words=0), "start_words"),
                      (dict(lvl_off=None), "null lvl_off"), (dict(max_level=None), "null max_level"),
                      (dict(num_entries=0), "num_entries"), (dict(num_entries=-3), "num_entries"),
                      (dict(puzzle_id=None), "null puzzle_id"), (dict(n=-1), "n must be"),
                      (dict(counter=None), "null counter"), (dict(keep_q16=65537), "keep_q16"),
                      (dict(keep_q16=(1 << 32) - 1), "keep_q16"), (dict(lo_n=P), "lo_n and hi_n"),
                      (dict(hi_n=P, band=P), "lo_n and hi_n"), (dict(pos=None), "null pos"), (dict(steps=None), "null steps"),
                      (dict(out_entry=None), "null out_entry"), (dict(out_level=None), "null out_level")):
        _refused("pw_start_pool_draw", _draw_args(**kw), words)


def _bands_args(**kw):
    a = dict(e=P, max_level=P, stats=P, base=P, band=P, delta=None, min_episodes=32, up_q16=52429, down_q16=13107, step=1,
             width=0, hi_min=1, lo_min=1, stream=None)
    assert set(kw) <= set(a)
    a.update(kw)
    return tuple(a.values())


def test_update_bands_argument_checks():
    for kw, words in ((dict(e=None), "null engine"), (dict(max_level=None), "null max_level"), (dict(stats=None), "null stats"),
                      (dict(base=None), "null base"), (dict(band=None), "null band"), (dict(min_episodes=0), "min_episodes"),
                      (dict(min_episodes=-5), "min_episodes"), (dict(up_q16=65537), "up_q16"),
                      (dict(down_q16=65537, up_q16=65536), "down_q16"), (dict(up_q16=100, down_q16=101), "up_q16 must not be below"),
                      (dict(step=0), "step"), (dict(step=-1), "step"), (dict(width=-1), "width")):
        _refused("pw_start_pool_update_bands", _bands_args(**kw), words)


# ---- the grouping on CPU tensors ----------------------------------------------------------------------------------------------
def _grouped(puzzle, level, num_puzzles):
    order, max_level, lvl_off, start = group_entries(torch.tensor(puzzle, dtype=torch.int32),
                                                     torch.tensor(level, dtype=torch.int32), num_puzzles)
    assert (order.dtype, max_level.dtype, lvl_off.dtype, start.dtype) == (torch.int32, torch.int32, torch.int64, torch.uint32)
    return order.tolist(), max_level.tolist(), lvl_off.tolist(), start.view(torch.int32).tolist()


def test_grouping_by_hand():
    # puzzle 0: levels 0 and 2 (1 empty), a duplicate pair; puzzle 1: nothing; puzzle 2: one level, given in descending order
    puzzle = [2, 0, 2, 0, 0, 2, 0]
    level = [3, 2, 3, 0, 2, 3, 0]
    got = _grouped(puzzle, level, 4)
    assert got == ([3, 6, 1, 4, 0, 2, 5], [2, -1, 3, -1], [0, 4, 5, 10], [0, 2, 2, 4, 4, 4, 4, 4, 4, 7, 7])
    assert got == tuple(SR.group(puzzle, level, 4))


@pytest.mark.parametrize("seed", range(4))
def test_grouping_against_the_restatement(seed):
    rng = np.random.default_rng(seed)
    num_puzzles, S = 7, 200
    puzzle = rng.choice([0, 1, 3, 4, 6], size=S)  # puzzles 2 and 5 have no entries
    level = rng.choice([0, 1, 2, 5, 9], size=S)   # empty levels between full ones
    if seed == 1:  # entries given in descending key order: stability shows as ascending entries inside a bucket
        keys = np.argsort(-(puzzle * 16 + level), kind="stable")
        puzzle, level = puzzle[keys], level[keys]
    if seed == 2:  # every entry twice
        puzzle, level = np.concatenate([puzzle, puzzle]), np.concatenate([level, level])
    got = _grouped(puzzle.tolist(), level.tolist(), num_puzzles)
    assert got == tuple(SR.group(puzzle, level, num_puzzles))
    order, max_level, lvl_off, start = got
    assert sorted(order) == list(range(len(puzzle))) and max_level[2] == max_level[5] == -1
    for p in range(num_puzzles):
        for lv in range(max_level[p] + 1):
            bucket = order[start[lvl_off[p] + lv]:start[lvl_off[p] + lv + 1]]
            assert bucket == [e for e in range(len(puzzle)) if puzzle[e] == p and level[e] == lv]


class _Set:
    def __len__(self):
        return 3


def _engine(npad=4):
    """An ``Engine`` without a handle on the CPU: a call that gets past the wrapper's checks fails with AttributeError."""
    e = _capi.Engine.__new__(_capi.Engine)
    e.pset, e.np, e.device = _Set(), npad, torch.device("cpu")
    return e


def _pool(engine=None):
    pos = np.zeros((5, 4, 2), np.int8)
    pos[:, 0, 0] = np.arange(5)
    return StartPool(engine or _engine(), [0, 0, 2, 2, 2], [1, 0, 3, 0, 3], pos)


def test_start_pool_object():
    pool = _pool()
    assert (pool.num_puzzles, pool.npad, pool.num_entries) == (3, 4, 5)
    assert pool.order.tolist() == [1, 0, 3, 2, 4] and pool.max_level.tolist() == [1, -1, 3]
    assert pool.lvl_off.tolist() == [0, 3, 4] and pool.start.view(torch.int32).tolist() == [0, 1, 2, 2, 2, 3, 3, 3, 5]
    assert pool.band.tolist() == [[1, 1], [0, 0], [1, 1]] and pool.band.dtype == torch.int32
    assert pool.base.shape == (3, 4) and pool.base.dtype == torch.int64 and pool.delta.dtype == torch.int8
    assert pool.bucket(2, 3).tolist() == [2, 4] and pool.bucket(2, 1).tolist() == [] and pool.bucket(0, 5).tolist() == []
    pool.set_band(0, None)
    assert pool.band.tolist() == [[0, -1]] * 3
    pool.set_band([0, 1, 2], [3, 3, 3])
    assert pool.band.tolist() == [[0, 3], [1, 3], [2, 3]]
    # tensors are taken as well as arrays
    same = StartPool(_engine(), torch.tensor([0, 0, 2, 2, 2]), torch.tensor([1, 0, 3, 0, 3]), pool.pos.clone())
    assert same.order.tolist() == pool.order.tolist() and same.pos.dtype == torch.int8


def test_start_pool_refusals():
    class NoEngine:
        @property
        def engine(self):
            raise AssertionError("an engine was asked for")

    pos = np.zeros((2, 4, 2), np.int8)
    with pytest.raises(ValueError, match="S = 0"):
        StartPool(NoEngine(), [], [], np.zeros((0, 4, 2), np.int8))
    with pytest.raises(ValueError, match=r"pos must be \[S, npad, 2\]"):
        StartPool(NoEngine(), [0, 0], [0, 0], np.zeros((2, 4), np.int8))
    with pytest.raises(ValueError, match="one integer per entry"):
        StartPool(NoEngine(), [0], [0, 0], pos)
    with pytest.raises(AssertionError, match="an engine was asked for"):
        StartPool(NoEngine(), [0, 0], [0, 0], pos)
    with pytest.raises(ValueError, match="expected a VecPushWorld"):
        StartPool(object(), [0, 0], [0, 0], pos)
    with pytest.raises(ValueError, match="engine's npad is 8, not 4"):
        StartPool(_engine(8), [0, 0], [0, 0], pos)
    for bad in ([0, 3], [-1, 0]):
        with pytest.raises(ValueError, match=r"indices into the set \(0 .. 2\)"):
            StartPool(_engine(), bad, [0, 0], pos)
    with pytest.raises(ValueError, match="level must be >= 0"):
        StartPool(_engine(), [0, 1], [0, -1], pos)
    with pytest.raises(ValueError, match="must hold integers"):
        StartPool(_engine(), [0, 1], [0.5, 1.0], pos)
    with pytest.raises(ValueError, match="fewer than 2\\^31"):  # (S >= 2^31: refused by its shape, before anything is made)
        StartPool(NoEngine(), np.broadcast_to(np.int32(0), (1 << 31,)), np.broadcast_to(np.int32(0), (1 << 31,)),
                  np.broadcast_to(np.int8(0), (1 << 31, 4, 2)))
    with pytest.raises(ValueError, match="int32 tensors"):
        group_entries(torch.zeros(3, dtype=torch.int64), torch.zeros(3, dtype=torch.int32), 2)
    pool = _pool()
    i32, u8 = torch.zeros(3, dtype=torch.int32), torch.zeros(3, dtype=torch.uint8)
    st = torch.zeros((3, 4, 2), dtype=torch.int8)
    for kw, words in ((dict(band="own"), "band must be"), (dict(band=(1,)), "band must be"), (dict(band=(0.5, 2)), "band must be"),
                      (dict(band=(i32, 3)), "band: hi"), (dict(band=(i32, i32.to(torch.int64))), "band: hi"),
                      (dict(keep_initial=1.5), "keep_initial"), (dict(keep_initial=-0.1), "keep_initial"),
                      (dict(keep_initial=True), "keep_initial"), (dict(mask=i32), "mask"),
                      (dict(terminated=i32), "terminated"), (dict(truncated=torch.zeros(4, dtype=torch.uint8)), "truncated"),
                      (dict(counter=u8), "counter"), (dict(out=(i32,)), "out must be"), (dict(out=(i32, u8)), "out: level")):
        with pytest.raises(ValueError, match=words):
            pool.draw(i32, st, i32.clone(), **kw)
    with pytest.raises(ValueError, match="puzzle_id"):
        pool.draw(i32.to(torch.int64), st, i32)
    with pytest.raises(ValueError, match="pos must be"):
        pool.draw(i32, torch.zeros((3, 8, 2), dtype=torch.int8), i32)
    with pytest.raises(ValueError, match="steps"):
        pool.draw(i32, st, u8)
    with pytest.raises(AttributeError, match="handle"):  # good arguments do reach the library
        pool.draw(i32, st, i32.clone(), terminated=u8, truncated=u8.bool(), band=(i32, i32), mask=u8.bool(), keep_initial=0.5)
    with pytest.raises(ValueError, match="needs statistics"):
        pool.update_bands()
    stats = torch.zeros((3, 4), dtype=torch.int64)
    for kw, words in ((dict(up=1.5), "up must be"), (dict(down=-1), "down must be"), (dict(up=0.1, down=0.2), "up_q16 must not be below"),
                      (dict(step=0), "step"), (dict(min_episodes=0), "min_episodes"), (dict(width=-1), "width"),
                      (dict(hi_min=1.5), "hi_min")):
        with pytest.raises(ValueError, match=words):
            pool.update_bands(stats, **kw)
    with pytest.raises(ValueError, match="stats"):
        pool.update_bands(stats[:2])
    with pytest.raises(AttributeError, match="handle"):
        pool.update_bands(stats)
    assert keep_to_q16(0) == 0 and keep_to_q16(1.0) == 65536 and keep_to_q16(0.5) == 32768


def test_environment_refusals_come_first():
    pool = _pool()
    # (an empty set of puzzles would be the next complaint: these come before anything is parsed or an engine is made)
    with pytest.raises(ValueError, match="start_pool needs autoreset=True"):
        VecPushWorld([], 4, start_pool=pool)
    with pytest.raises(ValueError, match="start_pool must be a start_pool.StartPool"):
        VecPushWorld([], 4, autoreset=True, start_pool=object())
    with pytest.raises(ValueError, match="need a start_pool"):
        VecPushWorld([], 4, autoreset=True, start_band=(1, 2))
    with pytest.raises(ValueError, match="need a start_pool"):
        VecPushWorld([], 4, autoreset=True, start_keep_initial=0.5)
    with pytest.raises(ValueError, match="band must be"):
        VecPushWorld([], 4, autoreset=True, start_pool=pool, start_band="mine")
    with pytest.raises(ValueError, match="keep_initial must be"):
        VecPushWorld([], 4, autoreset=True, start_pool=pool, start_keep_initial=2)
    with pytest.raises(ValueError, match="No PushWorld puzzles given"):  # well-formed options get as far as the puzzles
        VecPushWorld([], 4, autoreset=True, start_pool=pool, start_band=(1, None), start_keep_initial=0.25, device=0)
    assert check_start_options(None, "pool", 0.0, False) is None
    assert check_start_options(pool, (2, None), 0.5, True) == ("scalar", 2, -1, 32768)
    for cls in (PushWorldVectorEnv, PushWorldDmVectorEnv, PushWorldPushVectorEnv, PushWorldPushDmVectorEnv):
        with pytest.raises(ValueError, match="start_update_every needs a start_pool"):
            cls([], 4, start_update_every=4)
        for bad in (0, -3, 2.5, True, "4", {"min_episodes": 4}):
            with pytest.raises(ValueError, match="start_update_every must be"):
                cls([], 4, start_pool=pool, start_update_every=bad)
        with pytest.raises(ValueError, match="start_pool must be a start_pool.StartPool"):
            cls([], 4, start_pool="tables")
        with pytest.raises(ValueError, match="need a start_pool"):
            cls([], 4, start_keep_initial=0.5)
    vec = VecPushWorld.__new__(VecPushWorld)
    assert vec.start_pool is None and vec._call_pool_arm is None and vec._call_pool_draw is None
    vec.start_pool = pool  # a pool is set: the resets inside a rollout or a mailbox would draw nothing
    with pytest.raises(ValueError, match=r"rollout\(\) is not available with a start_pool"):
        vec.rollout(None)
    with pytest.raises(ValueError, match=r"mailbox\(\) is not available with a start_pool"):
        vec.mailbox()
    # a pool of another set size or layout is refused by the environment it is given to
    vec = VecPushWorld.__new__(VecPushWorld)
    vec.num_envs, vec.num_puzzles, vec.device, vec.engine = 4, 5, torch.device("cpu"), _engine()
    with pytest.raises(ValueError, match="the start pool covers 3 puzzles with npad 4"):
        vec._bind_start_pool(pool, "pool", "pool", 0, -1, 0)
    vec.num_puzzles, vec.engine = 3, _engine(8)
    with pytest.raises(ValueError, match="this environment 3 with npad 8"):
        vec._bind_start_pool(pool, "pool", "pool", 0, -1, 0)


# ---- the restatement against figures worked out by hand -------------------------------------------------------------------
def _splitmix(seed, env, ctr):
    z = (seed + 0x9E3779B97F4A7C15 * (env + 1) + 0xD1B54A32D192ED03 * ctr) & SR.MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & SR.MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & SR.MASK64
    return z ^ (z >> 31)


def _hand_pool():
    # puzzle 0: entries 1 (level 0) and 0 (level 1); puzzle 1: none; puzzle 2: entries 3 (level 0), 2, 4, 5 (level 3)
    pos = np.zeros((6, 4, 2), np.int8)
    pos[:, 0, 0] = 10 + np.arange(6)
    return SR.Pool([0, 0, 2, 2, 2, 2], [1, 0, 3, 0, 3, 3], pos, 3)


def _state(n):
    return dict(pos=np.full((n, 4, 2), 7, np.int8), steps=np.full(n, 9, np.int32), terminated=np.ones(n, np.uint8),
                truncated=np.ones(n, np.uint8), counter=np.zeros(n, np.int64), entry=np.full(n, -5, np.int32),
                level=np.full(n, -5, np.int32))


def test_draws_by_hand():
    pool = _hand_pool()
    assert (pool.order, pool.max_level, pool.lvl_off, pool.start) == ([1, 0, 3, 2, 4, 5], [1, -1, 3], [0, 3, 4],
                                                                      [0, 1, 2, 2, 2, 3, 3, 3, 6])
    assert SR.mix64(42 ^ SR.K_DRAW, 3, 1) == _splitmix(42 ^ SR.K_DRAW, 3, 1)
    seed = 42
    # env 0: puzzle 0, band (1, 1) -> the one entry of level 1, whatever the word
    # env 1: puzzle 1 has no entries: outs -1, nothing else
    # env 2: puzzle 2, band (3, 3) -> one of 2, 4, 5 by the word
    # env 3: puzzle 2, band (1, 2): both levels empty -> outs -1, counter stays
    # env 4: masked out: nothing at all
    # env 5: puzzle 7 is outside the set
    ids = [0, 1, 2, 2, 2, 7]
    lo_n, hi_n = [1, 0, 3, 1, 0, 0], [1, 5, 3, 2, 3, 3]
    s = _state(6)
    SR.draw(pool, ids, seed=seed, mask=[1, 1, 1, 1, 0, 1], lo_n=lo_n, hi_n=hi_n, **s)
    u = (_splitmix(seed ^ SR.K_DRAW, 2, 1) * 3) >> 64
    e2 = [2, 4, 5][u]
    assert s["entry"].tolist() == [0, -1, e2, -1, -5, -1] and s["level"].tolist() == [1, -1, 3, -1, -5, -1]
    assert s["counter"].tolist() == [1, 0, 1, 0, 0, 0]
    assert s["pos"][:, 0, 0].tolist() == [10, 7, 10 + e2, 7, 7, 7] and s["pos"][0, 1:].tolist() == [[0, 0]] * 3
    assert s["steps"].tolist() == [0, 9, 0, 9, 9, 9] and s["terminated"].tolist() == s["truncated"].tolist() == [0, 1, 0, 1, 1, 1]
    # the clamps: hi < lo -> hi = lo; hi beyond the maximum; lo < 0; hi = -1 -> everything of the puzzle
    s = _state(4)
    SR.draw(pool, [2, 2, 2, 0], seed=seed, lo_n=[3, 0, -4, 0], hi_n=[0, 99, 0, -1], **s)
    words = [_splitmix(seed ^ SR.K_DRAW, i, 1) for i in range(4)]
    assert s["entry"].tolist() == [[2, 4, 5][(words[0] * 3) >> 64], [3, 2, 4, 5][(words[1] * 4) >> 64], 3,
                                   [1, 0][(words[3] * 2) >> 64]]
    # a second draw uses count 2; the per-puzzle band and the scalars
    SR.draw(pool, [2, 2, 2, 0], seed=seed, band=[[0, 0], [0, 0], [3, -1]], **s)
    assert s["counter"].tolist() == [2, 2, 2, 2] and s["entry"][3] == 1
    assert s["entry"][:3].tolist() == [[2, 4, 5][(_splitmix(seed ^ SR.K_DRAW, i, 2) * 3) >> 64] for i in range(3)]
    SR.draw(pool, [2, 2, 2, 0], seed=seed, lo=0, hi=0, **s)
    assert s["entry"].tolist() == [3, 3, 3, 1] and s["level"].tolist() == [0, 0, 0, 0] and s["counter"].tolist() == [3] * 4
    # keep_q16: 65536 keeps always (the counter still advances), and at 32768 the top 16 bits of the keep word decide
    s = _state(3)
    SR.draw(pool, [0, 2, 2], seed=seed, keep_q16=65536, **s)
    assert s["entry"].tolist() == [-1] * 3 and s["counter"].tolist() == [1] * 3 and s["pos"].min() == 7 and s["steps"].tolist() == [9] * 3
    SR.draw(pool, [0, 2, 2], seed=seed, keep_q16=32768, **s)
    kept = [(_splitmix(seed ^ SR.K_KEEP, i, 2) >> 48) < 32768 for i in range(3)]
    assert [e == -1 for e in s["entry"].tolist()] == kept
    assert SR.arm([0, 1, 0, 0xFF, 0], [0, 0, 1, 0xFF, 0]).tolist() == [0, 1, 1, 1, 0]


def test_band_moves_by_hand():
    max_level = [5, 5, 5, -1, 5, 2, 5]
    stats = [[40, 32, 0, 0], [40, 7, 0, 0], [31, 31, 0, 0], [99, 99, 0, 0], [40, 20, 0, 0], [40, 40, 0, 0], [50, 8, 1, 1]]
    base = [[0] * 4 for _ in range(7)]
    base[6] = [10, 0, 0, 0]
    band = [[1, 1], [1, 3], [1, 1], [0, 0], [2, -1], [1, 2], [1, 1]]
    delta = SR.update_bands(max_level, stats, base, band, min_episodes=32, up_q16=52429, down_q16=13107)
    # 0: 32 / 40 = 0.8 and 32 * 65536 = 2097152 >= 52429 * 40 = 2097160?  No: 0.8 in Q16 rounds UP, so exactly 80 % is not enough
    assert 32 * 65536 < 52429 * 40 and band[0] == [1, 1] and delta[0] == 0 and base[0] == stats[0]
    # 1: 7 / 40 = 0.175 < 0.2 -> down by one; 2: 31 episodes, below min_episodes: nothing moves, the base stays
    assert band[1] == [1, 2] and delta[1] == -1 and band[2] == [1, 1] and base[2] == [0] * 4 and delta[2] is None
    # 3: no entries; 4: in between, hi -1 is written as the maximum; 5: up at the maximum stays; 6: the window 40 / 8 is exactly 0.2: not below
    assert delta[3] is None and base[3] == [0] * 4 and band[4] == [2, 5] and delta[4] == 0
    assert band[5] == [1, 2] and delta[5] == 0 and 8 * 65536 >= 13107 * 40 and band[6] == [1, 1] and base[6] == stats[6]
    # exact thresholds in Q16: up = 49152 (0.75): 30 of 40 moves up; width 2 drags lo along; step 3 is cut at the maximum
    band = [[1, 4]]
    assert SR.update_bands([5], [[40, 30, 0, 0]], [[0] * 4], band, up_q16=49152, down_q16=16384, step=3, width=2) == [1]
    assert band == [[4, 5]]
    # down: 9 of 40 < 0.25, step 3 from 3 is cut at hi_min 2; lo_min holds lo; the second window needs 32 NEW episodes
    band, base = [[1, 3]], [[0] * 4]
    assert SR.update_bands([5], [[40, 9, 0, 0]], base, band, up_q16=49152, down_q16=16384, step=3, width=4, hi_min=2) == [-1]
    assert band == [[1, 2]] and base == [[40, 9, 0, 0]]
    assert SR.update_bands([5], [[71, 40, 0, 0]], base, band, up_q16=49152, down_q16=16384) == [None] and band == [[1, 2]]
    assert SR.update_bands([5], [[72, 41, 0, 0]], base, band, up_q16=49152, down_q16=16384) == [1] and band == [[1, 3]]
    # a negative difference counts as nothing; more solved than ended counts as all solved; big counts are shifted alike
    assert SR.update_bands([5], [[5, 5, 0, 0]], [[9, 0, 0, 0]], [[1, 1]], min_episodes=1) == [None]
    band = [[1, 1]]
    assert SR.update_bands([5], [[40, 90, 0, 0]], [[0] * 4], band) == [1] and band == [[1, 2]]
    band = [[1, 1]]
    assert SR.update_bands([5], [[1 << 40, (1 << 40) - (1 << 37), 0, 0]], [[0] * 4], band) == [1] and band == [[1, 2]]

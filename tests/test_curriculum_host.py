"""Host side of the statistics per puzzle, the sampling weights and the weighted draw (``pw_episode_stats`` /
``pw_curriculum_update`` / ``pw_resample_weighted``): the header and ``SIGNATURES``, the argument checks that
return before anything touches a device, the wrappers' checks that come before an engine is asked for, and the restatement
(tests/curriculum_restatement.py) against weights and draws worked out by hand."""
import ctypes
import os

import numpy as np
import pytest
import torch

import curriculum_restatement as CR
from pushworld_amd import _capi
from pushworld_amd.curriculum import Curriculum, EpisodeStats, floor_to_q16, stats_tuple
from pushworld_amd.vec_env import VecPushWorld
from pushworld_amd.vector_env import (PushWorldDmVectorEnv, PushWorldPushDmVectorEnv, PushWorldPushVectorEnv,
                                      PushWorldVectorEnv)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p(4096)  # a stand-in for an engine or a buffer: every check below returns before anything is read through it
NAMES = ("pw_episode_stats", "pw_curriculum_update", "pw_resample_weighted")


def test_header_and_signatures():
    with open(os.path.join(ROOT, "include", "pushworld_amd.h")) as f:
        header = f.read()
    for name in NAMES:
        assert f"int {name}(PwEngine* e," in header and name in _capi.SIGNATURES and hasattr(_capi.lib, name)
    assert "#define PW_EPISODE_STATS 4 " in header and _capi.EPISODE_STATS == 4
    for name, value in _capi.CURRICULUM_MODES.items():
        assert f"#define PW_CURRICULUM_{name.upper()} {value}\n" in header
    assert (CR.UNIFORM, CR.FAILURE, CR.FRONTIER, CR.GIVEN) == tuple(_capi.CURRICULUM_MODES.values()) == (0, 1, 2, 3)
    assert "#define PW_OPT_RESAMPLE_FENCE 55 " in header and _capi.OPTIONS["resample_fence"] == 55
    assert "#define PW_OPT_STATS_LDS_PUZZLES 56 " in header and _capi.OPTIONS["stats_lds_puzzles"] == 56
    assert "#define PW_OPT_STATS_GROUPS 57 " in header and _capi.OPTIONS["stats_groups"] == 57
    assert all(list(_capi.OPTIONS.values()).count(k) == 1 for k in (55, 56, 57))
    assert _capi.lib.pw_abi_version() == _capi.ABI_VERSION == 4


def _refused(name, args, words):
    assert getattr(_capi.lib, name)(*args) == _capi.PW_EINVAL, (name, words)
    msg = _capi.last_error()
    assert name in msg and words in msg, (name, words, msg)


def test_episode_stats_argument_checks():
    for args, words in (((None, P, P, P, P, P, 4, None), "null engine"),
                        ((P, None, P, P, P, P, 4, None), "null puzzle_id"),
                        ((P, P, None, P, P, P, 4, None), "null steps"),
                        ((P, P, P, None, P, P, 4, None), "null terminated"),
                        ((P, P, P, P, None, P, 4, None), "null truncated"),
                        ((P, P, P, P, P, None, 4, None), "null stats"),
                        ((P, P, P, P, P, P, -1, None), "batch"),
                        ((P, P, P, P, P, P, -(1 << 31), None), "batch")):
        _refused("pw_episode_stats", args, words)


def test_curriculum_update_argument_checks():
    for args, words in (((None, 2, P, None, None, 0, P, P, None), "null engine"),
                        ((P, -1, P, None, None, 0, P, P, None), "unknown mode"),
                        ((P, 4, P, None, P, 0, P, P, None), "unknown mode"),
                        ((P, 1 << 30, P, None, P, 0, P, P, None), "unknown mode"),
                        ((P, CR.FAILURE, None, None, None, 0, P, P, None), "null stats"),
                        ((P, CR.FRONTIER, None, P, None, 0, P, P, None), "null stats"),
                        ((P, CR.GIVEN, P, None, None, 0, P, P, None), "null given"),
                        ((P, CR.GIVEN, None, None, None, 0, None, P, None), "null given"),
                        ((P, CR.UNIFORM, P, None, None, 0, P, None, None), "null cdf"),
                        ((P, CR.FRONTIER, P, P, None, 655, None, None, None), "null cdf"),
                        ((P, CR.GIVEN, P, None, P, 0, P, None, None), "null cdf")):
        _refused("pw_curriculum_update", args, words)


def test_resample_weighted_argument_checks():
    for args, words in (((None, P, P, P, P, 1, P, 4, None), "null engine"),
                        ((P, None, P, P, P, 1, P, 4, None), "null puzzle_id"),
                        ((P, P, None, None, None, 1, P, 4, None), "null cdf"),
                        ((P, P, P, P, P, 1, None, 4, None), "null episode"),
                        ((P, P, None, None, P, 1, P, -1, None), "batch"),
                        ((P, P, P, P, P, 1, P, -7, None), "batch")):
        _refused("pw_resample_weighted", args, words)


class _Set:
    def __len__(self):
        return 5


def _engine():
    """An ``Engine`` without a handle: a call that gets past the wrapper's checks fails with AttributeError."""
    e = _capi.Engine.__new__(_capi.Engine)
    e.pset = _Set()
    return e


def test_engine_wrapper_checks():
    e = _engine()
    i32, u8 = torch.zeros(3, dtype=torch.int32), torch.zeros(3, dtype=torch.uint8)
    stats = torch.zeros((5, 4), dtype=torch.int64)
    cdf, w = torch.zeros(5, dtype=torch.uint64), torch.zeros(5, dtype=torch.uint32)
    for args, words in (((i32.to(torch.int64), i32, u8, u8, stats), "puzzle_id"),
                        ((i32, torch.zeros(4, dtype=torch.int32), u8, u8, stats), "steps"),
                        ((i32, i32, u8.to(torch.bool), u8, stats), "terminated"),
                        ((i32, i32, u8, torch.zeros(6, dtype=torch.uint8)[::2], stats), "truncated"),
                        ((i32, i32, u8, u8, torch.zeros((4, 4), dtype=torch.int64)), "stats"),
                        ((i32, i32, u8, u8, torch.zeros((5, 4), dtype=torch.int32)), "stats"),
                        ((i32, i32, u8, u8, None), "stats")):
        for call in (e.episode_stats, e.bind_episode_stats):
            with pytest.raises(ValueError, match="pw_episode_stats: " + words):
                call(*args)
    with pytest.raises(AttributeError, match="handle"):  # good arguments do reach the library
        e.episode_stats(i32, i32, u8, u8, stats)
    for kw, words in ((dict(mode="hardest", stats=stats, cdf=cdf), "unknown mode"),
                      (dict(mode=7, stats=stats, cdf=cdf), "unknown mode"),
                      (dict(mode="frontier", stats=None, cdf=cdf), "stats"),
                      (dict(mode="failure", stats=stats.to(torch.int32), cdf=cdf), "stats"),
                      (dict(mode="frontier", stats=stats, cdf=cdf, base=stats[:4]), "base"),
                      (dict(mode="given", stats=None, cdf=cdf), "given"),
                      (dict(mode="given", stats=None, cdf=cdf, given=w.to(torch.int32)), "given"),
                      (dict(mode="uniform", stats=None, cdf=cdf.to(torch.int64)), "cdf"),
                      (dict(mode="uniform", stats=None, cdf=torch.zeros(6, dtype=torch.uint64)), "cdf"),
                      (dict(mode="uniform", stats=None, cdf=cdf, weights=w.to(torch.int64)), "weights"),
                      (dict(mode="uniform", stats=None, cdf=cdf, floor_q16=-1), "floor_q16"),
                      (dict(mode="uniform", stats=None, cdf=cdf, floor_q16=1 << 32), "floor_q16")):
        with pytest.raises(ValueError, match="pw_curriculum_update: .*" + words):
            e.curriculum_update(**kw)
    with pytest.raises(AttributeError, match="handle"):
        e.curriculum_update("given", None, cdf, weights=w, given=w, floor_q16=(1 << 32) - 1)
    for args, kw, words in (((i32.to(torch.int16), i32, 0, cdf), {}, "puzzle_id"),
                            ((i32, torch.zeros(2, dtype=torch.int32), 0, cdf), {}, "episode"),
                            ((i32, i32, 0, cdf[:4]), {}, "cdf"),
                            ((i32, i32, 0, cdf.to(torch.int64)), {}, "cdf"),
                            ((i32, i32, 0, cdf), dict(terminated=u8.to(torch.int8)), "terminated"),
                            ((i32, i32, 0, cdf), dict(truncated=torch.zeros(4, dtype=torch.uint8)), "truncated")):
        with pytest.raises(ValueError, match="pw_resample_weighted: " + words):
            e.resample_weighted(*args, **kw)
    with pytest.raises(ValueError, match="pw_resample_weighted: terminated"):
        e.bind_resample_weighted(i32, i32, cdf, None, u8)
    with pytest.raises(AttributeError, match="handle"):
        e.resample_weighted(i32, i32, -1, cdf, truncated=u8)


def test_environment_refusals_come_first():
    # (an empty pool would be the next complaint: these come before anything is parsed or an engine is made)
    with pytest.raises(ValueError, match="episode_stats needs autoreset"):
        VecPushWorld([], 4, episode_stats=True, autoreset=False)
    with pytest.raises(ValueError, match="episode_stats needs autoreset"):
        VecPushWorld([], 4, resample=True, curriculum="frontier")  # (a curriculum implies the statistics)
    with pytest.raises(ValueError, match="curriculum needs resample=True"):
        VecPushWorld([], 4, autoreset=True, curriculum="frontier")
    with pytest.raises(ValueError, match="curriculum needs resample=True"):
        VecPushWorld([], 4, autoreset=True, resample=[0, 1], curriculum="failure")
    with pytest.raises(ValueError, match="curriculum must be one of uniform, failure, frontier, given"):
        VecPushWorld([], 4, autoreset=True, resample=True, curriculum="hardest")
    with pytest.raises(ValueError, match="No PushWorld puzzles given"):  # well-formed options get as far as the pool
        VecPushWorld([], 4, autoreset=True, resample=True, curriculum="frontier", device=0)
    for cls in (PushWorldVectorEnv, PushWorldDmVectorEnv, PushWorldPushVectorEnv, PushWorldPushDmVectorEnv):
        with pytest.raises(ValueError, match="curriculum_update_every needs a curriculum"):
            cls([], 4, curriculum_update_every=16)
        for bad in (0, -3, 2.5, True, "16"):
            with pytest.raises(ValueError, match="curriculum_update_every must be"):
                cls([], 4, curriculum="frontier", curriculum_update_every=bad)
    vec = VecPushWorld.__new__(VecPushWorld)
    assert vec.stats is None and vec.curriculum is None
    with pytest.raises(RuntimeError, match="keeps no statistics"):
        vec.puzzle_stats()
    vec.stats = object()  # statistics are on: the steps inside a rollout or a mailbox could not be observed
    with pytest.raises(RuntimeError, match=r"rollout\(\) is not available while statistics"):
        vec.rollout(None)
    with pytest.raises(RuntimeError, match=r"mailbox\(\) is not available while statistics"):
        vec.mailbox()


def test_curriculum_object_checks():
    class NoEngine:
        @property
        def engine(self):
            raise AssertionError("an engine was asked for")

    with pytest.raises(ValueError, match="curriculum mode must be one of"):
        Curriculum(NoEngine(), mode="hardest")
    for bad in (-0.1, 65536.0, "1", None, True):
        with pytest.raises(ValueError, match="floor must be"):
            Curriculum(NoEngine(), floor=bad)
    with pytest.raises(AssertionError, match="an engine was asked for"):
        Curriculum(NoEngine(), mode="failure", floor=0)
    with pytest.raises(ValueError, match="expected a VecPushWorld"):
        EpisodeStats(object())
    assert floor_to_q16(0) == 0 and floor_to_q16(0.01) == 655 and floor_to_q16(1) == 65536 and floor_to_q16(0.5) == 32768
    cur = Curriculum.__new__(Curriculum)
    cur.mode, cur.stats, cur.window, cur.num_puzzles, cur.floor_q16 = "frontier", None, False, 5, 0
    with pytest.raises(ValueError, match="needs statistics"):
        cur.update()
    with pytest.raises(ValueError, match="belong to mode 'given'"):
        cur.update(stats=torch.zeros((5, 4), dtype=torch.int64), given=[1, 2, 3, 4, 5])
    cur.mode = "given"
    with pytest.raises(ValueError, match="needs the weights"):
        cur.update()
    for bad in ([1, 2, 3], [1, 2, 3, 4, -5], [1, 2, 3, 4, 1 << 32], [0.5] * 5):
        with pytest.raises(ValueError, match="one integer weight"):
            cur.update(given=bad)
    block = np.array([[4, 1, 40, 7], [0, 0, 0, 0], [3, 3, 9, 9]], dtype=np.int64)
    st = stats_tuple(block)
    assert st.episodes.tolist() == [4, 0, 3] and st.solved.tolist() == [1, 0, 3] and st.solved_steps.tolist() == [7, 0, 9]
    assert st.success_rate[0] == 0.25 and np.isnan(st.success_rate[1]) and st.success_rate[2] == 1.0
    assert st.mean_steps[0] == 10.0 and np.isnan(st.mean_steps[1]) and st.mean_steps[2] == 3.0


# ---- the restatement against figures worked out by hand ----------------------------------------------------------------------
def test_statistics_by_hand():
    stats = [[0] * 4 for _ in range(3)]
    #            ends:   solved  cut    both   no     refused  refused  id -1  id P   solved
    puzzle_id = [0, 0, 1, 1, 2, 2, -1, 3, 2]
    steps = [7, 20, 5, 3, 9, 4, 6, 6, 11]
    term = [1, 0, 1, 0, 0xFF, 0xFF, 1, 1, 1]
    trunc = [0, 1, 1, 0, 0xFF, 0, 0, 1, 0]
    CR.episode_stats(stats, puzzle_id, steps, term, trunc)
    assert stats == [[2, 1, 27, 7], [1, 1, 5, 5], [1, 1, 11, 11]]
    CR.episode_stats(stats, puzzle_id, steps, term, trunc)  # two calls accumulate
    assert stats == [[4, 2, 54, 14], [2, 2, 10, 10], [2, 2, 22, 22]]


def test_weights_by_hand():
    w = CR.weight
    # never seen
    assert (w(CR.UNIFORM, 0, 0), w(CR.FAILURE, 0, 0), w(CR.FRONTIER, 0, 0)) == (65536, 32768, 65536)
    # always solved: 65536 * 1 / 12 and 262144 * 11 * 1 / 144
    assert (w(CR.UNIFORM, 10, 10), w(CR.FAILURE, 10, 10), w(CR.FRONTIER, 10, 10)) == (65536, 5461, 20024)
    # never solved: 65536 * 11 / 12, and the frontier weight is symmetric
    assert (w(CR.FAILURE, 10, 0), w(CR.FRONTIER, 10, 0)) == (60074, 20024)
    # half solved: 65536 * 6 / 12 and 262144 * 36 / 144 -- the frontier's largest weight
    assert (w(CR.FAILURE, 10, 5), w(CR.FRONTIER, 10, 5)) == (32768, 65536)
    assert w(CR.FRONTIER, 11, 5) == w(CR.FRONTIER, 11, 6) == (262144 * 6 * 7) // 169 == 65148
    # n = 2^20 - 1 is not shifted: 65536 * 2^20 / (2^20 + 1) and 2^38 / (2^20 + 1)^2 < 1
    n = (1 << 20) - 1
    assert (w(CR.FAILURE, n, 0), w(CR.FRONTIER, n, 0), w(CR.FAILURE, n, n)) == (65535, 0, 0)
    assert w(CR.FRONTIER, n, n // 2) == (262144 * (1 << 19) * ((1 << 19) + 1)) // (((1 << 20) + 1) ** 2) == 65535
    # n = 2^20 is shifted by one: n' = 2^19
    n = 1 << 20
    assert (w(CR.FAILURE, n, 0), w(CR.FAILURE, n, n)) == (65535, 0)
    assert w(CR.FRONTIER, n, n // 2) == 65536  # s' = f' = 2^18: (2^18 + 1)^2 / (2^19 + 2)^2 = 1 / 4 exactly
    assert w(CR.FRONTIER, n, 1) == w(CR.FRONTIER, n, 0) == 0  # one success is shifted out
    assert w(CR.FAILURE, n, 2) == (65536 * (1 << 19)) // ((1 << 19) + 2) == 65535
    assert w(CR.FAILURE, n, n // 2) == (65536 * ((1 << 18) + 1)) // ((1 << 19) + 2) == 32768
    # n = 2^40 is shifted by 21: n' = 2^19 again, and 2^21 - 1 successes are shifted out
    n = 1 << 40
    assert (w(CR.FRONTIER, n, n // 2), w(CR.FAILURE, n, n // 2)) == (65536, 32768)
    assert w(CR.FAILURE, n, (1 << 21) - 1) == 65535 and w(CR.FAILURE, n, 1 << 21) == (65536 * (1 << 19)) // ((1 << 19) + 2)
    assert w(CR.FRONTIER, n, (1 << 21) - 1) == 0
    # three quarters solved: s' = 3 * 2^17, f' = 2^17
    assert w(CR.FRONTIER, n, 3 << 38) == (262144 * (3 * (1 << 17) + 1) * ((1 << 17) + 1)) // (((1 << 19) + 2) ** 2) == 49152
    # negative differences count as zero; more solved than ended counts as all solved
    assert w(CR.FAILURE, -5, -7) == 32768 and w(CR.FRONTIER, 10, 12) == w(CR.FRONTIER, 10, 10)
    # the floor
    assert w(CR.FAILURE, 1 << 20, 1 << 20, floor_q16=655) == 655 and w(CR.FAILURE, 10, 5, floor_q16=655) == 32768
    assert w(CR.UNIFORM, 0, 0, floor_q16=70000) == 70000 and w(CR.GIVEN, 0, 0, given=0, floor_q16=1) == 1
    assert w(CR.GIVEN, 5, 5, given=(1 << 32) - 1) == (1 << 32) - 1 and w(CR.GIVEN, 5, 5, given=0) == 0


def test_update_by_hand():
    stats = [[10, 10, 0, 0], [10, 0, 0, 0], [0, 0, 0, 0], [10, 5, 0, 0]]
    assert CR.curriculum_update(CR.FAILURE, stats) == ([5461, 60074, 32768, 32768], [5461, 65535, 98303, 131071])
    assert CR.curriculum_update(CR.FRONTIER, stats) == ([20024, 20024, 65536, 65536], [20024, 40048, 105584, 171120])
    assert CR.curriculum_update(CR.FRONTIER, stats, floor_q16=30000)[0] == [30000, 30000, 65536, 65536]
    base = [[4, 4, 0, 0], [10, 0, 0, 0], [3, 1, 0, 0], [0, 0, 0, 0]]  # the window: 6 of 6, nothing, negative, 5 of 10
    assert CR.curriculum_update(CR.FAILURE, stats, base=base)[0] == [65536 // 8, 32768, 32768, 32768]
    assert CR.curriculum_update(CR.UNIFORM, None, num_puzzles=3) == ([65536] * 3, [65536, 131072, 196608])
    given = [0, 5, 0, 0, 7, 0]
    assert CR.curriculum_update(CR.GIVEN, None, given=given, num_puzzles=6) == (given, [0, 5, 5, 5, 12, 12])
    big = [(1 << 32) - 1] * 4096
    assert CR.curriculum_update(CR.GIVEN, None, given=big, num_puzzles=4096)[1][-1] == (1 << 44) - 4096


def test_draw_by_hand():
    top = (1 << 64) - 1
    # no weight anywhere: floor(r P / 2^64)
    assert [CR.draw([0, 0, 0], r) for r in (0, (1 << 64) // 3, (1 << 64) // 3 + 1, top)] == [0, 0, 1, 2]
    # weights 0 5 0 0 7 0: t = floor(12 r / 2^64); t = 0 .. 4 draws puzzle 1, t = 5 .. 11 puzzle 4
    cdf = [0, 5, 5, 5, 12, 12]
    edge = -((-5 << 64) // 12)  # the smallest r with t = 5
    assert (edge * 12) >> 64 == 5 and ((edge - 1) * 12) >> 64 == 4
    assert [CR.draw(cdf, r) for r in (0, edge - 1, edge, top)] == [1, 1, 4, 4]
    # puzzles of weight zero at the first, a middle and the last index are never drawn
    rng = np.random.default_rng(5)
    words = [int(x) for x in rng.integers(0, 1 << 64, size=4000, dtype=np.uint64)]
    words += [-((-t << 64) // 12) + d for t in range(1, 12) for d in (-1, 0)]
    drawn = [CR.draw(cdf, r) for r in words]
    assert set(drawn) == {1, 4} and 0.35 < drawn.count(1) / len(drawn) < 0.48
    # a boundary inside the cdf: weights 3 1 -> t = 2 is the last of puzzle 0, t = 3 is puzzle 1
    assert [CR.draw([3, 4], -((-t << 64) // 4)) for t in range(4)] == [0, 0, 0, 1]
    assert CR.draw([9], top) == 0 and CR.draw([0], top) == 0
    # the whole call: only flagged environments move, their episode numbers advance, and the hash is pw_mix64's
    pid, ep = CR.resample_weighted([9, 9, 9, 9], [0, 7, 0xFFFFFFFF, 2], 42, cdf, terminated=[1, 0, 0, 0xFF], truncated=[0, 0, 1, 0])
    assert ep.tolist() == [1, 7, 0, 3] and pid[1] == 9
    assert [int(pid[i]) for i in (0, 2, 3)] == [CR.draw(cdf, CR.mix64(42, i, e)) for i, e in ((0, 1), (2, 0), (3, 3))]
    pid, ep = CR.resample_weighted([9, 9], [0, 0], 42, cdf)
    assert ep.tolist() == [1, 1] and set(pid.tolist()) <= {1, 4}
    z = 42 + 0x9E3779B97F4A7C15 * 3 + 0xD1B54A32D192ED03 * 5
    z &= CR.MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & CR.MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & CR.MASK64
    assert CR.mix64(42, 2, 5) == z ^ (z >> 31)

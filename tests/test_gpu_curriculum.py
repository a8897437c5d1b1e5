"""-m gpu: statistics per puzzle, sampling weights and the weighted draw on the device (pw_episode_stats /
pw_curriculum_update / pw_resample_weighted, curriculum.EpisodeStats / Curriculum, VecPushWorld(episode_stats=, curriculum=),
the facades' curriculum options).  Everything is integer arithmetic, so every comparison is bit for bit against
tests/curriculum_restatement.py and covers every puzzle and every environment."""
import os

import numpy as np
import pytest
import torch

import curriculum_restatement as CR
from pushworld_amd import _capi
from pushworld_amd.curriculum import Curriculum, EpisodeStats
from pushworld_amd.puzzle import PushWorldPuzzle
from pushworld_amd.vec_env import VecPushWorld
from pushworld_amd.vector_env import PushWorldPushVectorEnv, PushWorldVectorEnv

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVEL1 = os.path.join(ROOT, "pushworld_amd", "data", "puzzles", "level1")
CORRIDOR = "G0 . A M0 .\n"
LDS_MAX = 1024  # PW_STATS_LDS_PUZZLES of csrc/pw_curriculum.inc: larger sets can only take the global form of pw_episode_stats
LDS_DEFAULT = 256  # PW_STATS_LDS_DEFAULT: larger sets take the global form unless the option says otherwise
NEVER = 2048    # PW_OPT_STATS_LDS_PUZZLES: the global form for every set
FLOOR = 655     # floor_to_q16(0.01), the default of Curriculum

_ENGINES = {}


def _engine(P, which=0):
    """An engine over ``P`` copies of one small puzzle (made once per session): the three entry points look at the set's size only."""
    if (P, which) not in _ENGINES:
        parsed = PushWorldPuzzle(text=CORRIDOR)._parsed
        _ENGINES[P, which] = _capi.Engine(_capi.PuzzleSet([parsed] * P, 0), max_steps=20, obs_dtype=_capi.OBS_U8)
    return _ENGINES[P, which]


def _dev(arr, dtype):
    return torch.from_numpy(np.ascontiguousarray(arr)).to(dtype).cuda()


def _u64(t):
    """A device tensor of 64-bit words as Python integers."""
    return [int(x) for x in t.cpu().numpy().astype(np.uint64)]


def _rows(t):
    return t.cpu().numpy().astype(np.int64).tolist()


# ---- 1. statistics on hand-made flags ------------------------------------------------------------------------------------------
def _flags(B, P, rng, every=False):
    """Flags that mix 0, 1, 0xFF, truncated-only and both; ids that include -1 and P; step counts up to max_steps."""
    if every:
        term, trunc = np.ones(B, np.uint8), rng.integers(0, 2, B).astype(np.uint8)
    else:
        kind = rng.integers(0, 8, B)  # 0 .. 2 running, 3 solved, 4 cut, 5 both, 6 refused (0xFF in both), 7 refused in terminated
        term = np.select([kind == 3, kind == 5, kind >= 6], [1, 1, 0xFF], 0).astype(np.uint8)
        trunc = np.select([kind == 4, kind == 5, kind == 6], [1, 1, 0xFF], 0).astype(np.uint8)
    pid = rng.integers(0, P, B).astype(np.int32)
    if B >= 8 and not every:
        pid[rng.integers(0, B, max(1, B // 16))] = -1
        pid[rng.integers(0, B, max(1, B // 16))] = P
        pid[0], pid[-1] = P + 7, -(1 << 31)
    steps = rng.integers(0, 21, B).astype(np.int32)
    return pid, steps, term, trunc


@pytest.mark.parametrize("P", [1, 2, 68, LDS_DEFAULT, LDS_DEFAULT + 1, LDS_MAX, LDS_MAX + 1])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 257, 4099])
def test_statistics_on_hand_made_flags(B, P):
    eng = _engine(P)
    rng = np.random.default_rng(1000 * P + B)
    stats = EpisodeStats(eng)
    assert stats.tensor.shape == (P, 4) and stats.tensor.dtype == torch.int64
    want = [[0] * 4 for _ in range(P)]
    # the calls accumulate; the default launch, then the LDS form and the global form (where the set allows the choice), then
    # three workgroups striding over the batch, then one workgroup per 256 environments
    for call, (lds, groups) in enumerate(((0, 0), (LDS_MAX, 0), (NEVER, 0), (LDS_MAX, 3), (NEVER, 3), (LDS_MAX, 1 << 20))):
        eng.set_option("stats_lds_puzzles", lds)
        eng.set_option("stats_groups", groups)
        pid, steps, term, trunc = _flags(B, P, rng)
        stats.add(_dev(pid, torch.int32), _dev(steps, torch.int32), _dev(term, torch.uint8), _dev(trunc, torch.uint8))
        CR.episode_stats(want, pid, steps, term, trunc)
        assert _rows(stats.tensor) == want, call
    eng.set_option("stats_lds_puzzles", 0)
    eng.set_option("stats_groups", 0)
    read = stats.read()
    assert read.episodes.tolist() == [r[0] for r in want] and read.solved_steps.tolist() == [r[3] for r in want]
    snap = stats.snapshot()
    stats.reset()
    assert not stats.tensor.any() and _rows(snap) == want  # reset() zeroes; the snapshot is a copy of its own


@pytest.mark.parametrize("P", [1, LDS_DEFAULT + 1, LDS_MAX + 1])
def test_statistics_worst_contention_and_large_counts(P):
    """Every environment of 4099 ends on one puzzle; then step counts beyond what a workgroup's LDS counters may sum."""
    eng, B = _engine(P), 4099
    rng = np.random.default_rng(P)
    for lds, groups in ((0, 0), (LDS_MAX, 1), (NEVER, 0)):  # (one workgroup for the whole batch: its LDS counters take it all)
        eng.set_option("stats_lds_puzzles", lds)
        eng.set_option("stats_groups", groups)
        stats = EpisodeStats(eng)
        pid, steps, term, trunc = _flags(B, P, rng, every=True)
        pid[:] = P - 1
        stats.add(_dev(pid, torch.int32), _dev(steps, torch.int32), _dev(term, torch.uint8), _dev(trunc, torch.uint8))
        want = CR.episode_stats([[0] * 4 for _ in range(P)], pid, steps, term, trunc)
        assert want[P - 1][:2] == [B, B] and _rows(stats.tensor) == want
        # 65 535 steps is the most an environment adds to a counter in LDS
        big = np.where(rng.integers(0, 2, B) == 1, (1 << 31) - 1, 65535 + rng.integers(0, 2, B)).astype(np.int32)
        stats.add(_dev(pid, torch.int32), _dev(big, torch.int32), _dev(term, torch.uint8), _dev(trunc, torch.uint8))
        CR.episode_stats(want, pid, big, term, trunc)
        assert want[P - 1][2] > 1 << 41 and _rows(stats.tensor) == want
    eng.set_option("stats_lds_puzzles", 0)
    eng.set_option("stats_groups", 0)


# ---- 2. weights and prefix sums ------------------------------------------------------------------------------------------------
def _synthetic(P, rng):
    """Statistics that exercise the shift: episode counts around 2^20, at 2^40 and 2^62, success anywhere between none and all."""
    n = np.array([0, 1, 2, 10, 11, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, (1 << 21) - 1, 1 << 40, (1 << 40) + 12345, 1 << 62],
                 dtype=np.int64)
    n = np.concatenate([n, n, n, rng.integers(0, 1 << 22, 3 * len(n)), rng.integers(0, 50, 4 * len(n))])
    n = np.resize(n, P).astype(np.int64)
    frac = rng.integers(0, 5, P)  # none, a quarter, half, all, anything
    s = np.select([frac == 0, frac == 1, frac == 2, frac == 3], [0 * n, n // 4, n // 2, n],
                  (rng.random(P) * n.astype(np.float64)).astype(np.int64))
    s = np.minimum(s, n)
    return np.stack([n, s, n // 3, s // 5], axis=1).astype(np.int64)


def _check_update(eng, mode, block, base=None, given=None, floor_q16=0):
    P = len(eng.pset)
    weights = torch.full((P,), 7, dtype=torch.int32).cuda().view(torch.uint32)
    cdf = torch.full((P,), 7, dtype=torch.int64).cuda().view(torch.uint64)
    for with_weights in (True, False):
        eng.curriculum_update(mode, None if block is None else _dev(block, torch.int64), cdf,
                              weights=weights if with_weights else None, base=None if base is None else _dev(base, torch.int64),
                              given=None if given is None else _dev(given, torch.uint32), floor_q16=floor_q16)
        want_w, want_cdf = CR.curriculum_update(_capi.CURRICULUM_MODES[mode], block, base=base, given=given, floor_q16=floor_q16,
                                                num_puzzles=P)
        assert _u64(cdf) == want_cdf, (mode, with_weights)
        assert _u64(weights) == want_w, mode
        cdf.view(torch.int64).zero_()
    return want_w


@pytest.mark.parametrize("P", [1, 2, 68, LDS_MAX, LDS_MAX + 1, 4096])
def test_weights_and_cdf_every_mode(P):
    eng = _engine(P)
    rng = np.random.default_rng(77 + P)
    block = _synthetic(P, rng)
    for mode in ("uniform", "failure", "frontier"):
        for floor_q16 in (0, FLOOR, 40000):
            _check_update(eng, mode, block, floor_q16=floor_q16)
    # windows: the difference from a snapshot, negative differences included
    base = block.copy()
    base[::2, :2] //= 2
    base[1::5, 0] += 9
    base[3::7, 1] += 1 << 41
    for mode in ("failure", "frontier"):
        _check_update(eng, mode, block, base=base, floor_q16=FLOOR)
        _check_update(eng, mode, block, base=block)  # an empty window: every puzzle unseen
    # given weights with zeros at the first, a middle and the last index; the floor lifts them
    given = rng.integers(0, 1 << 32, P, dtype=np.uint64).astype(np.uint32)
    given[[0, P // 2, P - 1]] = 0
    given[rng.integers(0, P, P // 3)] = 0
    assert _check_update(eng, "given", None, given=given)[-1] == 0
    assert _check_update(eng, "given", block, given=given, floor_q16=3)[0] == 3
    _check_update(eng, "given", None, given=np.zeros(P, np.uint32))  # total 0


def test_given_weights_near_2_pow_44():
    eng = _engine(4096)
    given = np.full(4096, (1 << 32) - 1, dtype=np.uint32)
    _check_update(eng, "given", None, given=given)
    cur = Curriculum(eng, mode="given", floor=0)
    cur.update(given=given.tolist())
    assert _u64(cur.cdf)[-1] == (1 << 44) - 4096 and cur.updates == 1
    assert np.allclose(cur.probabilities(), 1.0 / 4096)


def test_curriculum_object_windows():
    eng = _engine(68)
    rng = np.random.default_rng(3)
    stats = EpisodeStats(eng)
    whole, window = Curriculum(eng, "failure", floor=0.01, stats=stats), Curriculum(eng, "frontier", window=True, stats=stats)
    assert not whole.cdf.view(torch.int64).any() and np.allclose(whole.probabilities(), 1 / 68)  # before the first update: uniform
    want = [[0] * 4 for _ in range(68)]
    previous = [[0] * 4 for _ in range(68)]
    for k in range(3):
        pid, steps, term, trunc = _flags(4099, 68, rng)
        stats.add(_dev(pid, torch.int32), _dev(steps, torch.int32), _dev(term, torch.uint8), _dev(trunc, torch.uint8))
        CR.episode_stats(want, pid, steps, term, trunc)
        whole.update()
        window.update()
        assert (_u64(whole.weights), _u64(whole.cdf)) == CR.curriculum_update(CR.FAILURE, want, floor_q16=FLOOR), k
        assert (_u64(window.weights), _u64(window.cdf)) == CR.curriculum_update(CR.FRONTIER, want, base=previous, floor_q16=FLOOR), k
        previous = [row[:] for row in want]
    p = whole.probabilities()
    assert abs(p.sum() - 1) < 1e-12 and p.argmax() == int(np.argmax(_u64(whole.weights)))


# ---- 3. draws ------------------------------------------------------------------------------------------------------------------
def _draw_inputs(P, B, rng):
    given = rng.integers(0, 1 << 20, P).astype(np.uint32)
    given[[0, P // 2, P - 1]] = 0
    if P > 8:
        given[rng.integers(0, P, P // 2)] = 0  # long runs of equal cdf entries
        given[P // 3] = (1 << 32) - 1
    else:
        given[P // 2 if P > 2 else 0] = 5
    pid = rng.integers(0, P, B).astype(np.int32)
    ep = rng.integers(0, 1 << 32, B, dtype=np.uint64).astype(np.uint32)
    ep[:4] = 0xFFFFFFFF  # wraps
    kind = rng.integers(0, 40, B)  # a step: about one in twenty ends, a few refused actions
    term = np.select([kind == 0, kind == 2], [1, 0xFF], 0).astype(np.uint8)
    trunc = np.select([kind == 1, kind == 2], [1, 0xFF], 0).astype(np.uint8)
    return given, pid, ep, term, trunc


@pytest.mark.parametrize("P, B", [(4096, 65536), (LDS_MAX + 1, 4099), (300, 4099), (68, 4099), (2, 257), (1, 65)])
def test_draws_against_the_restatement(P, B):
    rng = np.random.default_rng(P)
    given, pid, ep, term, trunc = _draw_inputs(P, B, rng)
    _, cdf_ref = CR.curriculum_update(CR.GIVEN, None, given=given, num_puzzles=P)
    seed = 0x1234567890ABCDEF + P
    results = []
    for which, fence in ((0, 0), (1, 0), (0, 1)):  # a second engine, and the search with the fence in LDS
        eng = _engine(P, which)
        eng.set_option("resample_fence", fence)
        cdf = torch.zeros(P, dtype=torch.int64).cuda().view(torch.uint64)
        eng.curriculum_update("given", None, cdf, given=_dev(given, torch.uint32))
        out = []
        for flags in ((term, trunc), (None, trunc), (term, None), (None, None)):  # a step-like mask ... every environment
            d_pid, d_ep = _dev(pid, torch.int32), _dev(ep.view(np.int32), torch.int32)
            t, u = (None if f is None else _dev(f, torch.uint8) for f in flags)
            eng.resample_weighted(d_pid, d_ep, seed, cdf, terminated=t, truncated=u)
            out.append((d_pid.cpu().numpy(), d_ep.cpu().numpy().view(np.uint32)))
        eng.set_option("resample_fence", 0)
        results.append(out)
    for k, flags in enumerate(((term, trunc), (None, trunc), (term, None), (None, None))):
        want_pid, want_ep = CR.resample_weighted(pid, ep, seed, cdf_ref, *flags)
        for out in results:
            assert (out[k][0] == want_pid).all() and (out[k][1] == want_ep).all(), k
        drawn = want_pid[(want_pid != pid) | (want_ep != ep)]
        assert (given[drawn] != 0).all()  # a puzzle of weight zero is never drawn
    if B == 65536:
        assert len(set(results[0][3][0].tolist())) > P // 3


def test_uniform_fallback_equals_pw_resample():
    P, B = 300, 4099
    rng = np.random.default_rng(9)
    _, pid, ep, term, trunc = _draw_inputs(P, B, rng)
    eng = _engine(P)
    cdf = torch.zeros(P, dtype=torch.int64).cuda().view(torch.uint64)
    for flags in ((term, trunc), (None, None)):
        t, u = (None if f is None else _dev(f, torch.uint8) for f in flags)
        a_pid, a_ep = _dev(pid, torch.int32), _dev(ep.view(np.int32), torch.int32)
        b_pid, b_ep = a_pid.clone(), a_ep.clone()
        eng.resample_weighted(a_pid, a_ep, 77, cdf, terminated=t, truncated=u)
        eng.resample(b_pid, b_ep, 77, terminated=t, truncated=u)
        assert torch.equal(a_pid, b_pid) and torch.equal(a_ep, b_ep)
        want_pid, want_ep = CR.resample_uniform(pid, ep, 77, P, *flags)
        assert (a_pid.cpu().numpy() == want_pid).all() and (a_ep.cpu().numpy().view(np.uint32) == want_ep).all()


# ---- 4. a live run -------------------------------------------------------------------------------------------------------------
def _follow(env, choose, num_steps, every, seed):
    """Steps ``env`` (a facade with ``curriculum="frontier"``) and follows the flags on the host: the statistics, the weights at
    every update and every puzzle id ever drawn are those of the restatement."""
    vec = env.vec
    P, B = vec.num_puzzles, vec.num_envs
    cdf_ref, stats_ref = [0] * P, [[0] * 4 for _ in range(P)]
    env.reset(seed=seed)
    pid_ref, ep_ref = CR.resample_weighted(np.zeros(B, np.int64), np.zeros(B, np.int64), seed, cdf_ref)
    assert (vec.puzzle_id.cpu().numpy() == pid_ref).all()
    vec.counters_reset()
    term, trunc = np.zeros(B, np.uint8), np.zeros(B, np.uint8)
    drawn = B
    for k in range(1, num_steps + 1):
        env.step(choose(env))
        pid_ref, ep_ref = CR.resample_weighted(pid_ref, ep_ref, seed, cdf_ref, term, trunc)
        drawn += int(((term | trunc) != 0).sum())
        term, trunc = vec.terminated.cpu().numpy(), vec.truncated.cpu().numpy()
        assert (vec.puzzle_id.cpu().numpy() == pid_ref).all(), k
        assert (vec.episode.cpu().numpy().view(np.uint32) == ep_ref).all(), k
        assert not (term == 0xFF).any()  # valid actions only
        CR.episode_stats(stats_ref, pid_ref, vec.steps.cpu().numpy(), term, trunc)
        if k % every == 0:
            want_w, cdf_ref = CR.curriculum_update(CR.FRONTIER, stats_ref, floor_q16=FLOOR)
            assert _u64(vec.curriculum.weights) == want_w and _u64(vec.curriculum.cdf) == cdf_ref, k
    assert vec.curriculum.updates == num_steps // every
    assert _rows(vec.stats.tensor) == stats_ref
    got = env.puzzle_stats()
    counters = vec.counters()
    assert got.episodes.sum() == counters["episodes_ended"] > 0 and got.solved.sum() == counters["episodes_solved"]
    assert counters["bad_actions"] == 0 and got.steps.sum() > 0 and (got.solved_steps <= got.steps).all()
    seen = got.episodes > 0
    assert (got.success_rate[seen] == got.solved[seen] / got.episodes[seen]).all() and np.isnan(got.success_rate[~seen]).all()
    return got, drawn


def test_live_run_level1():
    env = PushWorldVectorEnv(LEVEL1, 2048, max_steps=20, observation="cells", seed=0, curriculum="frontier",
                             curriculum_update_every=16)
    assert env.vec.num_puzzles == 68 and env.curriculum is env.vec.curriculum and env.curriculum.mode == "frontier"
    gen = torch.Generator(device=env.vec.device).manual_seed(11)

    def choose(e):
        return torch.randint(0, 4, (2048,), dtype=torch.uint8, device=e.vec.device, generator=gen)

    got, drawn = _follow(env, choose, 200, 16, seed=5)
    assert got.episodes.sum() >= 2048 * 9 and drawn >= got.episodes.sum()  # 200 steps of at most 20 + 1 per episode
    assert (got.episodes > 0).all()
    with pytest.raises(RuntimeError, match="rollout"):
        env.vec.rollout(torch.zeros((2, 2048), dtype=torch.uint8, device=env.vec.device))


def test_live_run_step_push_mask():
    env = PushWorldPushVectorEnv(LEVEL1, 64, max_steps=20, observation="cells", seed=0, curriculum="frontier",
                                 curriculum_update_every=16)
    gen = torch.Generator(device=env.vec.device).manual_seed(12)

    def choose(e):
        mask = e._action_mask().to(torch.float32)
        has = mask.sum(1, keepdim=True) > 0  # (a finished or stuck environment has no choice to make: its action is ignored)
        return torch.multinomial(torch.where(has, mask, torch.ones_like(mask)), 1, generator=gen).squeeze(1)

    got, _ = _follow(env, choose, 64, 16, seed=6)
    env.check_actions()
    assert got.episodes.sum() > 64


def test_step_push_counts_too():
    pool = [PushWorldPuzzle(os.path.join(LEVEL1, name)) for name in sorted(os.listdir(LEVEL1))[:6]]
    vec = VecPushWorld(pool, 96, max_steps=6, observation=None, autoreset=True, resample=True, episode_stats=True)
    assert vec.curriculum is None and vec.stats is not None
    vec.reset()
    vec.counters_reset()
    gen = torch.Generator(device=vec.device).manual_seed(2)
    want = [[0] * 4 for _ in range(6)]
    for _ in range(20):
        mask = vec.push_mask(expanded=True).reshape(96, -1).to(torch.float32)
        has = mask.sum(1, keepdim=True) > 0
        vec.step_push(choice=torch.multinomial(torch.where(has, mask, torch.ones_like(mask)), 1, generator=gen).squeeze(1))
        CR.episode_stats(want, vec.puzzle_id.cpu().numpy(), vec.steps.cpu().numpy(), vec.terminated.cpu().numpy(),
                         vec.truncated.cpu().numpy())
    assert _rows(vec.stats.tensor) == want
    c = vec.counters()
    got = vec.puzzle_stats()
    assert got.episodes.sum() == c["episodes_ended"] > 0 and got.solved.sum() == c["episodes_solved"]


# ---- 5. capture ----------------------------------------------------------------------------------------------------------------
def test_captured_step_stats_and_weighted_draw():
    pool = [PushWorldPuzzle(os.path.join(LEVEL1, name)) for name in sorted(os.listdir(LEVEL1))[:12]]
    B, R = 512, 3
    kw = dict(max_steps=5, observation=None, autoreset=True, resample=True, curriculum="failure", seed=3)
    eager, graphed = VecPushWorld(pool, B, **kw), VecPushWorld(pool, B, **kw)
    dev = eager.device
    gen = torch.Generator(device=dev).manual_seed(8)
    acts = torch.randint(0, 4, (R + 8, B), dtype=torch.uint8, device=dev, generator=gen)
    static_actions = torch.zeros((B,), dtype=torch.uint8, device=dev)
    for vec in (eager, graphed):
        vec.reset()
    s = torch.cuda.Stream(device=dev)  # warm-up on a side stream, then capture ONE step: the draw, the step and the statistics
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        for k in range(8):
            static_actions.copy_(acts[k])
            graphed.step(static_actions)
            graphed.curriculum.update()
    torch.cuda.current_stream(dev).wait_stream(s)
    for k in range(8):
        eager.step(acts[k])
        eager.curriculum.update()
    assert torch.equal(eager.stats.tensor, graphed.stats.tensor) and eager.stats.tensor[:, 0].sum() >= B
    g = torch.cuda.CUDAGraph()
    static_actions.copy_(acts[8])
    with torch.cuda.graph(g):
        graphed.step(static_actions)
        graphed.curriculum.update()
    for r in range(R):  # (the capture itself ran nothing: the first replay is step 8)
        static_actions.copy_(acts[8 + r])
        g.replay()
        eager.step(acts[8 + r])
        eager.curriculum.update()
        for name in ("puzzle_id", "episode", "pos", "steps", "terminated", "truncated"):
            assert torch.equal(getattr(eager, name), getattr(graphed, name)), (name, r)
        assert torch.equal(eager.stats.tensor, graphed.stats.tensor), r
        assert _u64(eager.curriculum.cdf) == _u64(graphed.curriculum.cdf), r
    want = CR.curriculum_update(CR.FAILURE, _rows(eager.stats.tensor), floor_q16=FLOOR)
    assert (_u64(graphed.curriculum.weights), _u64(graphed.curriculum.cdf)) == want and len(set(want[0])) > 1


# ---- 6. defaults untouched -----------------------------------------------------------------------------------------------------
def test_defaults_are_untouched():
    pool = [PushWorldPuzzle(os.path.join(LEVEL1, name)) for name in sorted(os.listdir(LEVEL1))[:9]]
    B, seed = 300, 21
    kw = dict(max_steps=4, pixels_per_cell=3, border_width=1, observation="uint8", autoreset=True, resample=True, seed=seed)
    plain, counted = VecPushWorld(pool, B, **kw), VecPushWorld(pool, B, episode_stats=True, **kw)
    assert plain.stats is None and plain.curriculum is None and plain._call_stats is None and plain._call_resample_weighted is None
    gen = torch.Generator(device=plain.device).manual_seed(4)
    for vec in (plain, counted):
        vec.reset()
    pid, ep = CR.resample_uniform(np.zeros(B, np.int64), np.zeros(B, np.int64), seed, 9)
    term, trunc = np.zeros(B, np.uint8), np.zeros(B, np.uint8)
    ended = 0
    for t in range(12):
        actions = torch.randint(0, 4, (B,), dtype=torch.uint8, device=plain.device, generator=gen)
        plain.step(actions)
        counted.step(actions)
        pid, ep = CR.resample_uniform(pid, ep, seed, 9, term, trunc)
        term, trunc = plain.terminated.cpu().numpy(), plain.truncated.cpu().numpy()
        ended += int(((term | trunc) != 0).sum())
        assert (plain.puzzle_id.cpu().numpy() == pid).all() and (plain.episode.cpu().numpy().view(np.uint32) == ep).all(), t
        for name in ("puzzle_id", "pos", "steps", "terminated", "truncated", "obs"):
            assert torch.equal(getattr(plain, name), getattr(counted, name)), (name, t)
        assert torch.equal(plain.reward.view(torch.int64), counted.reward.view(torch.int64)), t
    assert counted.puzzle_stats().episodes.sum() == counted.counters()["episodes_ended"] == ended >= 2 * B

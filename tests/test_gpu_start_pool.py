"""Start-state pools on the device (csrc/pw_start_pool.inc; start_pool.StartPool; VecPushWorld(start_pool=...) and the vector
facades) against the numpy restatement (tests/start_pool_restatement.py) and against an oracle made of calls
that existed before: a second environment without a pool, the restatement's draw applied with ``set_states``, ``render()``.
Every result is an integer (rewards are compared by their bits): equality is exact."""
import os
import zipfile

import numpy as np
import pytest
import torch

import start_pool_restatement as SR

pytestmark = pytest.mark.gpu

DATA = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pushworld_amd", "data")


def _grid(rows):
    return "\n".join(" ".join(r) for r in rows) + "\n"


def _puzzle_text(n_mov):
    """A puzzle with ``n_mov`` movables (the agent included): engine npad 4 / 8 / 16 / 32 for 3 / 8 / 9 / 17."""
    w = max(4, n_mov - 2)
    rows = [["A", "M0", ".", "G0"] + ["."] * (w - 4), ["."] * w, [f"M{k + 1}" for k in range(n_mov - 2)] + ["."] * (w - n_mov + 2)]
    return _grid(rows)


def _np(t):
    return t.cpu().numpy()


# ---- 1. / 2. the draw against the restatement ----------------------------------------------------------------------------------
class DrawWorld:
    """P = 3 copies of one puzzle: puzzle 0 without entries, puzzle 1 with one level (2), puzzle 2 with levels 0, 1, 3 (2 empty).
    B = 300: one full workgroup and a partial one."""

    B = 300

    def __init__(self, n_mov, npad):
        from pushworld_amd.puzzle import PushWorldPuzzle
        from pushworld_amd.start_pool import StartPool
        from pushworld_amd.vec_env import VecPushWorld

        rng = np.random.default_rng(npad)
        self.vec = VecPushWorld([PushWorldPuzzle(text=_puzzle_text(n_mov))] * 3, 4, observation=None)
        assert self.vec.engine.np == npad
        self.npad, self.dev = npad, self.vec.device
        puzzle = np.array([2, 1, 2, 2, 1, 2, 2, 1, 2, 2, 2], np.int32)
        level = np.array([3, 2, 0, 1, 2, 3, 0, 2, 3, 1, 1], np.int32)
        pos = rng.integers(0, 16, size=(len(puzzle), npad, 2)).astype(np.int8)
        self.pool = StartPool(self.vec, puzzle, level, pos)
        self.ref = SR.Pool(puzzle, level, pos, 3)
        assert self.pool.max_level.tolist() == self.ref.max_level == [-1, 2, 3]
        assert self.pool.order.tolist() == self.ref.order and self.pool.lvl_off.tolist() == self.ref.lvl_off
        assert self.pool.start.view(torch.int32).tolist() == self.ref.start
        # the batch: ids over the set and outside it, arbitrary states, step counts, flags and counts
        self.ids = rng.choice([-1, 0, 1, 2, 2, 2, 3], size=self.B).astype(np.int32)
        self.state = dict(pos=rng.integers(0, 16, size=(self.B, npad, 2)).astype(np.int8),
                          steps=rng.integers(0, 50, size=self.B).astype(np.int32),
                          terminated=rng.integers(0, 2, size=self.B).astype(np.uint8),
                          truncated=rng.choice([0, 1, 0xFF], size=self.B).astype(np.uint8),
                          counter=rng.integers(0, 1 << 32, size=self.B).astype(np.int64),
                          entry=np.full(self.B, -7, np.int32), level=np.full(self.B, -7, np.int32))
        self.state["counter"][:4] = [0, 0xFFFFFFFF, 0xFFFFFFFE, 1]  # the count wraps

    def run(self, state, flags=True, seed=0, mask=None, band=None, scalar=None, env=None, keep_initial=0.0):
        """One draw on the device and one by the restatement from ``state``; returns the state both agree on."""
        dev = self.dev
        t = {k: torch.from_numpy(v.copy()).to(dev) for k, v in state.items() if k != "counter"}
        counter = torch.from_numpy(state["counter"].astype(np.uint32).view(np.int32)).to(dev)
        kw = {}
        if band is not None:
            self.pool.set_band(band[:, 0], band[:, 1])
            kw["band"] = "pool"
        elif scalar is not None:
            kw["band"] = scalar
        else:
            kw["band"] = (torch.from_numpy(env[0]).to(dev), torch.from_numpy(env[1]).to(dev))
        got = self.pool.draw(torch.from_numpy(self.ids).to(dev), t["pos"], t["steps"], t["terminated"] if flags else None,
                             t["truncated"] if flags else None, mask=None if mask is None else torch.from_numpy(mask).to(dev),
                             seed=seed, counter=counter, keep_initial=keep_initial, out=(t["entry"], t["level"]), **kw)
        assert got[0] is t["entry"] and got[1] is t["level"]
        want = {k: v.copy() for k, v in state.items()}
        rkw = dict(band=band) if band is not None else dict(lo_n=env[0], hi_n=env[1]) if env is not None else \
            dict(lo=scalar[0], hi=-1 if scalar[1] is None else scalar[1])
        SR.draw(self.ref, self.ids, want["pos"], want["steps"], want["terminated"] if flags else None,
                want["truncated"] if flags else None, want["counter"], want["entry"], want["level"], seed=seed, mask=mask,
                keep_q16=int(round(keep_initial * 65536)), **rkw)
        for k in t:
            assert (_np(t[k]) == want[k]).all(), k
        assert (_np(counter).view(np.uint32) == want["counter"]).all()
        if not flags:
            assert (want["terminated"] == state["terminated"]).all() and (want["truncated"] == state["truncated"]).all()
        return want


@pytest.fixture(scope="module", params=[(3, 4), (8, 8), (9, 16), (17, 32)], ids=lambda p: f"npad{p[1]}")
def draw_world(request):
    return DrawWorld(*request.param)


def test_draw_every_band_source(draw_world):
    w, rng = draw_world, np.random.default_rng(1)
    drawn = lambda s: s["entry"] >= 0  # noqa: E731
    # the per-puzzle band tensor (puzzle 0 has no entries: its band is never read into a bucket)
    a = w.run(w.state, band=np.array([[0, 0], [0, 5], [1, 3]], np.int32), seed=11)
    assert drawn(a).sum() > 100 and set(a["level"][w.ids == 1]) == {2} and set(a["level"][w.ids == 2]) <= {1, 3}
    assert (a["entry"][(w.ids < 1) | (w.ids > 2)] == -1).all() and (a["counter"][w.ids == 0] == w.state["counter"][w.ids == 0]).all()
    assert (a["pos"][~drawn(a)] == w.state["pos"][~drawn(a)]).all() and (a["steps"][~drawn(a)] == w.state["steps"][~drawn(a)]).all()
    assert (a["steps"][drawn(a)] == 0).all() and (a["terminated"][drawn(a)] == 0).all() and (a["truncated"][drawn(a)] == 0).all()
    if w.ids[1] in (1, 2):
        assert a["counter"][1] == 0  # the count wrapped
    # scalars and their clamps: hi < lo, hi beyond the maximum, lo < 0, hi = -1 / None, an empty band (level 2 of puzzle 2)
    for scalar in ((0, None), (0, -1), (3, 1), (0, 99), (-3, 0), (2, 2), (1, 2)):
        s = w.run(w.state, scalar=scalar, seed=5)
        if scalar == (2, 2):  # puzzle 1 has its level 2; puzzle 2 has nothing there: outs -1, nothing moves, the count stays
            assert (s["entry"][w.ids == 2] == -1).all() and (s["entry"][w.ids == 1] >= 0).all()
            assert (s["counter"][w.ids == 2] == w.state["counter"][w.ids == 2]).all()
            assert (s["pos"][w.ids == 2] == w.state["pos"][w.ids == 2]).all()
        if scalar == (3, 1):
            assert set(s["level"][w.ids == 2]) == {3} and set(s["level"][w.ids == 1]) == {2}
        if scalar == (-3, 0):
            assert set(s["level"][w.ids == 2]) == {0} and set(s["level"][w.ids == 1]) == {-1}  # puzzle 1: levels 0 .. 0 are empty
    # a band per environment, a mask, no flags
    env = (rng.integers(-2, 6, size=w.B).astype(np.int32), rng.integers(-2, 6, size=w.B).astype(np.int32))
    mask = rng.integers(0, 2, size=w.B).astype(np.uint8)
    m = w.run(w.state, env=env, mask=mask, seed=(1 << 64) - 3)
    for k in m:  # environments outside the mask are untouched, byte for byte
        assert m[k][mask == 0].tobytes() == w.state[k][mask == 0].tobytes(), k
    w.run(w.state, env=env, flags=False, seed=9)
    # two draws in a row differ by the count alone; a seed restart (the counts back) gives the first draw again
    first = w.run(w.state, scalar=(0, None), seed=3)
    second = w.run(first, scalar=(0, None), seed=3)
    assert (second["counter"][drawn(first)] == (first["counter"][drawn(first)] + 1) & 0xFFFFFFFF).all()
    assert (second["entry"] != first["entry"]).sum() > 50
    again = w.run(w.state, scalar=(0, None), seed=3)
    assert all((again[k] == first[k]).all() for k in again)
    other = w.run(w.state, scalar=(0, None), seed=4)
    assert (other["entry"] != first["entry"]).sum() > 50


def test_keep_initial(draw_world):
    w = draw_world
    has = (w.ids == 1) | (w.ids == 2)
    none = w.run(w.state, scalar=(0, None), seed=2, keep_initial=0.0)
    assert (none["entry"][has] >= 0).all()
    every = w.run(w.state, scalar=(0, None), seed=2, keep_initial=1.0)
    assert (every["entry"] == -1).all() and (every["pos"] == w.state["pos"]).all() and (every["steps"] == w.state["steps"]).all()
    assert (every["counter"][has] == (w.state["counter"][has] + 1) & 0xFFFFFFFF).all()  # a kept state is a draw all the same
    half = w.run(w.state, scalar=(0, None), seed=2, keep_initial=0.5)
    kept = (half["entry"][has] == -1).mean()
    assert 0.3 < kept < 0.7
    assert (half["entry"][has & (half["entry"] >= 0)] == none["entry"][has & (half["entry"] >= 0)]).all()  # the draw stream is its own


# ---- 3. - 5., 8. autoreset loops against the oracle -----------------------------------------------------------------------------
def _level0(k):
    with zipfile.ZipFile(os.path.join(DATA, "puzzles", "level0.zip")) as z:
        return z.read(f"level0/base/train/level_0_base_train_{k}.pwp").decode()


class Level0:
    """Four small Level-0 puzzles (7 x 7 cells, three movables), their cost-to-go tables in moves and in pushes, and pools of
    at most 6 states per (puzzle, level)."""

    def __init__(self):
        from pushworld_amd.puzzle import PushWorldPuzzle
        from pushworld_amd.start_pool import StartPool
        from pushworld_amd.vec_env import VecPushWorld

        self.puzzles = [PushWorldPuzzle(text=_level0(k)) for k in range(4)]
        self.helper = VecPushWorld(self.puzzles, 64, observation=None)  # the set the tables are made on; answers the cost queries
        self.tables = self.helper.solution_tables(max_states_each=1 << 17)
        self.push_tables = self.helper.push_tables()
        self.pool = StartPool.from_tables(self.helper, [self.tables], max_per_level=6, seed=1)
        self.push_pool = StartPool.from_tables(self.helper, [self.push_tables], max_per_level=6, seed=1)
        self.ref, self.push_ref = _ref_of(self.pool), _ref_of(self.push_pool)

    def close(self):
        self.tables.close()
        self.push_tables.close()


def _ref_of(pool):
    return SR.Pool(_np(pool.puzzle), _np(pool.level), _np(pool.pos), pool.num_puzzles)


@pytest.fixture(scope="module")
def level0():
    w = Level0()
    yield w
    w.close()


def test_pools_from_tables(level0):
    for pool, ref in ((level0.pool, level0.ref), (level0.push_pool, level0.push_ref)):
        assert pool.order.tolist() == ref.order and pool.max_level.tolist() == ref.max_level
        assert pool.start.view(torch.int32).tolist() == ref.start and pool.lvl_off.tolist() == ref.lvl_off
        assert min(ref.max_level) >= 1  # every puzzle was solved: it has states a move / a push from the goal
        counts = np.bincount(_np(pool.puzzle).astype(np.int64) * 1000 + _np(pool.level))
        assert counts.max() == 6 and pool.num_entries == len(ref.order) > 40
    # every entry's level is its cost-to-go, by the tables' own query
    pool, h = level0.pool, level0.helper
    n = min(64, pool.num_entries)
    h.puzzle_id.copy_(pool.puzzle[:n].repeat(64 // n + 1)[:64])
    h.pos.copy_(pool.pos[:n].repeat(64 // n + 1, 1, 1)[:64])
    assert torch.equal(h.cost_to_go([level0.tables])[1], pool.level[:n].repeat(64 // n + 1)[:64])


class Oracle:
    """A second environment without a pool plus the restatement's draw, applied with ``set_states`` behind every step."""

    def __init__(self, vec, ref, seed, band):
        self.vec, self.ref, self.seed, self.band = vec, ref, seed, band
        B = vec.num_envs
        self.counter = np.zeros(B, np.int64)
        self.entry, self.level = np.full(B, -1, np.int32), np.full(B, -1, np.int32)

    def pending(self):
        return SR.arm(_np(self.vec.terminated), _np(self.vec.truncated))

    def draw(self, mask):
        v = self.vec
        pos, steps, term, trunc = _np(v.pos).copy(), _np(v.steps).copy(), _np(v.terminated).copy(), _np(v.truncated).copy()
        SR.draw(self.ref, _np(v.puzzle_id), pos, steps, term, trunc, self.counter, self.entry, self.level, seed=self.seed,
                mask=mask, band=self.band)
        v.set_states(pos)
        v.steps.copy_(torch.from_numpy(steps)), v.terminated.copy_(torch.from_numpy(term)), v.truncated.copy_(torch.from_numpy(trunc))

    def reset(self):
        self.vec.reset()
        self.entry[:], self.level[:] = -1, -1
        self.draw(None)
        if self.vec.obs is not None:
            self.vec.render()


def _same(vec, oracle, t, obs=True):
    o = oracle.vec
    for name in ("puzzle_id", "pos", "steps", "terminated", "truncated"):
        assert torch.equal(getattr(vec, name), getattr(o, name)), (name, t)
    assert torch.equal(vec.reward.view(torch.int64), o.reward.view(torch.int64)), t
    assert (_np(vec.start_entry) == oracle.entry).all() and (_np(vec.start_level) == oracle.level).all(), t
    assert (_np(vec.start_draws).view(np.uint32) == oracle.counter).all(), t
    if obs and vec.obs is not None:
        assert torch.equal(vec.obs, o.obs), t


def _band_of(pool):
    return _np(pool.band).copy()


@pytest.mark.parametrize("observation", ["uint8", "uint8 retained", "cells", None])
def test_autoreset_loop(level0, observation):
    from pushworld_amd.vec_env import VecPushWorld

    B, seed = 64, 5
    level0.pool.set_band(1, 3)
    kw = dict(max_steps=5, observation=None if observation is None else observation.split()[0], autoreset=True, seed=seed,
              pixels_per_cell=3, border_width=1)
    # (a retained buffer is one the library owns, of a bound batch: the tuner's own allocation, every puzzle bound)
    retained = dict(tune=True, tune_allocations=1, bind=True, engine_options={"bind_min_envs": 1}) \
        if observation == "uint8 retained" else {}
    if retained:
        kw["pad_cells"] = (16, 16)  # (frames of a page and more: smaller ones take the per-environment render, which retains nothing)
    vec = VecPushWorld(level0.puzzles, B, start_pool=level0.pool, **kw, **retained)
    oracle = Oracle(VecPushWorld(level0.puzzles, B, **kw), level0.ref, seed, _band_of(level0.pool))
    assert vec.start_pool is level0.pool and vec._call_pool_draw is not None and oracle.vec.start_pool is None
    if retained:
        assert vec.obs_owned_by_library
        assert vec.engine.get_option("obs_changed_pages") == 1 and vec.engine.get_option("obs_padding_once") == 1
    vec.reset(), oracle.reset()
    _same(vec, oracle, "reset")
    assert (_np(vec.start_level) >= 1).all() and (_np(vec.start_level) <= 3).all()
    gen = torch.Generator(device=vec.device).manual_seed(3)
    h, draws, zero_rewards = level0.helper, 0, 0
    for t in range(40):
        actions = torch.randint(0, 4, (B,), dtype=torch.uint8, device=vec.device, generator=gen)
        pending = oracle.pending()
        out = vec.step(actions)
        oracle.vec.step(actions)
        oracle.draw(pending)
        if oracle.vec.obs is not None:
            oracle.vec.render()
        assert out[0] is vec.obs and (_np(vec.start_pending) == pending).all()
        _same(vec, oracle, t)
        was = pending != 0
        assert (_np(vec.reward)[was] == 0.0).all() and (_np(vec.steps)[was] == 0).all()
        zero_rewards += int(was.sum())
        drawn = was & (oracle.entry >= 0)
        draws += int(drawn.sum())
        # every drawn state has the cost-to-go it was drawn for
        h.puzzle_id.copy_(vec.puzzle_id), h.pos.copy_(vec.pos)
        cost = _np(h.cost_to_go([level0.tables])[1])
        assert (cost[drawn] == _np(vec.start_level)[drawn]).all() and (cost[drawn] >= 1).all() and (cost[drawn] <= 3).all(), t
    assert draws == zero_rewards >= 4 * B  # (max_steps = 5: every environment ends at least every fifth step)
    if retained:
        # the render of the pool path is pw_render_retained: nothing differs from what the buffer shows, so no page is written
        # and a byte poked into it stays; the full render repairs it.  A buffer that is not the retained one gets the full render.
        good = vec.obs.clone()
        vec.obs[3, 0, 0, 0] ^= 0x55
        vec._render(retained=True)
        assert not torch.equal(vec.obs, good) and int((vec.obs != good).sum()) == 1
        vec.render()
        assert torch.equal(vec.obs, good)
        other, other_view = vec.engine.alloc_obs(B)
        vec.engine.render(vec.puzzle_id, vec.pos, other, retained=True)
        assert torch.equal(other_view, good)
        vec._render(retained=True)  # (the retained buffer is the engine's own again after the detour: the repair path)
        assert torch.equal(vec.obs, good)
    vec.reset(seed=seed)  # a seed restarts the counts
    oracle.counter[:] = 0
    oracle.reset()
    _same(vec, oracle, "reset(seed)")


def _choices(vec, gen):
    """A seeded valid push choice per environment (0 where there is none), from the views of the current states."""
    B, h, w = vec.push_view_mask.shape
    bits = torch.tensor([1, 2, 4, 8], dtype=torch.uint8, device=vec.device).view(1, 4, 1, 1)
    valid = ((vec.push_view_mask.unsqueeze(1) & bits) != 0).view(B, 4 * h * w)
    score = torch.rand((B, 4 * h * w), device=vec.device, generator=gen) * valid
    return score.argmax(dim=1)


def test_push_mode_loop(level0):
    from pushworld_amd.vec_env import VecPushWorld

    B, seed = 64, 8
    level0.push_pool.set_band(1, 2)
    kw = dict(max_steps=5, observation="cells", autoreset=True, seed=seed)
    vec = VecPushWorld(level0.puzzles, B, start_pool=level0.push_pool, **kw)
    oracle = Oracle(VecPushWorld(level0.puzzles, B, **kw), level0.push_ref, seed, _band_of(level0.push_pool))
    vec.reset(), oracle.reset()
    vec.observe_pushes(), oracle.vec.observe_pushes()
    gen = torch.Generator(device=vec.device).manual_seed(4)
    h, draws = level0.helper, 0
    for t in range(40):
        choice = _choices(vec, gen)
        pending = oracle.pending()
        step = vec.step_push_mask(choice=choice, end_stuck=True)
        ostep = oracle.vec.step_push_mask(choice=choice, end_stuck=True)
        oracle.draw(pending)
        oracle.vec.observe_pushes(), oracle.vec.render()
        _same(vec, oracle, t)
        assert torch.equal(step.moves, ostep.moves) and torch.equal(step.status, ostep.status)
        # the mask returned describes the state left, the drawn ones included
        mask, count = step.mask.clone(), step.num_pushes.clone()
        assert torch.equal(mask, vec.push_mask()) and torch.equal(count, vec.num_pushes), t
        assert torch.equal(mask, oracle.vec.push_view_mask)
        drawn = (pending != 0) & (oracle.entry >= 0)
        draws += int(drawn.sum())
        h.puzzle_id.copy_(vec.puzzle_id), h.pos.copy_(vec.pos)
        cost = _np(h.push_cost_to_go([level0.push_tables]).cost)
        assert (cost[drawn] == _np(vec.start_level)[drawn]).all() and (cost[drawn] >= 1).all() and (cost[drawn] <= 2).all(), t
        assert (_np(count)[drawn] > 0).all()
    assert draws >= 2 * B
    # step_push: the same pattern (arm, the step, the draw)
    pending = oracle.pending()
    q = h.push_cost_to_go([level0.push_tables])
    vec.step_push(q.push_from, q.push_action), oracle.vec.step_push(q.push_from, q.push_action)
    oracle.draw(pending), oracle.vec.render()
    _same(vec, oracle, "step_push")


def test_resample_draws_from_the_new_puzzle(level0):
    from pushworld_amd.vec_env import VecPushWorld

    B, seed = 64, 13
    level0.pool.set_band(0, None)
    kw = dict(max_steps=3, observation=None, autoreset=True, resample=True, seed=seed)
    vec = VecPushWorld(level0.puzzles, B, start_pool=level0.pool, **kw)
    oracle = Oracle(VecPushWorld(level0.puzzles, B, **kw), level0.ref, seed, _band_of(level0.pool))
    vec.reset(), oracle.reset()
    _same(vec, oracle, "reset")
    gen = torch.Generator(device=vec.device).manual_seed(6)
    moved = 0
    for t in range(12):
        before = _np(vec.puzzle_id).copy()
        actions = torch.randint(0, 4, (B,), dtype=torch.uint8, device=vec.device, generator=gen)
        pending = oracle.pending()
        vec.step(actions), oracle.vec.step(actions)
        oracle.draw(pending)
        _same(vec, oracle, t)
        was = pending != 0
        ids, entry = _np(vec.puzzle_id), _np(vec.start_entry)
        assert (entry[was] >= 0).all() and (_np(level0.pool.puzzle)[entry[was]] == ids[was]).all(), t
        moved += int((ids[was] != before[was]).sum())
        assert (ids[~was] == before[~was]).all()
    assert moved > B


def test_facades(level0):
    from pushworld_amd.vector_env import PushWorldPushVectorEnv, PushWorldVectorEnv

    B, seed = 16, 2
    for cls, pool, ref in ((PushWorldVectorEnv, level0.pool, level0.ref), (PushWorldPushVectorEnv, level0.push_pool, level0.push_ref)):
        push = cls is PushWorldPushVectorEnv
        pool.set_band(1, 1)
        pool.base.zero_()
        kw = dict(max_steps=4, observation="uint8", seed=seed, pixels_per_cell=3, border_width=1)
        env = cls(level0.puzzles, B, start_pool=pool, start_update_every={"every": 4, "min_episodes": 8, "up": 0.75}, **kw)
        plain = cls(level0.puzzles, B, **kw)
        assert env.start_pool is pool and env.vec.stats is not None and pool.stats is env.vec.stats
        oracle = Oracle(plain.vec, ref, seed, _band_of(pool))
        obs, info = env.reset()
        assert "start_level" not in plain.reset()[1] and (_np(info["start_level"]) == 1).all()
        oracle.entry[:], oracle.level[:] = -1, -1
        oracle.draw(None), plain.vec.render()
        if push:
            plain.vec.observe_pushes()
            assert torch.equal(info["push_mask"], plain.vec.push_view_mask)
        _same(env.vec, oracle, "reset")
        gen = torch.Generator(device=env.vec.device).manual_seed(9)
        for t in range(20):
            if push:
                actions = _choices(env.vec, gen)
            else:
                actions = torch.randint(0, 4, (B,), dtype=torch.uint8, device=env.vec.device, generator=gen)
            if t == 3:  # crafted successes: the update behind the fourth step moves every band up by one
                env.vec.stats.tensor[:, :2] += 100
                assert _np(pool.band).tolist() == [[1, 1]] * 4 and pool.updates == 0
            pending = oracle.pending()
            obs, reward, terminated, truncated, info = env.step(actions)
            plain.step(actions)
            oracle.draw(pending), plain.vec.render()
            if push:
                plain.vec.observe_pushes()
                assert torch.equal(info["push_mask"], plain.vec.push_view_mask), t
            _same(env.vec, oracle, t)
            assert obs is env.vec.obs and info["start_level"] is env.vec.start_level and info["start_entry"] is env.vec.start_entry
            if t == 3:
                hi = [min(2, ml) for ml in pool.max_level.tolist()]
                assert pool.updates == 1 and _np(pool.band).tolist() == [[1, x] for x in hi] and max(hi) == 2
                assert _np(pool.delta).tolist() == [x - 1 for x in hi]
                assert torch.equal(pool.base, env.vec.stats.tensor)
            if t % 4 == 3:  # (the draws of the following steps read the band the update left)
                assert pool.updates == t // 4 + 1
                oracle.band = _band_of(pool)
        assert pool.updates == 5
        pool.stats = None


# ---- 6. the bands against the restatement --------------------------------------------------------------------------------------
def test_update_bands():
    from pushworld_amd.puzzle import PushWorldPuzzle
    from pushworld_amd.start_pool import StartPool
    from pushworld_amd.vec_env import VecPushWorld

    vec = VecPushWorld([PushWorldPuzzle(text=_puzzle_text(3))] * 6, 4, observation=None)
    # max_level 5 5 5 - 5 2: puzzle 3 has no entries
    puzzle = np.array([0, 1, 2, 4, 5, 0], np.int32)
    level = np.array([5, 5, 5, 5, 2, 0], np.int32)
    pool = StartPool(vec, puzzle, level, np.zeros((6, 4, 2), np.int8))
    max_level = pool.max_level.tolist()
    assert max_level == [5, 5, 5, -1, 5, 2] and _np(pool.band).tolist() == [[1, 1], [1, 1], [1, 1], [0, 0], [1, 1], [1, 1]]
    dev = vec.device

    def both(stats, band, base, **kw):
        """One update on the device and one by the restatement; returns (band, base, delta) both agree on."""
        pool.band.copy_(torch.tensor(band, dtype=torch.int32))
        pool.base.copy_(torch.tensor(base, dtype=torch.int64))
        pool.delta.fill_(7)  # (what is not written stays)
        pool.update_bands(torch.tensor(stats, dtype=torch.int64, device=dev), **kw)
        band, base = [list(b) for b in band], [list(b) for b in base]
        q = {k: v for k, v in kw.items() if k not in ("up", "down")}
        delta = SR.update_bands(max_level, stats, base, band, up_q16=int(round(kw.get("up", 0.8) * 65536)),
                                down_q16=int(round(kw.get("down", 0.2) * 65536)), **q)
        assert _np(pool.band).tolist() == band and _np(pool.base).tolist() == base
        assert _np(pool.delta).tolist() == [7 if d is None else d for d in delta]
        return band, base, delta

    zero = [[0] * 4 for _ in range(6)]
    # 0: exactly on `up` (30 of 40 at 0.75) -> up; 1: exactly on `down` (10 of 40 at 0.25) -> not below: stays; 2: below
    # min_episodes: nothing written, the base stays; 3: no entries; 4: hi = -1 on entry, all solved: the clamp at max_level;
    # 5: below `down` at hi_min: the clamp
    stats = [[40, 30, 400, 300], [40, 10, 7, 7], [31, 31, 5, 5], [64, 64, 1, 1], [40, 40, 2, 2], [40, 9, 3, 3]]
    band = [[1, 4], [1, 3], [1, 2], [0, 0], [2, -1], [1, 1]]
    band, base, delta = both(stats, band, zero, up=0.75, down=0.25)
    assert band == [[1, 5], [1, 3], [1, 2], [0, 0], [2, 5], [1, 1]] and delta == [1, 0, None, None, 0, 0]
    assert base == [stats[0], stats[1], [0] * 4, [0] * 4, stats[4], stats[5]]
    # the second update: the windows of 0, 1, 4, 5 restart (nothing new: below min_episodes), 2 has its 32 now
    stats2 = [list(s) for s in stats]
    stats2[2] = [32, 31, 5, 5]
    band2, base2, delta2 = both(stats2, band, base, up=0.75, down=0.25)
    assert delta2 == [None, None, 1, None, None, None] and band2[2] == [1, 3] and base2[2] == stats2[2]
    # width 2 drags lo along, step 2, hi_min / lo_min, one step below `down`; width 0 leaves lo alone
    stats3 = [[s[0] + 40, s[1] + (9 if p % 2 else 31), s[2], s[3]] for p, s in enumerate(stats2)]
    band3, _, delta3 = both(stats3, [[1, 4], [1, 4], [1, 1], [0, 0], [3, 5], [2, 2]], base2, up=0.75, down=0.25, step=2, width=2,
                            hi_min=3, lo_min=2)
    assert band3 == [[4, 5], [2, 3], [2, 3], [0, 0], [4, 5], [2, 2]] and delta3 == [1, -1, 1, None, 0, 0]
    band4, _, _ = both(stats3, [[0, 4], [3, 4], [1, 1], [0, 0], [3, 5], [2, 2]], base2, min_episodes=40, width=0)
    assert [b[0] for b in band4] == [0, 3, 1, 0, 3, 2]
    # a negative window, more solved than ended, and counts beyond 2^20
    big = [[1 << 40, (1 << 40) - (1 << 37), 0, 0], [5, 5, 0, 0], [40, 90, 0, 0], [0, 0, 0, 0], [1 << 33, 1 << 30, 0, 0],
           [(1 << 62) + 40, 1 << 62, 0, 0]]
    both(big, [[1, 1]] * 6, [[0] * 4, [9, 0, 0, 0], [0] * 4, [0] * 4, [0] * 4, [1 << 62, (1 << 62) - 1, 0, 0]])


# ---- 7. capture ----------------------------------------------------------------------------------------------------------------
def test_captured_arm_draw_and_update(level0):
    from pushworld_amd.curriculum import EpisodeStats
    from pushworld_amd.start_pool import StartPool

    h, dev, B = level0.helper, level0.helper.device, 64
    pools = [StartPool(h, level0.pool.puzzle, level0.pool.level, level0.pool.pos) for _ in range(2)]  # eager, graphed

    def state():
        return dict(puzzle_id=torch.from_numpy((np.arange(B) % 4).astype(np.int32)).to(dev), pos=torch.zeros((B, h.engine.np, 2), dtype=torch.int8, device=dev),
                    steps=torch.full((B,), 3, dtype=torch.int32, device=dev), terminated=torch.zeros(B, dtype=torch.uint8, device=dev),
                    truncated=torch.zeros(B, dtype=torch.uint8, device=dev), pending=torch.zeros(B, dtype=torch.uint8, device=dev),
                    counter=torch.zeros(B, dtype=torch.int32, device=dev), entry=torch.full((B,), -1, dtype=torch.int32, device=dev),
                    level=torch.full((B,), -1, dtype=torch.int32, device=dev), stats=EpisodeStats(h))

    def launch(pool, s):
        h.engine.start_pool_arm(s["terminated"], s["truncated"], s["pending"])
        pool.draw(s["puzzle_id"], s["pos"], s["steps"], s["terminated"], s["truncated"], mask=s["pending"], seed=17,
                  counter=s["counter"], out=(s["entry"], s["level"]))
        pool.update_bands(s["stats"], min_episodes=4)

    def feed(s, k):
        """What a step would leave: flags for some environments, statistics that grow."""
        flags = torch.from_numpy(np.random.default_rng(k).integers(0, 2, size=B).astype(np.uint8)).to(dev)
        s["terminated"].copy_(flags)
        s["stats"].tensor[:, 0] += 5
        s["stats"].tensor[:, 1] += 5 if k % 2 == 0 else 0

    eager, graphed = state(), state()
    side = torch.cuda.Stream(device=dev)  # warm-up on a side stream, then capture the three launches: a linear graph
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        feed(graphed, 0)
        launch(pools[1], graphed)
    torch.cuda.current_stream(dev).wait_stream(side)
    feed(eager, 0)
    launch(pools[0], eager)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch(pools[1], graphed)
    for k in (1, 2):  # (the capture itself ran nothing)
        feed(graphed, k), feed(eager, k)
        g.replay()
        launch(pools[0], eager)
        for name in ("pos", "steps", "terminated", "truncated", "pending", "counter", "entry", "level"):
            assert torch.equal(eager[name], graphed[name]), (name, k)
        for name in ("band", "base", "delta"):
            assert torch.equal(getattr(pools[0], name), getattr(pools[1], name)), (name, k)
    assert int(graphed["counter"].sum()) > B and int(graphed["counter"].max()) <= 3
    assert _np(pools[1].band)[:, 1].max() > 1


# ---- defaults untouched --------------------------------------------------------------------------------------------------------
def test_without_a_pool_nothing_changes(level0):
    from pushworld_amd.vec_env import VecPushWorld

    vec = VecPushWorld(level0.puzzles, 8, max_steps=3, observation=None, autoreset=True)
    assert vec.start_pool is None and vec._call_pool_arm is None and vec._call_pool_draw is None
    assert not hasattr(vec, "start_entry") and not hasattr(vec, "start_pending")
    with pytest.raises(ValueError, match="the start pool covers 4 puzzles"):
        VecPushWorld(level0.puzzles[:3], 8, autoreset=True, observation=None, start_pool=level0.pool)

"""-m gpu: the frame padding of a retained observation buffer is written once (PW_OPT_OBS_PADDING_ONCE).

pw_step_render of a bound batch into a library-owned buffer renders the live pages only; every test compares the whole
buffer with a twin engine that has the option off (and sampled environments with the C oracle), for every form of the
live launch, and checks that the padding is really skipped, that pw_render repairs it and that everything that may change
the padding ends the retention."""
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PAD_H, PAD_W = 51, 42  # the Level-1 frame in cells
BIG, SMALL = 40, 36    # pool indices of the 51 x 42 puzzle (no padding rows at all) and of the 5 x 6 one (nearly all padding)


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def pool():
    import bench
    from oracle import c_oracle
    from pushworld_amd.puzzle import PushWorldPuzzle

    paths = bench.level1_paths()
    texts = [open(p).read() for p in paths]
    puzzles = [PushWorldPuzzle(p) for p in paths]
    heights = np.array([p.dimensions[1] for p in puzzles])
    assert tuple(puzzles[BIG].dimensions) == (PAD_W, PAD_H) and tuple(puzzles[SMALL].dimensions) == (6, 5)
    return {"puzzles": puzzles, "oracles": [c_oracle.COraclePuzzle(t) for t in texts], "heights": heights}


def _ids(B, n):
    """The mix of a batch: the benchmark's assignment where it holds every puzzle, else the two extremes first."""
    if B >= n:
        return (np.arange(B, dtype=np.int64) * n) // B
    first = [SMALL, BIG, 2, 8, 26]
    rest = [i for i in range(n) if i not in first]
    return np.array((first + rest)[:B] if B > 1 else [SMALL], dtype=np.int64)


def _vec(pool, B, dtype="uint8", option=1, ids=None, **kw):
    from pushworld_amd.vec_env import VecPushWorld

    ids = _ids(B, len(pool["puzzles"])) if ids is None else ids
    args = dict(puzzle_ids=ids, max_steps=5, pixels_per_cell=3, border_width=1, observation=dtype, device=0, autoreset=True,
                tune=False, bind=True, engine_options={"bind_min_envs": 1, "obs_padding_once": option})
    args.update(kw)
    return VecPushWorld(pool["puzzles"], B, **args), ids


def _step_into(vec, st, actions):
    vec.engine.step_render(vec.puzzle_id, actions, vec.pos, vec.steps, vec.reward, vec.dgoals, vec.terminated, vec.truncated, st,
                           vec.flags)


def _oracle(pool, vec, ids, envs, dtype):
    from oracle import c_oracle

    return c_oracle.observe_batch(pool["oracles"], ids, vec.states(), envs, PAD_H, PAD_W, 3, 1, "f32" if dtype == "float32" else "u8")


def _pages(heights, ids, es):
    """The rule, restated: (live mask, whole-page mask, pages) of a library-owned buffer of the batch.  A page is skippable
    iff every 16-byte chunk the full kernel stores in it lies outside [nz_lo, nz_hi) of its environment."""
    obs_bytes = PAD_H * 3 * PAD_W * 3 * 3 * es
    stride = (obs_bytes + 511) // 512 * 512
    cpe, n_chunks, B = stride // 16, (obs_bytes + 15) // 16, len(ids)
    n_pages = (B * cpe + 255) // 256
    H = heights[np.asarray(ids)]
    pady = (PAD_H - H) * 3 // 2
    row_b = 9 * PAD_W * es
    nz_lo, nz_hi = (pady * row_b) >> 4, ((pady + 3 * H) * row_b + 15) >> 4

    def padding(env, lo, hi):
        return (lo >= hi) | (hi <= nz_lo[env]) | (lo >= nz_hi[env])

    g0 = np.arange(n_pages, dtype=np.int64) * 256
    env0 = g0 // cpe
    c_first = g0 - env0 * cpe
    whole = c_first + 256 <= n_chunks
    split = cpe - c_first
    has_second = (split < 256) & (env0 + 1 <= B - 1)
    env1 = np.minimum(env0 + 1, B - 1)
    skip_tail = padding(env0, c_first, np.full_like(c_first, n_chunks))
    skip_head = ~has_second | padding(env1, np.zeros_like(c_first), np.minimum(256 - split, n_chunks))
    skip = np.where(whole, padding(env0, c_first, c_first + 256), skip_tail & skip_head)
    return ~skip, whole, n_pages


def _bytes(torch, st):
    return st.view(torch.uint8).reshape(-1)


def _twins(pool, B, dtype, option=1):
    """(vec, buffer, view) with the option on and off: same puzzles, same states, library-owned buffers, rendered."""
    out = []
    for opt in (option, 0):
        vec, ids = _vec(pool, B, dtype, opt)
        vec.reset()
        st, view = vec.engine.alloc_obs_owned(B)
        vec.engine.render(vec.puzzle_id, vec.pos, st)
        out.append((vec, st, view))
    return out[0], out[1], ids


@pytest.mark.parametrize("dtype", ["uint8", "float32"])
@pytest.mark.parametrize("B", [1, 3, 50, 4096])
def test_every_step_equals_the_full_render(torch_mod, pool, B, dtype):
    torch = torch_mod
    (vec, st, view), (ref, rst, rview), ids = _twins(pool, B, dtype)
    es = 1 if dtype == "uint8" else 4
    live, _, n_pages = _pages(pool["heights"], ids, es)
    assert vec.engine.get_option("obs_live_pages") == int(live.sum()) and ref.engine.get_option("obs_live_pages") == 0
    if B > 1:
        assert int(live.sum()) < n_pages
    g = torch.Generator(device=vec.device).manual_seed(7 + B)
    envs = sorted({0, B // 2, B - 1, min(1, B - 1)})
    for t in range(20):
        a = torch.randint(0, 4, (B,), generator=g, device=vec.device, dtype=torch.uint8)
        _step_into(vec, st, a)
        _step_into(ref, rst, a)
        assert torch.equal(view, rview), t
        assert torch.equal(vec.terminated, ref.terminated) and torch.equal(vec.truncated, ref.truncated)
        if t % 6 == 5:  # (after the autoresets of step 5, 11, 17 too)
            assert np.array_equal(view[envs].cpu().numpy(), _oracle(pool, vec, ids, envs, dtype)), t
    assert vec.engine.get_option("obs_live_pages") == int(live.sum())


@pytest.mark.parametrize("B,dtype", [(1, "uint8"), (3, "float32"), (50, "uint8"), (4096, "uint8")])
def test_every_launch_form(torch_mod, pool, B, dtype):
    """Page orders x run lengths x every-page-loads x {list, early exits}, with the exact grid and -- after a re-bind in-stream
    (pw_reset on the bound ids) -- with the upper-bound grid whose surplus workgroups read the count on the device."""
    torch = torch_mod
    (vec, st, view), (ref, rst, rview), ids = _twins(pool, B, dtype, option=3)
    live, _, n_pages = _pages(pool["heights"], ids, 1 if dtype == "uint8" else 4)
    n_live = int(live.sum())
    if B == 1:
        assert n_live % 8 != 0 and n_live < 8  # shorter than every span 8 << run_log2, and no multiple of 8
    g = torch.Generator(device=vec.device).manual_seed(100 + B)
    for upper_bound in (False, True):
        if upper_bound:
            for v, s in ((vec, st), (ref, rst)):
                v.engine.reset(v.puzzle_id, v.pos, v.steps, v.terminated, v.truncated, None)  # rebuilds the list behind itself
                v.engine.render(v.puzzle_id, v.pos, s)
        for form in (3, 2):
            vec.engine.set_option("obs_padding_once", form)
            vec.engine.render(vec.puzzle_id, vec.pos, st)  # (setting the option ends the retention: establish it again)
            assert vec.engine.get_option("obs_live_pages") == n_live
            for order in (0, 1, 2):
                for run_log2 in (0, 3, 6):
                    for load_all in (0, 1):
                        for k, v in (("page_order", order), ("page_run_log2", run_log2), ("page_load_all", load_all)):
                            vec.engine.set_option(k, v)
                        for _ in range(2):
                            a = torch.randint(0, 4, (B,), generator=g, device=vec.device, dtype=torch.uint8)
                            _step_into(vec, st, a)
                            _step_into(ref, rst, a)
                        assert torch.equal(view, rview), (upper_bound, form, order, run_log2, load_all)
    envs = sorted({0, B - 1})
    assert np.array_equal(view[envs].cpu().numpy(), _oracle(pool, vec, ids, envs, dtype))


@pytest.mark.parametrize("dtype,share", [("uint8", 0.323), ("float32", 0.2706)])
def test_the_list_is_the_rule(torch_mod, pool, dtype, share):
    B = 4096
    vec, ids = _vec(pool, B, dtype)
    vec.reset()
    st, view = vec.engine.alloc_obs_owned(B)
    assert vec.engine.get_option("obs_live_pages") == 0  # nothing rendered into a buffer of the library's yet
    vec.engine.render(vec.puzzle_id, vec.pos, st)
    live, whole, n_pages = _pages(pool["heights"], ids, 1 if dtype == "uint8" else 4)
    assert vec.engine.get_option("obs_live_pages") == int(live.sum())
    assert int(live.sum()) / n_pages == pytest.approx(share, abs=0.001)
    if dtype == "uint8":  # the issue's table: 60.7 % whole pages of padding, nearly all of the 7.08 % straddling ones
        assert int((whole & ~live).sum()) / n_pages == pytest.approx(0.607, abs=0.002)
        assert int((~whole & ~live).sum()) / n_pages == pytest.approx(0.0697, abs=0.001)


@pytest.mark.parametrize("dtype", ["uint8", "float32"])
def test_it_skips_and_render_repairs(torch_mod, pool, dtype):
    torch = torch_mod
    B = 50
    (vec, st, view), (ref, rst, rview), ids = _twins(pool, B, dtype)
    live, whole, n_pages = _pages(pool["heights"], ids, 1 if dtype == "uint8" else 4)
    p_whole = int(np.flatnonzero(whole & ~live)[3])
    p_strad = int(np.flatnonzero(~whole & ~live)[1])

    def poison(storage):
        flat = _bytes(torch, storage)
        for p in (p_whole, p_strad):
            flat[p * 4096:(p + 1) * 4096] = 0xAB

    g = torch.Generator(device=vec.device).manual_seed(5)
    a = torch.randint(0, 4, (B,), generator=g, device=vec.device, dtype=torch.uint8)
    poison(st)
    _step_into(vec, st, a)
    _step_into(ref, rst, a)
    want = rst.clone()
    poison(want)
    h, w, c = vec.engine.obs_shape
    want_view = want.as_strided((B, h, w, c), rview.stride())
    assert not torch.equal(view, rview) and torch.equal(view, want_view)  # both pages survive, every other byte is the reference's
    vec.engine.render(vec.puzzle_id, vec.pos, st)
    assert torch.equal(view, rview)
    # a buffer of torch's, or the option off: the same poison is gone after one step
    for v, s, vw in ((vec, vec._obs_storage, vec.obs), (ref, rst, rview)):
        v.engine.render(v.puzzle_id, v.pos, s)
        poison(s)
    a = torch.randint(0, 4, (B,), generator=g, device=vec.device, dtype=torch.uint8)
    _step_into(ref, rst, a)
    _step_into(vec, vec._obs_storage, a)
    assert torch.equal(vec.obs, rview)
    stride = vec.engine.obs_stride
    envs = sorted({p_whole * 4096 // stride, p_strad * 4096 // stride, p_strad * 4096 // stride + 1})
    assert np.array_equal(rview[envs].cpu().numpy(), _oracle(pool, ref, ids, envs, dtype))  # (the poisoned environments)
    # ... and that full render into another buffer left the retained one alone: it still skips
    a = torch.randint(0, 4, (B,), generator=g, device=vec.device, dtype=torch.uint8)
    poison(st)
    _step_into(vec, st, a)
    _step_into(ref, rst, a)
    want = rst.clone()
    poison(want)
    assert torch.equal(view, want.as_strided((B, h, w, c), rview.stride()))


@pytest.mark.parametrize("how", ["bind", "reset"])
def test_new_ids_end_the_retention(torch_mod, pool, how):
    """The small puzzle and the 51 x 42 one swap places: old pixels lie in the new padding."""
    torch = torch_mod
    B = 50
    (vec, st, view), (ref, rst, rview), ids = _twins(pool, B, "uint8")
    new_ids = ids.copy()
    i_small, i_big = int(np.flatnonzero(ids == SMALL)[0]), int(np.flatnonzero(ids == BIG)[0])
    new_ids[i_small], new_ids[i_big] = BIG, SMALL
    for v in (vec, ref):
        if how == "bind":
            v.set_puzzle_ids(new_ids)  # pw_batch_bind
            assert v.engine.get_option("obs_live_pages") == 0
        else:
            v.puzzle_id.copy_(torch.as_tensor(new_ids, dtype=torch.int32))
        v.engine.reset(v.puzzle_id, v.pos, v.steps, v.terminated, v.truncated, None)  # (re-binds behind itself)
        assert v.engine.get_option("obs_live_pages") == 0
    a = torch.zeros((B,), device=vec.device, dtype=torch.uint8)
    _step_into(vec, st, a)
    _step_into(ref, rst, a)
    assert torch.equal(view, rview)
    envs = [i_small, i_big, B - 1]
    assert np.array_equal(view[envs].cpu().numpy(), _oracle(pool, vec, new_ids, envs, "uint8"))
    live, _, _ = _pages(pool["heights"], new_ids, 1)
    assert vec.engine.get_option("obs_live_pages") == int(live.sum())  # retained again, with the new list
    _step_into(vec, st, a)
    _step_into(ref, rst, a)
    assert torch.equal(view, rview)


def test_resampled_puzzles_are_rendered_in_full(torch_mod, pool):
    torch = torch_mod
    B = 50
    vecs = []
    for opt in (1, 0):
        vec, ids = _vec(pool, B, "uint8", opt, resample=True, seed=3, tune=True, tune_allocations=1)
        assert vec.obs_owned_by_library and vec.engine.get_option("obs_padding_once") == opt
        vec.reset()
        vecs.append(vec)
    vec, ref = vecs
    g = torch.Generator(device=vec.device).manual_seed(9)
    for t in range(20):
        a = torch.randint(0, 4, (B,), generator=g, device=vec.device, dtype=torch.uint8)
        vec.step(a)
        ref.step(a)
        assert torch.equal(vec.puzzle_id, ref.puzzle_id) and torch.equal(vec.obs, ref.obs), t
    assert len(set(vec.puzzle_id.cpu().numpy().tolist()) - set(ids.tolist())) > 0  # puzzles did change
    envs = [0, 1, B - 1]
    assert np.array_equal(vec.obs[envs].cpu().numpy(), _oracle(pool, vec, vec.puzzle_id.cpu().numpy(), envs, "uint8"))


def test_vec_env_turns_it_on_for_its_own_buffer(torch_mod, pool):
    torch = torch_mod
    from pushworld_amd.vec_env import VecPushWorld

    B = 50
    ids = _ids(B, len(pool["puzzles"]))
    args = dict(puzzle_ids=ids, max_steps=5, pixels_per_cell=3, border_width=1, observation="uint8", device=0, autoreset=True,
                tune=True, tune_allocations=1)
    vec = VecPushWorld(pool["puzzles"], B, engine_options={"bind_min_envs": 1}, **args)
    off = VecPushWorld(pool["puzzles"], B, engine_options={"bind_min_envs": 1, "obs_padding_once": 0}, **args)
    torch_owned = VecPushWorld(pool["puzzles"], B, engine_options={"bind_min_envs": 1}, **dict(args, tune=False))
    assert vec.engine.get_option("obs_padding_once") == 1 and off.engine.get_option("obs_padding_once") == 0
    assert torch_owned.engine.get_option("obs_padding_once") == 0
    for v in (vec, off, torch_owned):
        v.reset()
    live, _, _ = _pages(pool["heights"], ids, 1)
    assert vec.engine.get_option("obs_live_pages") == int(live.sum())
    assert off.engine.get_option("obs_live_pages") == 0 and torch_owned.engine.get_option("obs_live_pages") == 0
    g = torch.Generator(device=vec.device).manual_seed(21)
    for t in range(12):
        a = torch.randint(0, 4, (B,), generator=g, device=vec.device, dtype=torch.uint8)
        for v in (vec, off, torch_owned):
            v.step(a)
        assert torch.equal(vec.obs, off.obs) and torch.equal(vec.obs, torch_owned.obs), t
    with pytest.raises(ValueError):
        vec.engine.set_option("obs_padding_once", 4)
    with pytest.raises(ValueError):
        vec.engine.set_option("obs_live_pages", 1)


def test_a_freed_buffer_is_forgotten_and_a_new_one_starts_unretained(torch_mod, pool):
    torch = torch_mod
    B = 50
    (vec, st, view), (ref, rst, rview), ids = _twins(pool, B, "uint8")
    assert vec.engine.get_option("obs_live_pages") > 0
    del st, view
    gc.collect()  # pw_obs_free
    assert vec.engine.get_option("obs_live_pages") == 0
    st, view = vec.engine.alloc_obs_owned(B)
    _bytes(torch, st).fill_(0xAB)  # (a fresh buffer is zero: only other bytes show whether its padding is written)
    a = torch.ones((B,), device=vec.device, dtype=torch.uint8)
    _step_into(vec, st, a)
    _step_into(ref, rst, a)
    assert torch.equal(view, rview)
    assert vec.engine.get_option("obs_live_pages") > 0
    # the options under which nothing is retained
    for key, value in (("page_slice_envs", 7), ("render_kernel", "lds"), ("fused_step_render", 1)):
        vec.engine.set_option(key, value)
        assert vec.engine.get_option("obs_live_pages") == 0
        _bytes(torch, st).fill_(0xAB)
        _step_into(vec, st, a)
        _step_into(ref, rst, a)
        assert torch.equal(view, rview), key
        assert vec.engine.get_option("obs_live_pages") == 0
        vec.engine.set_option(key, 0)
    vec.engine.unbind()
    _bytes(torch, st).fill_(0xAB)
    _step_into(vec, st, a)
    _step_into(ref, rst, a)
    assert torch.equal(view, rview) and vec.engine.get_option("obs_live_pages") == 0


def test_the_incremental_redraw_and_the_retained_buffer(torch_mod, pool):
    """pw_step_render_delta of the retained batch stays inside the puzzles' own rows (retention kept, steps alternate freely);
    a redraw of another id buffer into the retained buffer ends it."""
    torch = torch_mod
    B = 50
    (vec, st, view), (ref, rst, rview), ids = _twins(pool, B, "uint8")
    n_live = vec.engine.get_option("obs_live_pages")
    g = torch.Generator(device=vec.device).manual_seed(13)
    for t in range(12):
        a = torch.randint(0, 4, (B,), generator=g, device=vec.device, dtype=torch.uint8)
        if t % 2:
            vec.engine.step_render_delta(vec.puzzle_id, a, vec.pos, vec.steps, vec.reward, vec.dgoals, vec.terminated, vec.truncated,
                                         st, vec.flags)
        else:
            _step_into(vec, st, a)
        _step_into(ref, rst, a)
        assert torch.equal(view, rview), t
        assert vec.engine.get_option("obs_live_pages") == n_live
    other = vec.puzzle_id.clone()
    vec.engine.step_render_delta(other, a, vec.pos, vec.steps, vec.reward, vec.dgoals, vec.terminated, vec.truncated, st, vec.flags)
    _step_into(ref, rst, a)
    assert torch.equal(view, rview) and vec.engine.get_option("obs_live_pages") == 0

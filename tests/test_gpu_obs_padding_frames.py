"""-m gpu: the live-page render of a retained observation buffer (PW_OPT_OBS_PADDING_ONCE) on other frames, strides and launch
forms than tests/test_gpu_obs_padding.py -- the cases of tests/live_pages_restatement.py (test_live_pages_host.py shows on the
CPU that they hold every kind of page).  Every comparison is byte-exact.

  a. the bytes a live launch writes are exactly the stored chunks of the live pages, for every launch form: the whole storage
     is filled with 0xAB, one pw_step_render runs, and afterwards every byte is either still 0xAB or what the full render of the
     same state (pw_render, the repair path) puts there -- the latter exactly where the restatement says
  b. twenty random steps with autoreset against a twin with the option off
  c. a batch of more than 1 048 576 pages: the scan of the per-1 024-page counts carries from one round to the next
  d. a render or step of a sub-batch into a slice of the retained buffer ends the retention, one into another buffer does not
  e. captured pw_step_render launches replay the live form"""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import live_pages_restatement as lp  # noqa: E402

pytestmark = pytest.mark.gpu

POISON = 0xAB


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


@pytest.fixture(scope="module")
def pools(torch_mod):
    from oracle import c_oracle
    from pushworld_amd import _capi
    from pushworld_amd.puzzle import PushWorldPuzzle

    out = {}
    for name, texts in lp.POOLS.items():
        texts = texts()
        puzzles = [PushWorldPuzzle(text=t) for t in texts]
        heights = np.array([p.dimensions[1] for p in puzzles])
        assert np.array_equal(heights, lp.text_heights(texts))
        out[name] = {"pset": _capi.PuzzleSet([p._parsed for p in puzzles], 0), "heights": heights,
                     "oracles": [c_oracle.COraclePuzzle(t) for t in texts]}
    return out


def _vec(pool, c, ids, option, B=None):
    from pushworld_amd.vec_env import VecPushWorld

    return VecPushWorld(pool["pset"], c.B if B is None else B, puzzle_ids=ids, max_steps=5, pixels_per_cell=lp.PPC, border_width=lp.BW,
                        observation=c.dtype, pad_cells=(c.pad_h, c.pad_w), device=0, autoreset=True, tune=False, bind=True,
                        engine_options={"bind_min_envs": 1, "obs_padding_once": option})


def _retained(pool, c, ids, option):
    """(vec, storage, view): reset, a library-owned buffer, rendered -- which establishes the retention where the option is on."""
    vec = _vec(pool, c, ids, option, B=len(ids))
    vec.reset()
    st, view = vec.engine.alloc_obs_owned(len(ids))
    vec.engine.render(vec.puzzle_id, vec.pos, st)
    return vec, st, view


def _step_into(vec, st, actions, delta=False):
    fn = vec.engine.step_render_delta if delta else vec.engine.step_render
    fn(vec.puzzle_id, actions, vec.pos, vec.steps, vec.reward, vec.dgoals, vec.terminated, vec.truncated, st, vec.flags)


def _bytes(torch, st):
    return st.view(torch.uint8).reshape(-1)


def _oracle(pool, c, vec, ids, envs):
    from oracle import c_oracle

    return c_oracle.observe_batch(pool["oracles"], ids, vec.states(), envs, c.pad_h, c.pad_w, lp.PPC, lp.BW,
                                  "f32" if c.dtype == "float32" else "u8")


def _sample_envs(parts, B):
    """First, last, and the two environments that meet in a straddling page of padding (where there is one)."""
    envs = {0, B - 1}
    dead = np.flatnonzero(~parts["whole"] & parts["has_head"] & ~parts["live"])
    if dead.size:
        e = int(parts["env"][dead[dead.size // 2]])
        envs |= {e, e + 1}
    return sorted(envs)


def _byte_mask(torch, dev, c, heights, ids, live, n_bytes):
    m = lp.written_mask(c.pad_h, c.pad_w, lp.case_es(c), heights, ids, live=live, chunks=True)
    return torch.from_numpy(m).to(dev).repeat_interleave(16)[:n_bytes]


def _set_form(eng, order, run_log2, load_all):
    for k, v in (("page_order", order), ("page_run_log2", run_log2), ("page_load_all", load_all)):
        eng.set_option(k, v)


def _written_is_live(torch, vec, st, mask, actions, form, what):
    """One live launch in `form` over a poisoned buffer, then the repair -- the full render in its plainest form, whatever the
    live launch's: the launch wrote the masked bytes, all of them, nothing else."""
    flat = _bytes(torch, st)
    flat.fill_(POISON)
    _set_form(vec.engine, *form)
    _step_into(vec, st, actions)
    snapshot = flat.clone()
    _set_form(vec.engine, 0, 0, 0)
    vec.engine.render(vec.puzzle_id, vec.pos, st)
    want = torch.where(mask, flat, torch.full_like(flat[:1], POISON))
    if not torch.equal(snapshot, want):
        bad = torch.nonzero(snapshot != want).reshape(-1)
        missing = int((mask[bad] & (snapshot[bad] == POISON)).sum())
        stride = vec.engine.obs_stride
        pytest.fail(f"{what}: {bad.numel()} bytes differ ({missing} of them never written), first at byte {int(bad[0])} = page "
                    f"{int(bad[0]) // 4096}, environment {int(bad[0]) // stride} chunk {int(bad[0]) % stride // 16}")


# ---- a. the written set is exactly the live set --------------------------------------------------------------------------
@pytest.mark.parametrize("c", lp.CASES, ids=lp.case_id)
def test_the_written_set_is_the_live_set(torch_mod, pools, c):
    torch = torch_mod
    pool = pools[c.pool]
    ids = lp.case_ids(c, len(pool["oracles"]))
    parts = lp.page_parts(c.pad_h, c.pad_w, lp.case_es(c), pool["heights"], ids)
    live, n_live = parts["live"], int(parts["live"].sum())
    vec, st, view = _retained(pool, c, ids, 3)
    eng = vec.engine
    assert eng.obs_stride == parts["stride"] and eng.obs_bytes == parts["obs_bytes"]
    assert eng.render_kernel.startswith("pw_render_page"), eng.render_kernel
    assert eng.get_option("obs_live_pages") == n_live
    flat = _bytes(torch, st)
    assert flat.numel() == c.B * parts["stride"]
    mask = _byte_mask(torch, vec.device, c, pool["heights"], ids, live, flat.numel())
    assert 0 < int(mask.sum()) <= n_live * 4096  # (the mask itself is checked on the CPU: test_live_pages_host.py)
    g = torch.Generator(device=vec.device).manual_seed(1000 + c.B)
    envs = _sample_envs(parts, c.B)

    def actions():
        return torch.randint(0, 4, (c.B,), generator=g, device=vec.device, dtype=torch.uint8)

    if c.B >= 4096:  # two forms: the list with the exact grid, and with the upper bound behind a re-bind
        forms = [(False, 3, 2, 6, 0), (True, 3, 1, 3, 1)]
    else:
        forms = [(False, form, order, run, load) for form in (3, 2) for order in (0, 1, 2) for run in (0, 3, 6) for load in (0, 1)]
        forms += [(True, 3, order, run, load) for order in (0, 1, 2) for run in (0, 3, 6) for load in (0, 1)]
    state = (False, 3)
    for upper_bound, form, order, run_log2, load_all in forms:
        if (upper_bound, form) != state:
            if upper_bound and not state[0]:
                # a re-bind in-stream (pw_reset on the bound ids) rebuilds the list: its length stays on the device from here on,
                # the launch takes the upper-bound grid and the surplus workgroups return
                eng.reset(vec.puzzle_id, vec.pos, vec.steps, vec.terminated, vec.truncated, None)
                assert eng.get_option("obs_live_pages") == 0
            eng.set_option("obs_padding_once", form)  # (setting the option ends the retention: establish it again)
            eng.render(vec.puzzle_id, vec.pos, st)
            assert eng.get_option("obs_live_pages") == n_live
            state = (upper_bound, form)
        _written_is_live(torch, vec, st, mask, actions(), (order, run_log2, load_all),
                         (lp.case_id(c), upper_bound, form, order, run_log2, load_all))
    assert eng.get_option("obs_live_pages") == n_live
    # the repaired buffer is the full render at this frame: against the oracle
    assert np.array_equal(view[envs].cpu().numpy(), _oracle(pool, c, vec, ids, envs))


# ---- b. twenty random steps with autoreset ----------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [lp.Case("level1", 54, 47, "uint8", 50), lp.Case("level1", 54, 47, "float32", 50),
                               lp.Case("small", 16, 16, "uint8", 300), lp.Case("small", 16, 16, "float32", 300)], ids=lp.case_id)
def test_every_step_equals_the_full_render(torch_mod, pools, c):
    torch = torch_mod
    assert c in lp.CASES
    pool = pools[c.pool]
    ids = lp.case_ids(c, len(pool["oracles"]))
    parts = lp.page_parts(c.pad_h, c.pad_w, lp.case_es(c), pool["heights"], ids)
    n_live = int(parts["live"].sum())
    assert 0 < n_live < parts["n_pages"]
    vec, st, view = _retained(pool, c, ids, 1)
    ref, rst, rview = _retained(pool, c, ids, 0)
    assert vec.engine.get_option("obs_live_pages") == n_live and ref.engine.get_option("obs_live_pages") == 0
    g = torch.Generator(device=vec.device).manual_seed(7 + c.B)
    envs = _sample_envs(parts, c.B)
    for t in range(20):
        a = torch.randint(0, 4, (c.B,), generator=g, device=vec.device, dtype=torch.uint8)
        _step_into(vec, st, a, delta=c.dtype == "uint8" and t % 2 == 1)
        _step_into(ref, rst, a)
        assert torch.equal(view, rview), t
        assert torch.equal(vec.pos, ref.pos) and torch.equal(vec.terminated, ref.terminated) and torch.equal(vec.truncated, ref.truncated)
        if t % 6 == 5:  # (after the autoresets of step 5, 11, 17 too)
            assert np.array_equal(view[envs].cpu().numpy(), _oracle(pool, c, vec, ids, envs)), t
        assert vec.engine.get_option("obs_live_pages") == n_live


# ---- c. the scan's carry ------------------------------------------------------------------------------------------------
def test_the_scan_carries_over_a_million_pages(torch_mod, pools):
    torch = torch_mod
    t0 = time.perf_counter()
    pool = pools["level1"]
    pad_h, pad_w = 51, 42
    _, stride, cpe, _ = lp.frame(pad_h, pad_w, 4)
    B = (1 << 20) * 256 // cpe + 1  # the smallest batch with more than 1 024 x 1 024 pages
    assert stride == 231424 and B == 18559 and -(-(B * cpe) // 256) > 1 << 20 >= -(-((B - 1) * cpe) // 256)
    c = lp.Case("level1", pad_h, pad_w, "float32", B)
    ids = np.random.default_rng(51).integers(0, len(pool["oracles"]), B)
    ids[-1] = lp.BIG  # no padding rows at all: the last pages, whose list offsets start from the carry, are live
    live, _, n_pages, _, _ = lp.pages(pad_h, pad_w, 4, pool["heights"], ids)
    n_live = int(live.sum())
    assert n_pages == 1048584 and -(-n_pages // 1024) == 1025  # one count more than a round of the scan takes
    assert int(live[1 << 20:].sum()) > 0 and n_live % 512 != 0  # live pages behind the first round
    vec, st, view = _retained(pool, c, ids, 3)
    eng, dev = vec.engine, vec.device
    assert eng.get_option("obs_live_pages") == n_live
    flat = _bytes(torch, st)
    live_dev = torch.from_numpy(live).to(dev)
    g = torch.Generator(device=dev).manual_seed(3)
    slab = 1 << 16  # pages per comparison
    for order, run_log2 in ((0, 0), (2, 6)):
        flat.fill_(POISON)
        _set_form(eng, order, run_log2, 0)
        _step_into(vec, st, torch.randint(0, 4, (B,), generator=g, device=dev, dtype=torch.uint8))
        snapshot = flat.clone()
        _set_form(eng, 0, 0, 0)
        eng.render(vec.puzzle_id, vec.pos, st)
        for p0 in range(0, n_pages, slab):
            n = min(slab, n_pages - p0)
            m = lp.written_mask(pad_h, pad_w, 4, pool["heights"], ids, live=live_dev, first_page=p0, count=n, chunks=True,
                                arange=lambda lo, hi: torch.arange(lo, hi, device=dev))
            lo, hi = p0 * 4096, min((p0 + n) * 4096, flat.numel())
            m = m.repeat_interleave(16)[:hi - lo]
            want = torch.where(m, flat[lo:hi], torch.full_like(flat[:1], POISON))
            assert torch.equal(snapshot[lo:hi], want), (order, run_log2, p0)
        del snapshot
    assert eng.get_option("obs_live_pages") == n_live
    envs = [0, B // 2, B - 1]
    assert np.array_equal(view[envs].cpu().numpy(), _oracle(pool, c, vec, ids, envs))
    print(f"\nscan carry: B {B}, {n_pages} pages, {n_live} live, {time.perf_counter() - t0:.2f} s")


# ---- d. slices of the retained buffer --------------------------------------------------------------------------------------
def _slice_case(pools, dtype):
    c = lp.Case("level1", 54, 47, dtype, 50)
    pool = pools[c.pool]
    ids = lp.case_ids(c, len(pool["oracles"])).copy()
    for puzzle, at in ((lp.SMALL, 21), (lp.BIG, 23)):  # the two extremes inside the slice of environments 20 .. 24
        j = int(np.flatnonzero(ids == puzzle)[0])
        ids[j], ids[at] = ids[at], ids[j]
    other = ids.copy()
    other[21], other[23] = lp.BIG, lp.SMALL  # swapped: old pixels lie in the new padding
    return c, pool, ids, other


@pytest.mark.parametrize("how", ["render", "step_render"])
@pytest.mark.parametrize("dtype", ["uint8", "float32"])
def test_a_sub_batch_into_a_slice_ends_the_retention(torch_mod, pools, dtype, how):
    torch = torch_mod
    c, pool, ids, other = _slice_case(pools, dtype)
    n_live = int(lp.pages(c.pad_h, c.pad_w, lp.case_es(c), pool["heights"], ids)[0].sum())
    vec, st, view = _retained(pool, c, ids, 1)
    ref, rst, rview = _retained(pool, c, ids, 0)
    eng, dev = vec.engine, vec.device
    g = torch.Generator(device=dev).manual_seed(17)
    lo, n = 20, 5
    # the second id tensor with state tensors of its own, at the initial states (a pw_reset of ids that are not bound)
    oid = torch.as_tensor(other, dtype=torch.int32).to(dev)
    os_ = eng.alloc_state(c.B)
    eng.reset(oid, os_["pos"], os_["steps"], os_["terminated"], os_["truncated"], None)
    assert eng.get_option("obs_live_pages") == n_live
    sub = {k: v[lo:lo + n] for k, v in os_.items()}
    if how == "render":
        eng.render(oid[lo:lo + n], sub["pos"], st[lo:lo + n])
    else:
        a = torch.randint(0, 4, (n,), generator=g, device=dev, dtype=torch.uint8)
        eng.step_render(oid[lo:lo + n], a, sub["pos"], sub["steps"], sub["reward"], sub["dgoals"], sub["terminated"], sub["truncated"],
                        st[lo:lo + n], 0)
    assert eng.get_option("obs_live_pages") == 0
    # the slice holds the other puzzles now (the big one where the small one's padding was), the rest is untouched
    from oracle import c_oracle

    want = c_oracle.observe_batch(pool["oracles"], other, os_["pos"].cpu().numpy(), [21, 23], c.pad_h, c.pad_w, lp.PPC, lp.BW,
                                  "f32" if dtype == "float32" else "u8")
    assert np.array_equal(view[[21, 23]].cpu().numpy(), want)
    assert torch.equal(view[:lo], rview[:lo]) and torch.equal(view[lo + n:], rview[lo + n:]) and not torch.equal(view, rview)
    for t in range(3):
        a = torch.randint(0, 4, (c.B,), generator=g, device=dev, dtype=torch.uint8)
        _step_into(vec, st, a)
        _step_into(ref, rst, a)
        assert torch.equal(view, rview), t  # (environments 20 .. 24 included: the first of these steps rendered in full)
        assert eng.get_option("obs_live_pages") == n_live  # ... and retained the buffer again
    envs = [20, 21, 23, 24]
    assert np.array_equal(view[envs].cpu().numpy(), _oracle(pool, c, vec, ids, envs))


@pytest.mark.parametrize("dtype", ["uint8", "float32"])
def test_a_sub_batch_into_another_buffer_leaves_the_retention_alone(torch_mod, pools, dtype):
    torch = torch_mod
    c, pool, ids, other = _slice_case(pools, dtype)
    parts = lp.page_parts(c.pad_h, c.pad_w, lp.case_es(c), pool["heights"], ids)
    n_live = int(parts["live"].sum())
    vec, st, view = _retained(pool, c, ids, 1)
    ref, rst, rview = _retained(pool, c, ids, 0)
    eng, dev = vec.engine, vec.device
    st2, view2 = eng.alloc_obs_owned(c.B)
    oid = torch.as_tensor(other, dtype=torch.int32).to(dev)
    os_ = eng.alloc_state(c.B)
    eng.reset(oid, os_["pos"], os_["steps"], os_["terminated"], os_["truncated"], None)
    lo, n = 20, 5
    eng.render(oid[lo:lo + n], os_["pos"][lo:lo + n], st2[lo:lo + n])
    a = torch.zeros((n,), device=dev, dtype=torch.uint8)
    eng.step_render(oid[lo:lo + n], a, os_["pos"][lo:lo + n], os_["steps"][lo:lo + n], os_["reward"][lo:lo + n], os_["dgoals"][lo:lo + n],
                    os_["terminated"][lo:lo + n], os_["truncated"][lo:lo + n], st2[lo:lo + n], 0)
    assert eng.get_option("obs_live_pages") == n_live
    # still the live launch: poisoned pages of padding survive a step, everything else is the twin's
    dead = np.flatnonzero(~parts["live"])
    poisoned = [int(dead[0]), int(dead[dead.size // 2]), int(dead[-1])]
    flat = _bytes(torch, st)
    for p in poisoned:
        flat[p * 4096:(p + 1) * 4096] = POISON
    a = torch.ones((c.B,), device=dev, dtype=torch.uint8)
    _step_into(vec, st, a)
    _step_into(ref, rst, a)
    want = _bytes(torch, rst).clone()
    for p in poisoned:
        want[p * 4096:(p + 1) * 4096] = POISON
    assert torch.equal(flat, want)


# ---- e. capture --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [3, 2], ids=["list", "early-exits"])
def test_captured_steps_replay_the_live_launch(torch_mod, pools, form):
    torch = torch_mod
    c = lp.Case("level1", 54, 47, "uint8", 50)
    pool = pools[c.pool]
    ids = lp.case_ids(c, len(pool["oracles"]))
    parts = lp.page_parts(c.pad_h, c.pad_w, 1, pool["heights"], ids)
    n_live = int(parts["live"].sum())
    vec, st, view = _retained(pool, c, ids, form)
    ref, rst, rview = _retained(pool, c, ids, 0)
    dev = vec.device
    assert vec.engine.get_option("obs_live_pages") == n_live
    K, R = 4, 9
    gen = torch.Generator(device=dev).manual_seed(6)
    acts = torch.randint(0, 4, (R, K, c.B), dtype=torch.uint8, device=dev, generator=gen)
    static_actions = torch.zeros((K, c.B), dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream(device=dev)  # warm-up on a side stream, then capture K steps: a linear chain of launches
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        static_actions.copy_(acts[0])
        for k in range(K):
            _step_into(vec, st, static_actions[k])
    torch.cuda.current_stream(dev).wait_stream(s)
    for k in range(K):
        _step_into(ref, rst, acts[0, k])
    assert torch.equal(view, rview) and vec.engine.get_option("obs_live_pages") == n_live
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for k in range(K):
            _step_into(vec, st, static_actions[k])
    dead = np.flatnonzero(~parts["live"])
    poisoned = [int(dead[1]), int(np.flatnonzero(~parts["whole"] & parts["has_head"] & ~parts["live"])[0])]
    flat = _bytes(torch, st)
    for r in range(1, R):
        static_actions.copy_(acts[r])
        if r == R - 1:  # what was captured is the live launch, not a full render: pages of padding are left alone
            for p in poisoned:
                flat[p * 4096:(p + 1) * 4096] = POISON
        graph.replay()
        for k in range(K):
            _step_into(ref, rst, acts[r, k])
        for name in ("pos", "steps", "reward", "dgoals", "terminated", "truncated"):
            assert torch.equal(getattr(vec, name), getattr(ref, name)), (r, name)
        if r < R - 1:
            assert torch.equal(view, rview), r
    want = _bytes(torch, rst).clone()
    for p in poisoned:
        want[p * 4096:(p + 1) * 4096] = POISON
    assert torch.equal(flat, want)
    assert vec.engine.get_option("obs_live_pages") == n_live

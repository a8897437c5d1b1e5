"""-m gpu: only the changed pages of a retained observation buffer are written (PW_OPT_OBS_CHANGED_PAGES).

Twins as in tests/test_gpu_obs_padding.py: one engine with obs_padding_once 1 + obs_changed_pages 1, one with both 0; the
whole buffers are compared after every step (and sampled environments with the C oracle).  The written set is checked against
tests/changed_pages_restatement.py: every page of the TIGHT set is written, no page outside the WIDE set is, and what is
written equals the reference's bytes."""
import gc
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import changed_pages_restatement as cp  # noqa: E402
import live_pages_restatement as lp  # noqa: E402

pytestmark = pytest.mark.gpu

POISON = 0xAB


@pytest.fixture(scope="module")
def torch_mod():
    import torch

    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch


def _make_pool(texts, frame):
    from oracle import c_oracle
    from pushworld_amd.puzzle import PushWorldPuzzle

    oracles = [c_oracle.COraclePuzzle(t) for t in texts]
    return {"puzzles": [PushWorldPuzzle(text=t) for t in texts], "oracles": oracles, "heights": lp.text_heights(texts),
            "obj_heights": cp.obj_heights_of(oracles), "frame": frame}


@pytest.fixture(scope="module")
def pools():
    return {"level1": _make_pool(lp.level1_texts(), (51, 42)), "small": _make_pool(lp.small_texts(), (16, 16))}


def _ids(pool, B, name):
    n = len(pool["puzzles"])
    if name == "small":
        return np.arange(B, dtype=np.int64) % n
    if B >= n:
        return (np.arange(B, dtype=np.int64) * n) // B
    first = [lp.SMALL, lp.BIG, 2, 8, 26]
    rest = [i for i in range(n) if i not in first]
    return np.array((first + rest)[:B] if B > 1 else [lp.BIG], dtype=np.int64)


def _vec(pool, ids, dtype, on, opts=None, **kw):
    from pushworld_amd.vec_env import VecPushWorld

    pad_h, pad_w = pool["frame"]
    eo = {"bind_min_envs": 1, "obs_padding_once": int(on), "obs_changed_pages": int(on)}
    eo.update(opts or {})
    args = dict(puzzle_ids=ids, max_steps=5, pixels_per_cell=3, border_width=1, observation=dtype, pad_cells=(pad_h, pad_w), device=0,
                autoreset=True, tune=False, bind=True, engine_options=eo)
    args.update(kw)
    return VecPushWorld(pool["puzzles"], len(ids), **args)


def _step_into(vec, st, actions):
    vec.engine.step_render(vec.puzzle_id, actions, vec.pos, vec.steps, vec.reward, vec.dgoals, vec.terminated, vec.truncated, st,
                           vec.flags)


def _bytes(torch, st):
    return st.view(torch.uint8).reshape(-1)


def _twins(pool, ids, dtype, opts=None, **kw):
    """((vec, buffer, view) with both options on, the same with both off): same states, library-owned buffers, rendered."""
    out = []
    for on in (True, False):
        vec = _vec(pool, ids, dtype, on, opts, **kw)
        vec.reset()
        st, view = vec.engine.alloc_obs_owned(len(ids))
        vec.engine.render(vec.puzzle_id, vec.pos, st)
        out.append((vec, st, view))
    return out[0], out[1]


def _oracle(pool, vec, ids, envs, dtype):
    from oracle import c_oracle

    pad_h, pad_w = pool["frame"]
    return c_oracle.observe_batch(pool["oracles"], ids, vec.states(), envs, pad_h, pad_w, 3, 1, "f32" if dtype == "float32" else "u8")


def _sets(pool, ids, es, before, after):
    pad_h, pad_w = pool["frame"]
    rows = cp.changed_rows(pool["obj_heights"], ids, pool["heights"], before, after)
    return cp.page_sets(pad_h, pad_w, es, pool["heights"], ids, rows)


def _host_pages(torch, st, n_pages):
    """uint8 [n_pages, 4096]: the buffer page by page on the host (what lies behind the last environment reads as poison)."""
    out = np.full(n_pages * 4096, POISON, np.uint8)
    raw = _bytes(torch, st).cpu().numpy()
    out[:raw.size] = raw
    return out.reshape(n_pages, 4096)


def _step_and_form(torch, pool, pair, ids, es, a):
    """Steps both twins with the whole buffer of the first one poisoned; True when the step left some live page alone (the
    changed form), False when it rewrote every live page (the live or the full launch).  What the step left alone holds its
    bytes again afterwards."""
    (vec, st, view), (ref, rst, rview) = pair
    pad_h, pad_w = pool["frame"]
    live, _, n_pages, _, _ = lp.pages(pad_h, pad_w, es, pool["heights"], ids)
    flat = _bytes(torch, st)
    keep = flat.clone()
    flat.fill_(POISON)
    _step_into(vec, st, a)
    _step_into(ref, rst, a)
    left = flat == POISON
    survived = (_host_pages(torch, st, n_pages) == POISON).all(axis=1) & live
    flat[left] = keep[left]
    return bool(survived.any())


def _rand(torch, g, vec, B):
    return torch.randint(0, 4, (B,), generator=g, device=vec.device, dtype=torch.uint8)


# ---- equality and oracle -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,B,dtype", [("level1", 1, "uint8"), ("level1", 3, "uint8"), ("level1", 50, "uint8"),
                                          ("level1", 1, "float32"), ("level1", 3, "float32"), ("level1", 50, "float32"),
                                          ("small", 300, "uint8"), ("small", 300, "float32"), ("level1", 4096, "uint8")])
def test_every_step_equals_the_reference(torch_mod, pools, name, B, dtype):
    torch = torch_mod
    pool = pools[name]
    ids = _ids(pool, B, name)
    (vec, st, view), (ref, rst, rview) = _twins(pool, ids, dtype)
    assert vec.engine.get_option("obs_changed_pages") == 1 and ref.engine.get_option("obs_changed_pages") == 0
    if name == "small" and dtype == "uint8":
        assert vec.engine.obs_stride == 7168  # (1.75 pages per environment: three pages in four straddle two environments)
    g = torch.Generator(device=vec.device).manual_seed(3 + B)
    envs = sorted({0, B // 2, B - 1, min(1, B - 1)})
    for t in range(24):
        a = _rand(torch, g, vec, B)
        _step_into(vec, st, a)
        _step_into(ref, rst, a)
        assert torch.equal(view, rview), t
        assert torch.equal(vec.pos, ref.pos) and torch.equal(vec.terminated, ref.terminated) and torch.equal(vec.truncated, ref.truncated)
        if t % 6 == 5:  # (after the autoresets of step 5, 11, 17, 23 too)
            assert np.array_equal(view[envs].cpu().numpy(), _oracle(pool, vec, ids, envs, dtype)), t


# ---- the written set -----------------------------------------------------------------------------------------------------
def _check_written_set(torch, pool, pair, ids, dtype, a, tag):
    (vec, st, view), (ref, rst, rview) = pair
    es = 1 if dtype == "uint8" else 4
    pad_h, pad_w = pool["frame"]
    before = vec.states()
    flat = _bytes(torch, st)
    flat.fill_(POISON)
    _step_into(vec, st, a)
    _step_into(ref, rst, a)
    tight, wide, live = _sets(pool, ids, es, before, vec.states())
    n_pages = len(live)
    got = _host_pages(torch, st, n_pages)
    touched = (got != POISON).any(axis=1)
    assert not (tight & ~touched).any(), (tag, "a page of the tight set kept its poison", int(np.flatnonzero(tight & ~touched)[0]))
    assert not (touched & ~wide).any(), (tag, "a page outside the wide set was written", int(np.flatnonzero(touched & ~wide)[0]))
    stored = lp.written_mask(pad_h, pad_w, es, pool["heights"], ids, live=touched).reshape(n_pages, 4096)
    want = np.where(stored, _host_pages(torch, rst, n_pages), POISON)
    assert np.array_equal(got, want), tag
    vec.engine.render(vec.puzzle_id, vec.pos, st)  # repair
    assert torch.equal(view, rview), tag
    return int(touched.sum()), int(tight.sum())


@pytest.mark.parametrize("dtype", ["uint8", "float32"])
def test_the_written_set_in_every_launch_configuration(torch_mod, pools, dtype):
    torch = torch_mod
    pool, B = pools["level1"], 50
    ids = _ids(pool, B, "level1")
    pair = _twins(pool, ids, dtype)
    vec = pair[0][0]
    g = torch.Generator(device=vec.device).manual_seed(17)
    some = 0
    for order in (0, 1, 2):
        for run_log2 in (0, 3, 6):
            for load_all in (0, 1):
                for k, v in (("page_order", order), ("page_run_log2", run_log2), ("page_load_all", load_all)):
                    vec.engine.set_option(k, v)
                touched, tight = _check_written_set(torch, pool, pair, ids, dtype, _rand(torch, g, vec, B), (order, run_log2, load_all))
                some += tight
                assert touched < int(vec.engine.get_option("obs_live_pages"))  # (not the live launch)
    assert some > 0


@pytest.mark.parametrize("B", [50, 4096])
def test_the_written_set_with_the_upper_bound_grid(torch_mod, pools, B):
    """After a re-bind in-stream (pw_reset on the bound ids) the list's length is known to the device only."""
    torch = torch_mod
    pool = pools["level1"]
    ids = _ids(pool, B, "level1")
    pair = _twins(pool, ids, "uint8")
    for v, s, _ in pair:
        v.engine.reset(v.puzzle_id, v.pos, v.steps, v.terminated, v.truncated, None)  # rebuilds the list behind itself
        v.engine.render(v.puzzle_id, v.pos, s)
    vec = pair[0][0]
    g = torch.Generator(device=vec.device).manual_seed(B)
    for order, run_log2 in ((0, 0), (1, 0), (2, 3)):
        vec.engine.set_option("page_order", order)
        vec.engine.set_option("page_run_log2", run_log2)
        touched, tight = _check_written_set(torch, pool, pair, ids, "uint8", _rand(torch, g, vec, B), (order, run_log2))
        assert 0 < tight <= touched


def test_a_step_without_a_move_writes_nothing(torch_mod, pools):
    torch = torch_mod
    pool = pools["level1"]
    ids, acts = [], []
    for p, o in enumerate(pool["oracles"]):  # puzzles whose agent stands against something at the start
        init = tuple(tuple(int(v) for v in xy) for xy in o.initial_state)
        blocked = [a for a in range(4) if o.get_next_state(init, a) == init]
        if blocked and len(ids) < 8:
            ids.append(p)
            acts.append(blocked[0])
    assert len(ids) == 8
    ids = np.array(ids, dtype=np.int64)
    (vec, st, view), (ref, rst, rview) = _twins(pool, ids, "uint8")
    before = vec.states()
    a = torch.as_tensor(np.array(acts, np.uint8), device=vec.device)
    flat = _bytes(torch, st)
    flat.fill_(POISON)
    _step_into(vec, st, a)
    _step_into(ref, rst, a)
    assert np.array_equal(before, vec.states()) and torch.equal(vec.pos, ref.pos)  # (the restatement: nothing moved)
    assert bool((flat == POISON).all())
    vec.engine.render(vec.puzzle_id, vec.pos, st)
    assert torch.equal(view, rview)


# ---- positions that change behind the engine's back ---------------------------------------------------------------------
@pytest.mark.parametrize("how", ["set_states", "masked reset", "step without a render", "write into pos"])
def test_position_changes_behind_the_engines_back(torch_mod, pools, how):
    torch = torch_mod
    pool, B = pools["level1"], 50
    ids = _ids(pool, B, "level1")
    pair = _twins(pool, ids, "uint8")
    (vec, st, view), (ref, rst, rview) = pair
    g = torch.Generator(device=vec.device).manual_seed(23)
    for _ in range(3):
        a = _rand(torch, g, vec, B)
        _step_into(vec, st, a)
        _step_into(ref, rst, a)
    assert torch.equal(view, rview)
    e_big = int(np.flatnonzero(ids == lp.BIG)[0])
    for v in (vec, ref):
        if how == "set_states":
            pos = v.states()
            pos[:, :] = cp.positions_of(pool["oracles"], ids, [pool["oracles"][p].initial_state for p in ids], pos.shape[1])
            v.set_states(pos)
        elif how == "masked reset":
            mask = torch.zeros((B,), dtype=torch.uint8, device=v.device)
            mask[::3] = 1
            v.engine.reset(v.puzzle_id, v.pos, v.steps, v.terminated, v.truncated, mask)
        elif how == "step without a render":
            a2 = torch.full((B,), 1, dtype=torch.uint8, device=v.device)
            v.engine.step(v.puzzle_id, a2, v.pos, v.steps, v.reward, v.dgoals, v.terminated, v.truncated, v.flags)
        else:
            o = pool["oracles"][lp.BIG]
            v.pos[e_big, 0, 0] = int(o.initial_state[0][0])
            v.pos[e_big, 0, 1] = int(o.initial_state[0][1])
    a = _rand(torch, g, vec, B)
    # still the changed form, since nothing told the engine -- but pw_reset on the bound ids re-binds behind itself, which ends
    # the retention as ever: a full render, then the changed form again
    assert _step_and_form(torch, pool, pair, ids, 1, a) == (how != "masked reset")
    if how == "masked reset":
        assert torch.equal(view, rview)
        assert _step_and_form(torch, pool, pair, ids, 1, _rand(torch, g, vec, B))
    assert torch.equal(view, rview) and torch.equal(vec.pos, ref.pos)
    envs = sorted({0, e_big, B - 1})
    assert np.array_equal(view[envs].cpu().numpy(), _oracle(pool, vec, ids, envs, "uint8"))


# ---- interleavings -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["delta", "second buffer", "tune_render", "obs_changed_pages", "obs_padding_once", "set_puzzle_ids",
                                  "unbind", "new buffer"])
def test_interleavings(torch_mod, pools, what):
    """The thing, then two steps: equal after each, and the form each took (True = the changed pages only)."""
    torch = torch_mod
    pool, B = pools["level1"], 50
    ids = _ids(pool, B, "level1")
    pair = _twins(pool, ids, "uint8")
    (vec, st, view), (ref, rst, rview) = pair
    e_big = int(np.flatnonzero(ids == lp.BIG)[0])
    g = torch.Generator(device=vec.device).manual_seed(31)
    assert _step_and_form(torch, pool, pair, ids, 1, _rand(torch, g, vec, B))  # the changed form to start with
    assert torch.equal(view, rview)
    a = _rand(torch, g, vec, B)
    forms = [False, True]  # most of them: the live (or full) launch once, then the changed pages again
    if what == "delta":
        for v, s in ((vec, st), (ref, rst)):
            v.engine.step_render_delta(v.puzzle_id, a, v.pos, v.steps, v.reward, v.dgoals, v.terminated, v.truncated, s, v.flags)
    elif what == "second buffer":  # (library-owned too: the retention moves there, and back with the next step into the first)
        other = [v.engine.alloc_obs_owned(B) for v in (vec, ref)]
        for v, (s2, _) in zip((vec, ref), other):
            v.engine.render(v.puzzle_id, v.pos, s2)
        assert torch.equal(other[0][1], other[1][1])
    elif what == "tune_render":
        for v, s in ((vec, st), (ref, rst)):
            v.engine.tune_render(v.puzzle_id, v.pos, s)
        forms = [True, True]  # (it ends with the buffer showing pos and says so)
    elif what in ("obs_changed_pages", "obs_padding_once"):
        vec.engine.set_option(what, 1)
    elif what == "set_puzzle_ids":
        new_ids = ids.copy()
        i_small = int(np.flatnonzero(ids == lp.SMALL)[0])
        new_ids[i_small], new_ids[e_big] = lp.BIG, lp.SMALL
        for v in (vec, ref):
            v.set_puzzle_ids(new_ids)
            v.engine.reset(v.puzzle_id, v.pos, v.steps, v.terminated, v.truncated, None)
        ids, e_big = new_ids, i_small
    elif what == "unbind":
        vec.engine.unbind()
        forms = [False, False]  # (nothing is retained without a binding)
    else:
        pair = None
        del st, view
        gc.collect()  # pw_obs_free
        st, view = vec.engine.alloc_obs_owned(B)
        _bytes(torch, st).fill_(POISON)
        pair = ((vec, st, view), (ref, rst, rview))
    got = []
    for _ in range(2):
        got.append(_step_and_form(torch, pool, pair, ids, 1, _rand(torch, g, vec, B)))
        assert torch.equal(view, rview), (what, got)
    assert got == forms, what
    envs = sorted({0, e_big, B - 1})
    assert np.array_equal(view[envs].cpu().numpy(), _oracle(pool, vec, ids, envs, "uint8"))


# ---- every record writer -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def levels_pool():
    from pushworld_amd import benchmark_data as bd

    texts = []
    for lv in (1, 2, 3, 4):  # 223 puzzles, up to 19 movables: N_pad 32
        for p in bd.level_paths(lv):
            with open(p) as f:
                texts.append(f.read())
    from pushworld_amd.puzzle import PushWorldPuzzle

    return {"puzzles": [PushWorldPuzzle(text=t) for t in texts], "texts": texts}


@pytest.mark.parametrize("opts", [{"bind_lanes": 2}, {"bind_lanes": 3}, {"bind_lanes": 4}, {"bind_min_envs": 10000},
                                  {"step_kernel": 1}, {"step_kernel": 2}, {}],
                         ids=["2 lanes", "4 lanes", "8 lanes", "lane groups", "wavefront kernel", "lane kernel", "default"])
def test_every_record_writer_on_an_n_pad_32_set(torch_mod, levels_pool, opts):
    torch = torch_mod
    from oracle import c_oracle
    from pushworld_amd.vec_env import VecPushWorld

    n = len(levels_pool["puzzles"])
    B = 2 * n
    ids = (np.arange(B, dtype=np.int64) * n) // B
    vecs = []
    for on in (True, False):
        eo = {"bind_min_envs": 1, "obs_padding_once": int(on), "obs_changed_pages": int(on)}
        eo.update(opts)
        vec = VecPushWorld(levels_pool["puzzles"], B, puzzle_ids=ids, max_steps=5, pixels_per_cell=3, border_width=1,
                           observation="uint8", device=0, autoreset=True, tune=False, bind=True, engine_options=eo)
        assert vec.pos.shape[1] == 32
        vec.reset()
        st, view = vec.engine.alloc_obs_owned(B)
        vec.engine.render(vec.puzzle_id, vec.pos, st)
        vecs.append((vec, st, view))
    (vec, st, view), (ref, rst, rview) = vecs
    g = torch.Generator(device=vec.device).manual_seed(41)
    flat = _bytes(torch, st)
    for t in range(12):
        a = _rand(torch, g, vec, B)
        if t == 3:  # the changed form is the one running: a step leaves most of a poisoned buffer alone
            keep = flat.clone()
            flat.fill_(POISON)
        _step_into(vec, st, a)
        _step_into(ref, rst, a)
        if t == 3:
            left = flat == POISON
            assert int(left.sum()) > flat.numel() // 2
            flat[left] = keep[left]
        assert torch.equal(view, rview) and torch.equal(vec.pos, ref.pos), t
    envs = [0, B // 2, B - 1]
    sel = sorted(set(ids[envs].tolist()))
    oracles = [c_oracle.COraclePuzzle(levels_pool["texts"][p]) for p in sel]
    h, w, _ = vec.engine.obs_shape
    want = c_oracle.observe_batch(oracles, [sel.index(int(ids[e])) for e in envs], vec.states()[envs], np.arange(len(envs)), h // 3, w // 3, 3, 1, "u8")
    assert np.array_equal(view[envs].cpu().numpy(), want)


# ---- graph capture -------------------------------------------------------------------------------------------------------
def test_a_captured_step_replays_the_changed_form(torch_mod, pools):
    torch = torch_mod
    pool, B = pools["level1"], 50
    ids = _ids(pool, B, "level1")
    (vec, st, view), (ref, rst, rview) = _twins(pool, ids, "uint8")
    dev = vec.device
    gen = torch.Generator(device=dev).manual_seed(6)
    static_a = torch.zeros((B,), dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):  # warm-up on a side stream
        a = _rand(torch, gen, vec, B)
        static_a.copy_(a)
        _step_into(vec, st, static_a)
    torch.cuda.current_stream(dev).wait_stream(s)
    _step_into(ref, rst, a)
    assert torch.equal(view, rview)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _step_into(vec, st, static_a)
    _step_into(ref, rst, a)  # (the captured launches run during capture on this runtime or not: settle it with a full render)
    vec.pos.copy_(ref.pos)
    vec.steps.copy_(ref.steps)
    vec.terminated.copy_(ref.terminated)
    vec.truncated.copy_(ref.truncated)
    vec.engine.render(vec.puzzle_id, vec.pos, st)
    assert torch.equal(view, rview)
    flat = _bytes(torch, st)
    for r in range(6):
        a = _rand(torch, gen, vec, B)
        static_a.copy_(a)
        if r == 2:
            keep = flat.clone()
            flat.fill_(POISON)
        graph.replay()
        _step_into(ref, rst, a)
        if r == 2:  # the replay is the changed form: most of the buffer is left alone
            left = flat == POISON
            assert int(left.sum()) > flat.numel() // 2
            flat[left] = keep[left]
        assert torch.equal(view, rview) and torch.equal(vec.pos, ref.pos), r
    envs = [0, 1, B - 1]
    assert np.array_equal(view[envs].cpu().numpy(), _oracle(pool, vec, ids, envs, "uint8"))


# ---- the library's own buffer --------------------------------------------------------------------------------------------
def test_vec_env_turns_it_on_for_its_own_buffer(torch_mod, pools):
    torch = torch_mod
    from pushworld_amd.vec_env import VecPushWorld

    pool, B = pools["level1"], 50
    ids = _ids(pool, B, "level1")
    args = dict(puzzle_ids=ids, max_steps=5, pixels_per_cell=3, border_width=1, observation="uint8", device=0, autoreset=True,
                tune=True, tune_allocations=1)
    want = {"default": (1, 1), "changed off": (1, 0), "padding off": (0, 0), "padding given": (1, 0), "torch buffer": (0, 0)}
    opts = {"default": {}, "changed off": {"obs_changed_pages": 0}, "padding off": {"obs_padding_once": 0},
            "padding given": {"obs_padding_once": 1}, "torch buffer": {}}
    vecs = {}
    for k in want:
        eo = dict({"bind_min_envs": 1}, **opts[k])
        vecs[k] = VecPushWorld(pool["puzzles"], B, engine_options=eo, **dict(args, tune=k != "torch buffer"))
        got = (vecs[k].engine.get_option("obs_padding_once"), vecs[k].engine.get_option("obs_changed_pages"))
        assert got == want[k], (k, got)
        vecs[k].reset()
    g = torch.Generator(device=vecs["default"].device).manual_seed(21)
    for t in range(12):
        a = _rand(torch, g, vecs["default"], B)
        for v in vecs.values():
            v.step(a)
        for k, v in vecs.items():
            assert torch.equal(v.obs, vecs["padding off"].obs), (k, t)
    envs = [0, 1, B - 1]
    assert np.array_equal(vecs["default"].obs[envs].cpu().numpy(), _oracle(pool, vecs["default"], ids, envs, "uint8"))
    with pytest.raises(ValueError):
        vecs["default"].engine.set_option("obs_changed_pages", 2)

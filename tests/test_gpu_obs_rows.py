"""-m gpu: only the changed pixel rows of a retained observation buffer are written (pw_engine_set_obs_changed_rows on top of
PW_OPT_OBS_CHANGED_PAGES).

Twins as in tests/test_gpu_obs_changed.py: one engine with obs_padding_once 1 + obs_changed_pages 1 + the row switch, one with
all of them off; the whole buffers are compared after every step (and sampled environments with the C oracle).  The written set
is checked chunk by chunk against tests/changed_rows_restatement.py: every chunk of the TIGHT set is written, no chunk outside
the WIDE set is, and every written chunk is whole and equals the reference's."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import changed_pages_restatement as cp  # noqa: E402
import changed_rows_restatement as cr  # noqa: E402
import live_pages_restatement as lp  # noqa: E402
import test_gpu_obs_changed as oc  # noqa: E402  (its pools, twins and helpers)

pytestmark = pytest.mark.gpu

POISON = oc.POISON
torch_mod = oc.torch_mod
pools = oc.pools
levels_pool = oc.levels_pool


def _twins(pool, ids, dtype, opts=None, **kw):
    pair = oc._twins(pool, ids, dtype, opts, **kw)
    pair[0][0].engine.obs_changed_rows = True
    assert pair[0][0].engine.obs_changed_rows and not pair[1][0].engine.obs_changed_rows
    return pair


def _chunks(torch, st, B, cpe):
    """uint8 [B, cpe, 16]: the buffer chunk by chunk on the host."""
    return oc._bytes(torch, st).cpu().numpy()[:B * cpe * lp.CHUNK].reshape(B, cpe, lp.CHUNK)


def _poisoned_step(torch, pool, pair, ids, es, a, shown=None):
    """Steps both twins with the whole buffer of the first poisoned.  Returns (touched [B, cpe], tight, wide) and leaves the
    buffer repaired (what the step left alone gets its bytes back); every written chunk is whole and equals the twin's.
    shown: the positions the buffer shows when they are not the state before the step."""
    (vec, st, view), (ref, rst, rview) = pair
    pad_h, pad_w = pool["frame"]
    B = len(ids)
    cpe = lp.frame(pad_h, pad_w, es)[2]
    before = vec.states() if shown is None else shown
    flat = oc._bytes(torch, st)
    keep = flat.clone()
    flat.fill_(POISON)
    oc._step_into(vec, st, a)
    oc._step_into(ref, rst, a)
    rows = cp.changed_rows(pool["obj_heights"], ids, pool["heights"], before, vec.states())
    tight, wide = cr.chunk_sets(pad_h, pad_w, es, pool["heights"], ids, rows)
    got, want = _chunks(torch, st, B, cpe), _chunks(torch, rst, B, cpe)
    touched = (got != POISON).any(axis=2)
    assert np.array_equal(got[touched], want[touched]), "a written chunk is not whole or differs from the reference"
    left = flat == POISON
    flat[left] = keep[left]
    return touched, tight, wide


def _partial_pages(touched, n_chunks):
    """Pages of which a step wrote some image chunks and left others (the page forms never do)."""
    B, cpe = touched.shape
    image = np.zeros((B, cpe), bool)
    image[:, :n_chunks] = True
    n_pages = -(-B * cpe // lp.PAGE_CHUNKS)
    t = np.zeros(n_pages * lp.PAGE_CHUNKS, bool)
    i = np.zeros(n_pages * lp.PAGE_CHUNKS, bool)
    t[:B * cpe], i[:B * cpe] = touched.reshape(-1), image.reshape(-1)
    t, i = t.reshape(n_pages, -1), i.reshape(n_pages, -1)
    return int((t.any(axis=1) & (i & ~t).any(axis=1)).sum())


# ---- equality and oracle -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,B,dtype", [("level1", 1, "uint8"), ("level1", 3, "uint8"), ("level1", 5, "uint8"), ("level1", 50, "uint8"),
                                          ("level1", 1, "float32"), ("level1", 3, "float32"), ("level1", 5, "float32"),
                                          ("level1", 50, "float32"), ("small", 300, "uint8"), ("small", 300, "float32")])
def test_every_step_equals_the_reference(torch_mod, pools, name, B, dtype):
    torch = torch_mod
    pool = pools[name]
    ids = oc._ids(pool, B, name)
    (vec, st, view), (ref, rst, rview) = _twins(pool, ids, dtype)
    assert vec.engine.get_option("obs_changed_pages") == 1 and ref.engine.get_option("obs_changed_pages") == 0
    if name == "small" and dtype == "uint8":
        assert vec.engine.obs_stride == 7168
    g = torch.Generator(device=vec.device).manual_seed(3 + B)
    envs = sorted({0, B // 2, B - 1, min(1, B - 1)})
    for t in range(24):
        a = oc._rand(torch, g, vec, B)
        oc._step_into(vec, st, a)
        oc._step_into(ref, rst, a)
        assert torch.equal(view, rview), t
        assert torch.equal(vec.pos, ref.pos) and torch.equal(vec.terminated, ref.terminated) and torch.equal(vec.truncated, ref.truncated)
        if t % 6 == 5:  # (after the autoresets of step 5, 11, 17, 23 too)
            assert np.array_equal(view[envs].cpu().numpy(), oc._oracle(pool, vec, ids, envs, dtype)), t


# ---- the written set, chunk by chunk ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,B,dtype", [("level1", 50, "uint8"), ("level1", 50, "float32"), ("small", 300, "uint8")])
def test_the_written_set_chunk_by_chunk(torch_mod, pools, name, B, dtype):
    torch = torch_mod
    pool = pools[name]
    ids = oc._ids(pool, B, name)
    es = 1 if dtype == "uint8" else 4
    pair = _twins(pool, ids, dtype)
    (vec, st, view), (ref, rst, rview) = pair
    n_chunks = lp.frame(*pool["frame"], es)[3]
    g = torch.Generator(device=vec.device).manual_seed(17)
    some = partial = 0
    for t in range(8):  # (max_steps 5: the autoresets of step 5 are among them)
        touched, tight, wide = _poisoned_step(torch, pool, pair, ids, es, oc._rand(torch, g, vec, B))
        assert not (tight & ~touched).any(), (t, "a chunk of the tight set kept its poison", np.argwhere(tight & ~touched)[0])
        assert not (touched & ~wide).any(), (t, "a chunk outside the wide set was written", np.argwhere(touched & ~wide)[0])
        assert torch.equal(view, rview), t
        some += int(tight.sum())
        partial += _partial_pages(touched, n_chunks)
    assert some > 0 and partial > 0  # (rows, not pages)


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
    oc._step_into(vec, st, torch.as_tensor(np.array(acts, np.uint8), device=vec.device))  # (the first step: the live launch; shown = pos)
    oc._step_into(ref, rst, torch.as_tensor(np.array(acts, np.uint8), device=vec.device))
    before = vec.states()
    a = torch.as_tensor(np.array(acts, np.uint8), device=vec.device)
    flat = oc._bytes(torch, st)
    flat.fill_(POISON)
    oc._step_into(vec, st, a)
    oc._step_into(ref, rst, a)
    assert np.array_equal(before, vec.states()) and torch.equal(vec.pos, ref.pos)  # (the restatement: nothing moved)
    assert bool((flat == POISON).all())
    vec.engine.render(vec.puzzle_id, vec.pos, st)
    assert torch.equal(view, rview)


# ---- positions that change behind the engine's back ---------------------------------------------------------------------
@pytest.mark.parametrize("how", ["write into pos", "set_states", "state-only step, then render_retained"])
def test_position_changes_behind_the_engines_back(torch_mod, pools, how):
    torch = torch_mod
    pool, B = pools["level1"], 50
    ids = oc._ids(pool, B, "level1")
    pair = _twins(pool, ids, "uint8")
    (vec, st, view), (ref, rst, rview) = pair
    g = torch.Generator(device=vec.device).manual_seed(23)
    for _ in range(3):
        a = oc._rand(torch, g, vec, B)
        oc._step_into(vec, st, a)
        oc._step_into(ref, rst, a)
    assert torch.equal(view, rview)
    e_big = int(np.flatnonzero(ids == lp.BIG)[0])
    shown = vec.states()  # what the buffer shows, whatever happens to pos now
    for v in (vec, ref):
        if how == "set_states":
            pos = v.states()
            pos[:, :] = cp.positions_of(pool["oracles"], ids, [pool["oracles"][p].initial_state for p in ids], pos.shape[1])
            v.set_states(pos)
        elif how == "write into pos":
            o = pool["oracles"][lp.BIG]
            v.pos[e_big, 0, 0] = int(o.initial_state[0][0])
            v.pos[e_big, 0, 1] = int(o.initial_state[0][1])
        else:
            a2 = torch.full((B,), 1, dtype=torch.uint8, device=v.device)
            v.engine.step(v.puzzle_id, a2, v.pos, v.steps, v.reward, v.dgoals, v.terminated, v.truncated, v.flags)
    if how.startswith("state-only"):
        flat = oc._bytes(torch, st)
        keep = flat.clone()
        flat.fill_(POISON)
        vec.engine.render(vec.puzzle_id, vec.pos, st, retained=True)
        ref.engine.render(ref.puzzle_id, ref.pos, rst, retained=True)
        left = flat == POISON
        assert int(left.sum()) > flat.numel() // 2  # (the changed rows only)
        flat[left] = keep[left]
        assert torch.equal(view, rview)
        shown = None  # (the render told the engine)
    touched, tight, wide = _poisoned_step(torch, pool, pair, ids, 1, oc._rand(torch, g, vec, B), shown)
    assert not (tight & ~touched).any() and not (touched & ~wide).any()  # still the changed rows: nothing told the engine
    assert torch.equal(view, rview) and torch.equal(vec.pos, ref.pos)
    envs = sorted({0, e_big, B - 1})
    assert np.array_equal(view[envs].cpu().numpy(), oc._oracle(pool, vec, ids, envs, "uint8"))


# ---- every record writer -----------------------------------------------------------------------------------------------
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
        vec.engine.obs_changed_rows = on
        vec.reset()
        st, view = vec.engine.alloc_obs_owned(B)
        vec.engine.render(vec.puzzle_id, vec.pos, st)
        vecs.append((vec, st, view))
    (vec, st, view), (ref, rst, rview) = vecs
    g = torch.Generator(device=vec.device).manual_seed(41)
    flat = oc._bytes(torch, st)
    for t in range(12):
        a = oc._rand(torch, g, vec, B)
        if t == 3:  # the changed form is the one running: a step leaves most of a poisoned buffer alone
            keep = flat.clone()
            flat.fill_(POISON)
        oc._step_into(vec, st, a)
        oc._step_into(ref, rst, a)
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


# ---- geometry edge cases -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["uint8", "float32"])
def test_a_y_outside_the_mask_and_an_object_taller_than_one_pass(torch_mod, pools, dtype):
    torch = torch_mod
    pool = pools["level1"]
    tall = [(p, j) for p, hs in enumerate(pool["obj_heights"]) for j, h in enumerate(hs) if h > 3 and j > 0]
    assert tall
    p_tall, j_tall = tall[0]
    ids = np.array([lp.BIG, p_tall, lp.SMALL, p_tall, 2], dtype=np.int64)
    es = 1 if dtype == "uint8" else 4
    pair = _twins(pool, ids, dtype)
    (vec, st, view), (ref, rst, rview) = pair
    B = len(ids)
    noop = torch.full((B,), 0, dtype=torch.uint8, device=vec.device)
    oc._step_into(vec, st, noop)  # (the live launch; from here on the changed rows)
    oc._step_into(ref, rst, noop)
    assert torch.equal(view, rview)
    y_was = [int(vec.pos[0, 0, 1]), int(vec.pos[4, 0, 1])]
    h_agent = [int(pool["obj_heights"][ids[e]][0]) for e in (0, 4)]
    for y_out in (-1, 70, None):  # (-1: the agent's last row one above the grid -- nothing of it inside, whatever its height)
        for v in (vec, ref):
            if y_out is None:  # the tall object one column to the side, and the others back where they stood
                v.pos[1, j_tall, 0] += 1
                v.pos[0, 0, 1] = y_was[0]
                v.pos[4, 0, 1] = y_was[1]
            else:              # every row of environments 0 and 4: several passes at 51 x 42
                v.pos[0, 0, 1] = y_out if y_out > 0 else -h_agent[0]
                v.pos[4, 0, 1] = y_out if y_out > 0 else -h_agent[1]
        before = vec.states()
        flat = oc._bytes(torch, st)
        keep = flat.clone()
        flat.fill_(POISON)
        vec.engine.render(vec.puzzle_id, vec.pos, st, retained=True)
        ref.engine.render(ref.puzzle_id, ref.pos, rst, retained=True)
        left = flat == POISON
        flat[left] = keep[left]
        diff = (oc._bytes(torch, st) != oc._bytes(torch, rst)).nonzero().reshape(-1)
        assert diff.numel() == 0, (y_out, int(diff.numel()), [divmod(int(d), vec.engine.obs_stride) for d in diff[:4]])
        pad_h, pad_w = pool["frame"]
        cpe = lp.frame(pad_h, pad_w, es)[2]
        touched = ~left.cpu().numpy()[:B * cpe * lp.CHUNK].reshape(B, cpe, lp.CHUNK).all(axis=2)
        if y_out is None:
            assert touched[1].sum() * lp.CHUNK > 4096 and not touched[2].any() and not touched[3].any()  # more than one pass
        else:
            own = lp.own_chunks(pad_h, pad_w, es, int(pool["heights"][ids[0]]))
            assert touched[0, own[0] + 1:own[1] - 1].all() and not touched[1:4].any()  # all rows of the puzzle
        assert before.shape == vec.states().shape
    envs = [0, 4]
    assert np.array_equal(view[envs].cpu().numpy(), oc._oracle(pool, vec, ids, envs, dtype))


# ---- the switch ----------------------------------------------------------------------------------------------------------
def test_the_switch_between_steps(torch_mod, pools):
    torch = torch_mod
    pool, B = pools["level1"], 50
    ids = oc._ids(pool, B, "level1")
    pair = _twins(pool, ids, "uint8")
    (vec, st, view), (ref, rst, rview) = pair
    n_chunks = lp.frame(*pool["frame"], 1)[3]
    g = torch.Generator(device=vec.device).manual_seed(5)
    _poisoned_step(torch, pool, pair, ids, 1, oc._rand(torch, g, vec, B))  # (the live launch)
    partial = {True: 0, False: 0}
    for on in (True, False, True, False, True):
        vec.engine.obs_changed_rows = on
        assert vec.engine.obs_changed_rows == on
        for _ in range(2):
            touched, tight, wide = _poisoned_step(torch, pool, pair, ids, 1, oc._rand(torch, g, vec, B))
            assert not (tight & ~touched).any()
            assert torch.equal(view, rview), on
            if on:
                assert not (touched & ~wide).any()
            n = _partial_pages(touched, n_chunks)
            assert on or n == 0  # (the page form writes its pages whole)
            partial[on] += n
    assert partial[True] > 0


def test_the_switch_alone_changes_nothing(torch_mod, pools):
    """On with obs_changed_pages 0: the live launch as ever."""
    torch = torch_mod
    pool, B = pools["level1"], 50
    ids = oc._ids(pool, B, "level1")
    pair = oc._twins(pool, ids, "uint8", {"obs_changed_pages": 0})
    (vec, st, view), (ref, rst, rview) = pair
    vec.engine.obs_changed_rows = True
    assert vec.engine.get_option("obs_padding_once") == 1 and vec.engine.get_option("obs_changed_pages") == 0
    g = torch.Generator(device=vec.device).manual_seed(9)
    for t in range(4):
        assert not oc._step_and_form(torch, pool, pair, ids, 1, oc._rand(torch, g, vec, B))  # every live page is rewritten
        assert torch.equal(view, rview), t


# ---- graph capture -------------------------------------------------------------------------------------------------------
def test_a_captured_step_replays_the_changed_rows(torch_mod, pools):
    torch = torch_mod
    pool, B = pools["level1"], 50
    ids = oc._ids(pool, B, "level1")
    (vec, st, view), (ref, rst, rview) = _twins(pool, ids, "uint8")
    dev = vec.device
    gen = torch.Generator(device=dev).manual_seed(6)
    static_a = torch.zeros((B,), dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream(device=dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):  # warm-up on a side stream
        a = oc._rand(torch, gen, vec, B)
        static_a.copy_(a)
        oc._step_into(vec, st, static_a)
    torch.cuda.current_stream(dev).wait_stream(s)
    oc._step_into(ref, rst, a)
    assert torch.equal(view, rview)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        oc._step_into(vec, st, static_a)
    oc._step_into(ref, rst, a)  # (the captured launches run during capture on this runtime or not: settle it with a full render)
    vec.pos.copy_(ref.pos)
    vec.steps.copy_(ref.steps)
    vec.terminated.copy_(ref.terminated)
    vec.truncated.copy_(ref.truncated)
    vec.engine.render(vec.puzzle_id, vec.pos, st)
    assert torch.equal(view, rview)
    flat = oc._bytes(torch, st)
    for r in range(6):
        a = oc._rand(torch, gen, vec, B)
        static_a.copy_(a)
        if r == 2:
            keep = flat.clone()
            flat.fill_(POISON)
        graph.replay()
        oc._step_into(ref, rst, a)
        if r == 2:  # the replay is the changed form: most of the buffer is left alone
            left = flat == POISON
            assert int(left.sum()) > flat.numel() // 2
            flat[left] = keep[left]
        assert torch.equal(view, rview) and torch.equal(vec.pos, ref.pos), r
    envs = [0, 1, B - 1]
    assert np.array_equal(view[envs].cpu().numpy(), oc._oracle(pool, vec, ids, envs, "uint8"))


# ---- profiling -----------------------------------------------------------------------------------------------------------
def test_one_profiled_launch_per_step(torch_mod, pools):
    torch = torch_mod
    pool, B = pools["level1"], 50
    ids = oc._ids(pool, B, "level1")
    (vec, st, view), (ref, rst, rview) = _twins(pool, ids, "uint8")
    g = torch.Generator(device=vec.device).manual_seed(2)
    oc._step_into(vec, st, oc._rand(torch, g, vec, B))
    vec.engine.profile_render(5)
    for _ in range(5):
        oc._step_into(vec, st, oc._rand(torch, g, vec, B))
    ms = vec.engine.profile_read()
    assert len(ms) == 5 and all(m >= 0.0 for m in ms)


# ---- the library's own buffer --------------------------------------------------------------------------------------------
def test_vec_env_turns_it_on_for_its_own_buffer(torch_mod, pools):
    torch = torch_mod
    from pushworld_amd.vec_env import VecPushWorld

    pool, B = pools["level1"], 50
    ids = oc._ids(pool, B, "level1")
    args = dict(puzzle_ids=ids, max_steps=5, pixels_per_cell=3, border_width=1, observation="uint8", device=0, autoreset=True,
                tune=True, tune_allocations=1)
    want = {"default": True, "changed given": False, "padding given": False, "keyword": False, "torch buffer": False, "padding off": False}
    opts = {"default": {}, "changed given": {"obs_changed_pages": 1}, "padding given": {"obs_padding_once": 1}, "keyword": {},
            "torch buffer": {}, "padding off": {"obs_padding_once": 0}}
    vecs = {}
    for k in want:
        eo = dict({"bind_min_envs": 1}, **opts[k])
        kw = dict(args, tune=k != "torch buffer")
        if k == "keyword":
            kw["changed_rows"] = False
        vecs[k] = VecPushWorld(pool["puzzles"], B, engine_options=eo, **kw)
        assert vecs[k].engine.obs_changed_rows == want[k], k
        vecs[k].reset()
    assert vecs["keyword"].engine.get_option("obs_changed_pages") == 1
    g = torch.Generator(device=vecs["default"].device).manual_seed(21)
    for t in range(12):
        a = oc._rand(torch, g, vecs["default"], B)
        for v in vecs.values():
            v.step(a)
        for k, v in vecs.items():
            assert torch.equal(v.obs, vecs["padding off"].obs), (k, t)
    envs = [0, 1, B - 1]
    assert np.array_equal(vecs["default"].obs[envs].cpu().numpy(), oc._oracle(pool, vecs["default"], ids, envs, "uint8"))

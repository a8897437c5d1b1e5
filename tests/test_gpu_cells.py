"""Cell-grid observations on the GPU: ``pw_render_cells`` / ``pw_step_cells`` against the numpy
definition ``PushWorldPuzzle.cells``, ``pw_step_cells`` state outputs against ``pw_step`` on twin buffers, strides, guard
bytes, streams, graph capture and the vector facades in cells mode."""
import glob
import os
import zipfile

import numpy as np
import pytest
import torch

from pushworld_amd import _capi
from pushworld_amd.puzzle import PushWorldPuzzle
from pushworld_amd.vec_env import VecPushWorld
from pushworld_amd.vector_env import PushWorldDmVectorEnv, PushWorldVectorEnv

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PUZZLES = os.path.join(ROOT, "pushworld_amd", "data", "puzzles")
REF_PY = os.path.join(ROOT, "tests", "puzzles", "ref_python")


def _level(lvl, order="python"):
    return [PushWorldPuzzle(p, order=order) for p in sorted(glob.glob(os.path.join(PUZZLES, lvl, "*.pwp")))]


def _level0_sample(n=48, order="python"):
    with zipfile.ZipFile(os.path.join(PUZZLES, "level0.zip")) as z:
        names = sorted(x for x in z.namelist() if x.endswith(".pwp"))
        step = max(1, len(names) // n)
        return [PushWorldPuzzle(text=z.read(x).decode(), order=order) for x in names[::step][:n]]


def _spec(puzzles, ids, pos, frame):
    """[B, 3, Hc, Wc] from the numpy definition (identical (puzzle, state) pairs computed once)."""
    out = np.zeros((len(ids), 3) + tuple(frame), np.uint8)
    memo = {}
    for e, (i, p) in enumerate(zip(ids, pos)):
        pz = puzzles[int(i)]
        state = tuple((int(x), int(y)) for x, y in p[: pz.num_movables])
        key = (int(i), state)
        if key not in memo:
            memo[key] = pz.cells(state, frame=frame)
        out[e] = memo[key]
    return out


def _random_walk(vec, steps, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    for _ in range(steps):
        vec.step(torch.randint(0, 4, (vec.num_envs,), generator=g, dtype=torch.uint8).to(vec.device))


def _check_vec(vec, frame=None):
    torch.cuda.synchronize()
    frame = frame or tuple(vec.obs.shape[2:])
    want = _spec(vec.puzzles, vec.puzzle_id.cpu().numpy(), vec.states(), frame)
    got = vec.obs.cpu().numpy()
    bad = np.argwhere((got != want).reshape(len(want), -1).any(1))
    assert bad.size == 0, f"{bad.size} environments differ, first {bad[0][0]}"


@pytest.fixture(scope="module")
def levels():
    return {o: _level("level1", o) + _level("level2", o) + _level("level3", o) + _level("level4", o) + _level0_sample(order=o)
            for o in ("python", "cpp")}


@pytest.mark.parametrize("order", ["python", "cpp"])
def test_random_walks_every_level_puzzle(levels, order):
    pool = levels[order]
    P = len(pool)
    vec = VecPushWorld(pool, 2 * P, observation="cells", tune=False, device=0)
    assert vec.engine.np == 32 and vec.engine.get_option("cells_base_bytes") >= P * vec.obs[0].numel()
    vec.reset()
    _check_vec(vec)
    for t in range(3):
        _random_walk(vec, 7, seed=11 * t + (order == "cpp"))
        _check_vec(vec)


def _np_buckets():
    """Pools whose largest movable count gives NP = 4, 8, 16 and 32 (Clean Sweep)."""
    pool = [PushWorldPuzzle(os.path.join(REF_PY, f)) for f in ("multiple_goals.pwp", "file_parsing.pwp")]
    pool += _level("level1") + _level("level2") + _level("level3") + _level("level4")
    out = {}
    for npad, lo in ((4, 0), (8, 5), (16, 9), (32, 17)):
        out[npad] = [p for p in pool if lo < p.num_movables <= npad][:12]
    assert any("Clean Sweep" in (p.file_path or "") for p in out[32]) or out[32]
    return out


@pytest.mark.parametrize("npad", [4, 8, 16, 32])
def test_np_frames_and_strides(npad):
    pool = _np_buckets()[npad]
    assert pool, npad
    W = max(p.dimensions[0] for p in pool)
    H = max(p.dimensions[1] for p in pool)
    for pad in (None, (H + 3, W + 5)):  # default frame, and a larger one with odd margins
        vec = VecPushWorld(pool, 63, observation="cells", pad_cells=pad, tune=False, device=0)
        assert vec.engine.np == npad
        assert vec.obs.shape == (63, 3) + ((H, W) if pad is None else pad)
        vec.reset()
        _random_walk(vec, 5, seed=npad)
        _check_vec(vec)
        want = vec.obs.clone()
        S = vec.obs[0].numel()
        for stride in (S + 1, S + 37, ((S + 15) & ~15) + 16):  # padded strides, 16-byte multiple or not
            buf = torch.full((63 * stride + 64,), 0xAB, dtype=torch.uint8, device=vec.device)
            for off in (0, 3):  # an unaligned first environment too
                buf.fill_(0xAB)
                vec.engine.render_cells(vec.puzzle_id, vec.pos, buf[off:], env_stride=stride)
                torch.cuda.synchronize()
                host = buf.cpu().numpy()
                body = np.stack([host[off + e * stride : off + e * stride + S] for e in range(63)])
                assert (body == want.cpu().numpy().reshape(63, -1)).all(), (stride, off)
                mask = np.ones(host.size, bool)
                for e in range(63):
                    mask[off + e * stride : off + e * stride + S] = False
                assert (host[mask] == 0xAB).all(), (stride, off)  # guard bytes untouched


def test_batch_of_one_and_golden_trajectories(golden):
    keys = [k for k in golden.keys if k.startswith(("bench:level1", "pytest:"))][:14]
    assert keys
    for key in keys:
        pz = PushWorldPuzzle(text=golden.text(key))
        vec = VecPushWorld([pz], 1, observation="cells", tune=False, device=0)
        for name, actions, start, pos, _reward, _term, _goals in golden.sequences(key):
            vec.reset()
            if start is not None:
                vec.set_states(np.pad(np.asarray(start, np.int8)[None], ((0, 0), (0, vec.engine.np - pz.num_movables), (0, 0))))
                vec.render()
            for t, a in enumerate(actions[:60]):
                vec.step(torch.full((1,), int(a), dtype=torch.uint8, device=vec.device))
                st = vec.states()[0, : pz.num_movables]
                assert (st == pos[t]).all(), (key, name, t)
                assert (vec.obs[0].cpu().numpy() == pz.cells(st)).all(), (key, name, t)


@pytest.fixture(scope="module")
def big():
    """The C3 shape: 65 536 environments over the Level-1 pool, default frame."""
    vec = VecPushWorld(_level("level1"), 65536, observation="cells", tune=False, device=0)
    vec.reset()
    return vec


def test_batch_65536(big):
    idx = np.arange(0, big.num_envs, 61)
    for t in range(2):
        torch.cuda.synchronize()
        want = _spec(big.puzzles, big.puzzle_id.cpu().numpy()[idx], big.states()[idx], tuple(big.obs.shape[2:]))
        assert (big.obs.cpu().numpy()[idx] == want).all(), t
        _random_walk(big, 4, seed=5 + t)


@pytest.mark.parametrize("bound", [False, True])
def test_step_cells_matches_step(bound):
    pool = _level("level1")[:24] + _level("level3")[:8]
    pset = _capi.PuzzleSet([p._parsed for p in pool], 0)
    eng = _capi.Engine(pset, max_steps=6, pixels_per_cell=3, border_width=1, obs_dtype=_capi.OBS_U8)
    shape = eng.cells_shape()
    B = 3000
    dev = eng.device
    ids = torch.as_tensor(np.repeat(np.arange(len(pool)), B // len(pool) + 1)[:B], dtype=torch.int32, device=dev)
    pid_a, pid_b = ids.clone(), ids.clone()
    a, b = eng.alloc_state(B), eng.alloc_state(B)
    cells = torch.zeros((B,) + shape, dtype=torch.uint8, device=dev)
    ep_a = torch.zeros(B, dtype=torch.int32, device=dev)
    ep_b = torch.zeros(B, dtype=torch.int32, device=dev)
    for s, pid in ((a, pid_a), (b, pid_b)):
        eng.reset(pid, s["pos"], s["steps"], s["terminated"], s["truncated"], None)
    if bound:  # one binding per engine: the pw_step_cells side takes the bound segments, pw_step the unbound kernels
        assert eng.bind(pid_b)["bound_envs"] > 0
    g = torch.Generator(device="cpu").manual_seed(3)
    for t in range(14):
        act = torch.randint(0, 4, (B,), generator=g, dtype=torch.uint8)
        if t == 4:
            act[17] = 9  # a bad action: flagged 0xFF, env untouched, reset by the next autoreset step
        act = act.to(dev)
        if not bound:
            eng.resample(pid_a, ep_a, 7, a["terminated"], a["truncated"])
            eng.resample(pid_b, ep_b, 7, b["terminated"], b["truncated"])
        eng.step(pid_a, act, a["pos"], a["steps"], a["reward"], a["dgoals"], a["terminated"], a["truncated"],
                 _capi.STEP_AUTORESET)
        eng.step_cells(pid_b, act, b["pos"], b["steps"], b["reward"], b["dgoals"], b["terminated"], b["truncated"], cells,
                       _capi.STEP_AUTORESET)
        torch.cuda.synchronize()
        for k in a:
            assert torch.equal(a[k], b[k]), (t, k)
        assert torch.equal(pid_a, pid_b)
        if t == 4:
            assert int(b["terminated"][17]) == 0xFF
        want = _spec(pool, pid_b.cpu().numpy(), b["pos"].cpu().numpy(), shape[1:])
        assert (cells.cpu().numpy() == want).all(), t
    assert eng.bad_actions() == 2


def test_non_default_stream_and_graph_capture():
    pool = _level("level1")[:16]
    kw = dict(observation="cells", tune=False, device=0, autoreset=True, max_steps=9)
    eager = VecPushWorld(pool, 512, **kw)
    graphed = VecPushWorld(pool, 512, **kw)
    eager.reset()
    graphed.reset()
    s = torch.cuda.Stream()
    act = torch.zeros(512, dtype=torch.uint8, device=graphed.device)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # stream order: the render sees the positions written just before it on this stream
        saved = graphed.pos.clone()
        graphed.pos.zero_()
        graphed.pos.copy_(saved)
        graphed.render()
        graphed.step(act)  # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    eager.step(act)
    torch.cuda.synchronize()
    assert torch.equal(eager.obs, graphed.obs)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        graphed.step(act)
    g = torch.Generator(device="cpu").manual_seed(9)
    for _ in range(12):
        act.copy_(torch.randint(0, 4, (512,), generator=g, dtype=torch.uint8))
        graph.replay()
        eager.step(act)
        torch.cuda.synchronize()
        for x, y in ((eager.obs, graphed.obs), (eager.pos, graphed.pos), (eager.reward, graphed.reward),
                     (eager.terminated, graphed.terminated), (eager.truncated, graphed.truncated)):
            assert torch.equal(x, y)
    _check_vec(graphed)


def test_vector_facades_cells():
    path = os.path.join(PUZZLES, "level1")
    env = PushWorldVectorEnv(path, 96, observation="cells", seed=4, max_steps=12)
    rgb = PushWorldVectorEnv(path, 96, observation="uint8", seed=4, max_steps=12)
    hc, wc = env.vec.obs.shape[2:]
    high = max(3, max(p.num_movables for p in env.puzzles))
    assert env.single_observation_space.shape == (3, hc, wc)
    assert env.single_observation_space.dtype == np.uint8
    assert np.asarray(env.single_observation_space.high).max() == high
    assert env.observation_space.shape == (96, 3, hc, wc)
    obs, _ = env.reset()
    rgb.reset()
    _check_vec(env.vec)
    assert obs.shape == (96, 3, hc, wc)
    g = np.random.default_rng(1)
    for _ in range(20):
        acts = g.integers(0, 4, 96)
        obs, *_ = env.step(acts)
        rgb.step(acts)
    _check_vec(env.vec)
    assert torch.equal(env.puzzle_ids, rgb.puzzle_ids)
    frames = env.render()  # RGB on demand
    assert frames.dtype == torch.uint8 and torch.equal(frames, rgb.render())
    dm = PushWorldDmVectorEnv(path, 32, observation="cells", seed=2, to_numpy=True)
    spec = dm.observation_spec()
    assert tuple(spec.shape) == (3,) + tuple(dm.vec.obs.shape[2:]) and spec.dtype == np.uint8
    assert np.asarray(spec.maximum).max() == max(3, max(p.num_movables for p in dm.puzzles))
    ts = dm.reset()
    want = _spec(dm.puzzles, dm.vec.puzzle_id.cpu().numpy(), dm.vec.states(), tuple(dm.vec.obs.shape[2:]))
    assert (ts.observation == want).all()
    ts = dm.step(np.zeros(32, np.int64))
    want = _spec(dm.puzzles, dm.vec.puzzle_id.cpu().numpy(), dm.vec.states(), tuple(dm.vec.obs.shape[2:]))
    assert (ts.observation == want).all()

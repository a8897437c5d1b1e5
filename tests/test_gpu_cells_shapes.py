"""Cell-grid observations on the device (pw_render_cells / pw_step_cells) where the shipped puzzles do not take
them: the random-shape puzzles and the state lists of tests/shape_states.py -- overlapping movables (the largest index wins),
movables one cell beyond the grid and coordinates far outside it (every cell outside the frame is dropped), frames that give
the kernel 4, 3, 2 and 1 wavefronts per workgroup up to the limit of 65 504 cells, planes that are a multiple of 16 bytes and
planes smaller than one 16-byte chunk, the 64 x 64 board.  Every comparison is against tests/cells_restatement.py, built from
the oracle's sets alone, byte for byte, and the guard bytes around and between environments must stay untouched.

Out-of-range positions are safe to render: in ``pw_cells_kernel`` the bounds test ``cx >= 0 && cx < wc && cy >= 0 && cy < hc``
precedes the only write that depends on a position (the LDS byte ``occ[cy * wc + cx]``), and the shape rows it reads are
indexed by the bounding-box cell alone."""
import numpy as np
import pytest
import torch

import cells_restatement as CR
import replay_cases as RC
import shape_states as SS
from pushworld_amd import _capi
from pushworld_amd.puzzle import PushWorldPuzzle
from pushworld_amd.vec_env import VecPushWorld

pytestmark = pytest.mark.gpu

GUARD = 0xAB
_VECS, _WANT = {}, {}


def _vec(keys, frame=None, **kw):
    """One cells engine per (puzzles, frame), kept for the session."""
    k = (tuple(keys), frame, tuple(sorted(kw.items())))
    if k not in _VECS:
        _VECS[k] = VecPushWorld([PushWorldPuzzle(text=RC.text(key)) for key in keys], 1, observation="cells", pad_cells=frame,
                                max_steps=None, device=0, **kw)
    return _VECS[k]


def _want(key, state, frame):
    """The restatement's observation, computed once per (puzzle, state, frame) and never changed."""
    k = (key, tuple(map(tuple, state)), tuple(frame))
    if k not in _WANT:
        _WANT[k] = CR.cells(RC.puzzle(key), k[1], frame)
        _WANT[k].setflags(write=False)
    return _WANT[k]


def _render(vec, keys, ids, states, stride_extra=0, offset=0):
    """Renders (ids, states) into a guarded byte buffer and compares every environment and every guard byte."""
    eng = vec.engine
    _, hc, wc = eng.cells_shape()
    S, B = 3 * hc * wc, len(ids)
    stride = S + stride_extra
    pos = np.zeros((B, eng.np, 2), np.int8)
    for i, s in enumerate(states):
        pos[i, :len(s)] = np.asarray(s, np.int8)
    t_ids = torch.as_tensor(np.asarray(ids, np.int32), device=vec.device)
    t_pos = torch.as_tensor(pos, device=vec.device)
    buf = torch.full((offset + B * stride + 64,), GUARD, dtype=torch.uint8, device=vec.device)
    eng.render_cells(t_ids, t_pos, buf[offset:], env_stride=stride)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    mask = np.ones(host.size, bool)
    for i in range(B):
        lo = offset + i * stride
        got = host[lo:lo + S].reshape(3, hc, wc)
        want = _want(keys[ids[i]], states[i], (hc, wc))
        assert (got == want).all(), (keys[ids[i]], i, states[i], np.argwhere(got != want)[:4].tolist())
        mask[lo:lo + S] = False
    assert (host[mask] == GUARD).all(), (stride_extra, offset)
    return host


PADDINGS = {4: [SS.CASES[0]], 8: [SS.CASES[1], SS.CASES[2]], 16: [SS.CASES[3]], 32: [SS.CASES[4], SS.CASES[5]]}


@pytest.mark.parametrize("odd_frame", [False, True])
@pytest.mark.parametrize("npad", [4, 8, 16, 32])
def test_overlapping_states(npad, odd_frame):
    keys = PADDINGS[npad]
    H = max(RC.puzzle(k).height for k in keys)
    W = max(RC.puzzle(k).width for k in keys)
    vec = _vec(keys, (H + 3, W + 5) if odd_frame else None)
    assert vec.engine.np == npad and vec.engine.cells_shape() == ((3, H + 3, W + 5) if odd_frame else (3, H, W))
    ids, states = [], []
    for pid, key in enumerate(keys):
        for _, s in RC.states(key):
            ids.append(pid)
            states.append(s)
    assert sum(bool(CR.hidden(RC.puzzle(keys[i]), s)) for i, s in zip(ids, states)) >= 6
    for extra in (0, 1):
        for off in (0, 3):
            _render(vec, keys, ids, states, extra, off)


def _edge_states(key):
    """Listed states with one movable (each in turn) moved to x = -1, y = -1, x + w = W + 1, y + h = H + 1, and states with a
    movable at -128 or 127: [(state, movable, cells of it outside the grid)]."""
    cp = RC.puzzle(key)
    listed = [s for _, s in RC.states(key)]
    out = []
    for n, s in enumerate(listed[:16]):
        k = n % cp.num_movables
        w, h = cp.py.sizes[k]
        x, y = s[k]
        for at in ((-1, y), (x, -1), (cp.width + 1 - w, y), (x, cp.height + 1 - h)):
            t = s[:k] + (at,) + s[k + 1:]
            outside = [c for c in CR.covered(cp, k, at) if not (0 <= c[0] < cp.width and 0 <= c[1] < cp.height)]
            assert outside  # (tight bounding boxes: a box one cell beyond the grid has a cell there)
            out.append((t, k, outside))
    return out


@pytest.mark.parametrize("key", [SS.CASES[0], SS.CASES[2]])
def test_domain_edge(key):
    cp = RC.puzzle(key)
    H, W = cp.height, cp.width
    edge = _edge_states(key)
    states = [s for s, _, _ in edge]
    for frame in (None, (H + 2, W + 2), (H, W + 1)):
        vec = _vec([key], frame)
        hc, wc = vec.engine.cells_shape()[1:]
        oy, ox = (hc - H) // 2, (wc - W) // 2
        assert (oy, ox) == {None: (0, 0), (H + 2, W + 2): (1, 1), (H, W + 1): (0, 0)}[frame]
        for s, k, outside in edge:  # what the restatement says about the cell beyond the grid, before the kernel is asked
            want = _want(key, s, (hc, wc))
            shown = [(x, y) for x, y in outside if 0 <= x + ox < wc and 0 <= y + oy < hc]
            if frame is None:
                assert not shown and (want[1][want[0] == 0] == 0).all()  # dropped: nothing of it at the end of another row
            elif frame == (H + 2, W + 2):
                assert len(shown) == len(outside)
                assert all(want[0, y + oy, x + ox] == 0 and want[1, y + oy, x + ox] >= 1 + k for x, y in shown)  # in the padding
            else:
                assert all(x == W for x, _ in shown)  # the right margin only
        for extra, off in ((0, 0), (1, 3)):
            _render(vec, [key], [0] * len(states), states, extra, off)
    # far outside: everything of the movable is dropped
    vec = _vec([key], (H + 2, W + 2))
    far = []
    for n, (_, s) in enumerate(RC.states(key)[:8]):
        k = n % cp.num_movables
        at = [(-128, s[k][1]), (127, s[k][1]), (s[k][0], -128), (s[k][0], 127), (-128, -128), (127, 127)][n % 6]
        far.append(s[:k] + (at,) + s[k + 1:])
        assert not (_want(key, far[-1], (H + 2, W + 2))[1] == 1 + k).any()
    _render(vec, [key], [0] * len(far), far, 0, 3)


# frame -> (wavefronts per workgroup, plane mod 16): fill_cells_args' epw = min(4, 65536 / (16 * occ_chunks))
WORKGROUPS = {(128, 128): (4, 0), (130, 130): (3, 4), (150, 150): (2, 4), (178, 368): (1, 0), (181, 361): (1, 13)}


def _epw(hc, wc):
    plane = hc * wc
    chunks = ((2 * plane + 15) >> 4) - (plane >> 4)
    return min(4, 65536 // (16 * chunks))


@pytest.mark.parametrize("frame", list(WORKGROUPS))
def test_workgroup_shapes(frame):
    epw, rest = WORKGROUPS[frame]
    assert _epw(*frame) == epw and (frame[0] * frame[1]) % 16 == rest and frame[0] * frame[1] <= 65504
    if frame == (178, 368):
        assert frame[0] * frame[1] == 65504  # the documented limit
    keys = [SS.CASES[0], SS.CASES[2]]
    vec = _vec(keys, frame)
    pool = [(pid, s) for pid, key in enumerate(keys) for _, s in RC.states(key) if SS.overlapping(RC.puzzle(key), s)]
    pool = [pool[i] for i in (1, 30, 7, 41, 12, 35, 20)]  # both puzzles, interleaved
    for batch in (1, 7):  # one environment: a workgroup with idle wavefronts; seven: a last partial workgroup for epw 4, 3, 2
        _render(vec, keys, [p for p, _ in pool[:batch]], [s for _, s in pool[:batch]])


def test_frame_beyond_the_limit_is_refused():
    pz = PushWorldPuzzle(text=RC.text(SS.CASES[0]))
    pset = _capi.PuzzleSet([pz._parsed], 0)
    eng = _capi.Engine(pset, None, 3, 1, _capi.OBS_U8, 165, 397)
    assert 165 * 397 == 65505
    with pytest.raises(ValueError, match="65504"):
        eng.cells_shape()
    ids = torch.zeros(1, dtype=torch.int32, device=eng.device)
    pos = torch.zeros((1, eng.np, 2), dtype=torch.int8, device=eng.device)
    buf = torch.full((3 * 65505 + 64,), GUARD, dtype=torch.uint8, device=eng.device)
    rc = _capi.lib.pw_render_cells(eng.handle, _capi._ptr(ids), _capi._ptr(pos), _capi._ptr(buf), 3 * 65505, 1, None)
    assert rc == _capi.PW_ELIMIT and "65504" in _capi.last_error()
    torch.cuda.synchronize()
    assert bool((buf == GUARD).all())  # refused before any launch


SMALLEST = "A"  # one file cell: 3 x 3 with the border walls, 9 cells per plane -- less than one 16-byte chunk


def test_smallest_frame():
    from oracle import c_oracle

    cp = c_oracle.COraclePuzzle(SMALLEST)
    assert (cp.width, cp.height, cp.num_movables, cp.num_goals) == (3, 3, 1, 0)
    vec = VecPushWorld([PushWorldPuzzle(text=SMALLEST)], 1, observation="cells", max_steps=None, device=0)
    assert vec.engine.cells_shape() == (3, 3, 3)
    starts = [(x, y) for y in (-1, 0, 1, 2, 3) for x in (-1, 0, 1, 2, 3)]  # the agent on and around the grid
    for batch in (1, 65):
        states = [(starts[i % len(starts)],) for i in range(batch)]
        want = [CR.cells(cp, s) for s in states]
        for off in (0, 3):
            pos = np.zeros((batch, vec.engine.np, 2), np.int8)
            pos[:, 0] = [s[0] for s in states]
            buf = torch.full((off + 27 * batch + 64,), GUARD, dtype=torch.uint8, device=vec.device)
            vec.engine.render_cells(torch.zeros(batch, dtype=torch.int32, device=vec.device), torch.as_tensor(pos, device=vec.device),
                                    buf[off:], env_stride=27)
            torch.cuda.synchronize()
            host = buf.cpu().numpy()
            assert (host[off:off + 27 * batch].reshape(batch, 3, 3, 3) == np.stack(want)).all(), (batch, off)
            assert (host[:off] == GUARD).all() and (host[off + 27 * batch:] == GUARD).all()


def test_board_64x64():
    key = SS.CASES[5]
    vec = _vec([key])
    assert vec.engine.cells_shape() == (3, 64, 64) and vec.engine.np == 32
    states = [s for _, s in RC.states(key)]
    for off in (0, 5):  # 768 chunks: exactly 12 rounds of the streaming loop; 13 when the first environment is misaligned
        _render(vec, [key], [0] * len(states), states, 0, off)


def test_step_cells_from_far_states():
    keys = RC.SETS[16]
    puzzles = [PushWorldPuzzle(text=RC.text(k)) for k in keys]
    pset = _capi.PuzzleSet([p._parsed for p in puzzles], 0)
    eng = _capi.Engine(pset, None, 3, 1, _capi.OBS_U8)
    assert eng.np == 16
    shape = eng.cells_shape()
    ids, states = [], []
    for pid, key in enumerate(keys):
        for kind, s in RC.states(key):
            if kind == "far":
                ids.append(pid)
                states.append(s)
    B, dev = len(ids), eng.device
    assert B >= 30
    pos0 = np.zeros((B, 16, 2), np.int8)
    for i, s in enumerate(states):
        pos0[i, :len(s)] = np.asarray(s, np.int8)
    pid = torch.as_tensor(np.asarray(ids, np.int32), device=dev)
    for action in range(4):
        a, b = eng.alloc_state(B), eng.alloc_state(B)
        for s in (a, b):
            eng.reset(pid, s["pos"], s["steps"], s["terminated"], s["truncated"], None)
            s["pos"].copy_(torch.as_tensor(pos0, device=dev))
        act = torch.full((B,), action, dtype=torch.uint8, device=dev)
        cells = torch.full((B,) + shape, GUARD, dtype=torch.uint8, device=dev)
        eng.step(pid, act, a["pos"], a["steps"], a["reward"], a["dgoals"], a["terminated"], a["truncated"], 0)
        eng.step_cells(pid, act, b["pos"], b["steps"], b["reward"], b["dgoals"], b["terminated"], b["truncated"], cells, 0)
        torch.cuda.synchronize()
        for k in a:
            assert torch.equal(a[k], b[k]), (action, k)
        new, got = b["pos"].cpu().numpy(), cells.cpu().numpy()
        reward, term = b["reward"].cpu().numpy(), b["terminated"].cpu().numpy()
        moved = 0
        for i in range(B):
            cp = RC.puzzle(keys[ids[i]])
            want_state, want_reward, want_term = cp.env_step(states[i], action)
            assert reward[i:i + 1].view(np.uint64)[0] == np.array([want_reward]).view(np.uint64)[0] and term[i] == want_term
            state = tuple((int(x), int(y)) for x, y in new[i, :cp.num_movables])
            assert state == want_state, (action, i)
            moved += state != states[i]
            assert (got[i] == _want(keys[ids[i]], state, shape[1:])).all(), (action, i)
        assert moved > 0

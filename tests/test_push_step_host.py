"""Host side of stepping by pushes: the restatement (tests/push_step_restatement.py) against values worked out by
hand on ``deep_puzzles.corridor(8)``, the argument checks of ``pw_step_push`` / ``pw_push_mask`` that return before any launch,
the header against ``_capi.SIGNATURES`` and the ``PW_PUSH_*`` values, the input checks of the Python wrappers and the decoding of
``choice``."""
import ctypes
import os
import re

import pytest
import torch

import deep_puzzles
import push_step_restatement as SR
from oracle import c_oracle
from pushworld_amd import _capi
from pushworld_amd.search import PUSH_NONE, decode_push_choice, push_mask
from pushworld_amd.vec_env import VecPushWorld
from test_walk_host import HAND

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# stand-ins for device pointers (and for the engine): every check below returns before anything is read through them
P = ctypes.c_void_p(4096)
C = -0.01


def _corridor():
    """corridor(8) is `A . . . . M0 . G0`; with its border the board is 10 x 3 and the agent starts at (1, 1)."""
    cp = c_oracle.COraclePuzzle(deep_puzzles.corridor(8))
    assert (cp.width, cp.height, cp.num_movables, cp.num_goals) == (10, 3, 2, 1)
    assert cp.initial_state == ((1, 1), (6, 1)) and tuple(cp.py.goal_state[0]) == (8, 1)
    return cp


def _env(cp, state=None, steps=0, terminated=0, truncated=0):
    return SR.Env(cp.initial_state if state is None else state, steps, terminated, truncated)


def test_restatement_by_hand_without_max_steps():
    cp = _corridor()
    first = SR.macro_step(cp, _env(cp), (5, 1), 1)  # the cell left of M0, RIGHT: dist 4
    assert first == SR.Result(((6, 1), (7, 1)), 5, ((((C + C) + C) + C) + C), 0, 0, 0, 5, SR.DONE)
    second = SR.macro_step(cp, SR.Env(first.state, first.steps, 0, 0), (6, 1), 1)  # dist 0
    assert second == SR.Result(((7, 1), (8, 1)), 6, 10.0, 1, 1, 0, 1, SR.DONE)
    counts = SR.Counts()
    counts.add(first)
    counts.add(second)
    assert (counts.env_steps, counts.ended, counts.solved) == (6, 1, 1)


def test_restatement_by_hand_with_max_steps():
    cp = _corridor()
    cut = SR.macro_step(cp, _env(cp), (5, 1), 1, max_steps=3)
    assert cut == SR.Result(((4, 1), (6, 1)), 3, ((C + C) + C), 0, 0, 1, 3, SR.CUT)  # three cells right, M0 unmoved
    done = SR.macro_step(cp, _env(cp), (5, 1), 1, max_steps=5)
    assert done == SR.Result(((6, 1), (7, 1)), 5, ((((C + C) + C) + C) + C), 0, 0, 1, 5, SR.DONE)  # M0 one cell right
    # an environment past max_steps already (no autoreset): the first step returns truncated
    late = SR.macro_step(cp, _env(cp, steps=9), (5, 1), 1, max_steps=3)
    assert late == SR.Result(((2, 1), (6, 1)), 10, C, 0, 0, 1, 1, SR.CUT)


def test_restatement_goal_state_and_autoreset():
    cp = _corridor()
    solved = ((3, 1), (8, 1))
    # the box on its goal can only be pushed into the border: nothing moves, no push move
    assert SR.macro_step(cp, _env(cp, ((7, 1), (8, 1))), (7, 1), 1).status == SR.REFUSED
    reset = SR.macro_step(cp, _env(cp, solved, steps=7, terminated=1), (5, 1), 1, autoreset=True)
    assert reset == SR.Result(cp.initial_state, 0, 0.0, 0, 0, 0, 0, SR.RESET)
    reset = SR.macro_step(cp, _env(cp, solved, steps=7, truncated=1), (-9, 99), 0xFF, autoreset=True)  # the choice is not read
    assert reset.status == SR.RESET and reset.state == cp.initial_state
    # without autoreset the flags on entry are not looked at, as the primitive step
    again = SR.macro_step(cp, _env(cp, terminated=1), (5, 1), 1)
    assert again.status == SR.DONE and again.moves == 5
    # a goal state already (the hand puzzle of the walk tests after M0 went onto its goal): the first walking step terminates
    hp = c_oracle.COraclePuzzle(HAND)
    m0, m2 = hp.py.names.index("m0"), hp.py.names.index("m2")
    goal = tuple((2, 2) if k == 0 else ((4, 2) if k == m0 else xy) for k, xy in enumerate(hp.initial_state))
    assert hp.py.is_goal_state(goal)
    walk = SR.macro_step(hp, _env(hp, goal), (2, 1), 1)  # UP, then RIGHT would push M2
    assert walk == SR.Result(((2, 1),) + goal[1:], 1, 10.0, 0, 1, 0, 1, SR.CUT)
    # at dist 0 the push is the first step: M2 moves, M0 stays on its goal
    off = SR.macro_step(hp, _env(hp, ((2, 1),) + goal[1:]), (2, 1), 1)
    assert off.status == SR.DONE and off.moves == 1 and off.state[m2] == (5, 1) and off.terminated == 1 and off.reward == 10.0


REFUSALS = [
    ("outside the grid", dict(frm=(10, 1))),
    ("negative position", dict(frm=(-1, 1))),
    ("outside the region", dict(frm=(7, 1))),     # behind the box
    ("a walk move", dict(frm=(3, 1))),
    ("a move that displaces nothing", dict(frm=(1, 1), action=0)),  # LEFT into the border
    ("action 4", dict(action=4)),
    ("PUSH_NONE", dict(action=0xFF)),
    ("puzzle id outside the set", dict(no_puzzle=True)),
    ("a movable outside its grid", dict(state=((1, 1), (10, 1)))),
]


@pytest.mark.parametrize("kind, kw", REFUSALS, ids=[k for k, _ in REFUSALS])
def test_restatement_refusals(kind, kw):
    cp = _corridor()
    env = _env(cp, kw.get("state"), steps=4, terminated=7, truncated=9)  # sentinels: left as they were
    res = SR.macro_step(None if kw.get("no_puzzle") else cp, env, kw.get("frm", (5, 1)), kw.get("action", 1), max_steps=50)
    assert res == SR.Result(tuple(env.state), 4, 0.0, 0, 7, 9, 0, SR.REFUSED)
    counts = SR.Counts()
    counts.add(res)
    assert (counts.env_steps, counts.ended, counts.solved) == (0, 0, 0)


def _step_push(e=P, ids=P, frm=P, act=P, pos=P, steps=P, term=P, trunc=P, batch=4):
    return _capi.lib.pw_step_push(e, ids, frm, act, pos, steps, None, None, term, trunc, None, None, batch, 0, None)


@pytest.mark.parametrize("kw, words", [
    (dict(e=None), "null engine"),
    (dict(ids=None), "null puzzle_id"),
    (dict(frm=None), "null push_from"),
    (dict(act=None), "null push_action"),
    (dict(pos=None), "null pos"),
    (dict(steps=None), "null steps"),
    (dict(term=None), "null terminated"),
    (dict(trunc=None), "null truncated"),
])
def test_step_push_argument_checks(kw, words):
    assert _step_push(**kw) == _capi.PW_EINVAL
    msg = _capi.last_error()
    assert words in msg and "pw_step_push" in msg


def _mask(e=P, ids=P, npad=8, n=4, out=P, map_h=8, map_w=8):
    return _capi.lib.pw_push_mask(e, ids, None, npad, None, n, out, None, map_h, map_w, None)


@pytest.mark.parametrize("kw, words", [
    (dict(e=None), "null engine"),
    (dict(ids=None), "null puzzle_id"),
    (dict(out=None), "null push_mask"),
    (dict(n=0), "n must be"),
    (dict(n=-3), "n must be"),
    (dict(npad=0), "npad"),
    (dict(npad=12), "npad"),
    (dict(map_h=0), "map_h"),
    (dict(map_h=65), "map_h"),
    (dict(map_w=0), "map_w"),
    (dict(map_w=65), "map_w"),
])
def test_push_mask_argument_checks(kw, words):
    assert _mask(**kw) == _capi.PW_EINVAL
    msg = _capi.last_error()
    assert words in msg and "pw_push_mask" in msg


def test_batch_must_be_positive():
    """batch < 1 is looked at after the pointers and before the engine is."""
    for batch in (0, -5):
        assert _step_push(batch=batch) == _capi.PW_EINVAL
        msg = _capi.last_error()
        assert "batch must be" in msg and "pw_step_push" in msg


def test_header_signatures_and_status_values():
    with open(os.path.join(ROOT, "include", "pushworld_amd.h")) as f:
        src = f.read()
    assert _capi.lib.pw_abi_version() == 4 and re.search(r"#define PW_ABI_VERSION 4\b", src)
    for name, value in (("REFUSED", 0), ("DONE", 1), ("CUT", 2), ("RESET", 3)):
        assert re.search(r"#define PW_PUSH_%s %d\b" % (name, value), src), name
        assert getattr(_capi, "PUSH_" + name) == value == getattr(SR, name)
    for name in ("pw_step_push", "pw_push_mask"):
        decl = re.search(r"\bint %s\((.*?)\);" % name, src, re.S)
        assert decl, name
        params = [p for p in re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",") if p.strip()]
        restype, argtypes = _capi.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == len(params), name
        for p, t in zip(params, argtypes):
            want = ctypes.c_void_p if "*" in p else (ctypes.c_uint32 if "uint32_t" in p else ctypes.c_int32)
            assert t is want, (name, p)
        assert hasattr(_capi.lib, name)


def test_choice_decoding():
    map_h, map_w = 5, 7
    # (a, y, x) = (2, 3, 4) is flat index (2 * 5 + 3) * 7 + 4 = 95
    choice = torch.tensor([95, 0, 4 * 35 - 1, 34, 35, -1, 4 * 35], dtype=torch.int64)
    frm, act = decode_push_choice(choice, map_h, map_w)
    assert frm.dtype == torch.int8 and act.dtype == torch.uint8 and frm.is_contiguous() and act.is_contiguous()
    assert frm.tolist()[:5] == [[4, 3], [0, 0], [6, 4], [6, 4], [0, 0]]
    assert act.tolist() == [2, 0, 3, 0, 1, PUSH_NONE, PUSH_NONE]  # an index outside the shape: no push move
    # the index of an expanded mask's entry decodes to that entry
    m = torch.zeros((4, map_h, map_w), dtype=torch.bool)
    m[2, 3, 4] = True
    assert int(m.flatten().nonzero()[0, 0]) == 95


def test_wrapper_input_checks():
    with pytest.raises(ValueError, match="engine_or_vec"):
        push_mask(object(), None)
    with pytest.raises(ValueError, match="engine_or_vec"):
        push_mask(None, None)
    vec = VecPushWorld.__new__(VecPushWorld)  # the checks come before anything of the engine is used
    vec._has_reset = False
    with pytest.raises(RuntimeError, match="reset"):
        vec.step_push(torch.zeros((3, 2), dtype=torch.int8), torch.zeros(3, dtype=torch.uint8))
    vec._has_reset = True
    vec.device, vec.num_envs, vec._act_shape = torch.device("cpu"), 3, (3,)
    frm, act = torch.zeros((3, 2), dtype=torch.int8), torch.zeros(3, dtype=torch.uint8)
    bad = [
        (dict(), "either"),
        (dict(push_from=frm), "either"),
        (dict(push_action=act), "either"),
        (dict(push_from=frm, push_action=act, choice=torch.zeros(3, dtype=torch.int64)), "either"),
        (dict(choice=torch.zeros(3, dtype=torch.int32)), "choice"),
        (dict(choice=torch.zeros(4, dtype=torch.int64)), "choice"),
        (dict(choice=[0, 0, 0]), "choice"),
        (dict(push_from=frm.to(torch.uint8), push_action=act), "push_from"),
        (dict(push_from=torch.zeros((3, 3), dtype=torch.int8), push_action=act), "push_from"),
        (dict(push_from=torch.zeros((2, 3), dtype=torch.int8).t(), push_action=act), "push_from"),
        (dict(push_from=frm, push_action=act.to(torch.int8)), "push_action"),
        (dict(push_from=frm, push_action=torch.zeros(4, dtype=torch.uint8)), "push_action"),
        (dict(push_from=frm, push_action=torch.zeros(6, dtype=torch.uint8)[::2]), "push_action"),
    ]
    for kw, words in bad:
        with pytest.raises(ValueError, match=words):
            vec.step_push(**kw)
    vec.device = torch.device("cuda", 0)
    with pytest.raises(ValueError, match="push_from"):
        vec.step_push(frm, act)
    with pytest.raises(ValueError, match="choice"):
        vec.step_push(choice=torch.zeros(3, dtype=torch.int64))

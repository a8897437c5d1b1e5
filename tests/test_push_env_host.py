"""Host side of push-mode stepping with the mask kept: the header's declaration of ``pw_step_push_mask`` against
``_capi.SIGNATURES``, the include order and ``build.HEADERS``, the argument checks that return before any launch, the input checks
of ``VecPushWorld.step_push_mask`` / ``observe_pushes``, the restatement (tests/push_env_restatement.py) against values worked out
by hand on ``SEALED`` and the HAND puzzle, and the action spaces of the push-mode facades."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import push_env_restatement as ER
import push_step_restatement as SR
from oracle import c_oracle
from pushworld_amd import _capi, build
from pushworld_amd.vec_env import PushStep, VecPushWorld
from pushworld_amd.vector_env import PushWorldPushDmVectorEnv, PushWorldPushVectorEnv, push_action_spaces
from test_walk_host import HAND

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEALED = "A W M0 . G0\n"  # the agent sealed in one cell: a region of one position, no push

# stand-ins for device pointers (and for the engine): every check below returns before anything is read through them
P = ctypes.c_void_p(4096)
C = -0.01


def test_header_signature_and_flag():
    with open(os.path.join(ROOT, "include", "pushworld_amd.h")) as f:
        src = f.read()
    assert _capi.lib.pw_abi_version() == 4 and re.search(r"#define PW_ABI_VERSION 4\b", src)
    assert re.search(r"#define PW_PUSH_END_STUCK 0x100u\b", src) and _capi.PUSH_END_STUCK == 0x100
    assert _capi.PUSH_END_STUCK & _capi.STEP_AUTORESET == 0
    decl = re.search(r"\bint pw_step_push_mask\((.*?)\);", src, re.S)
    assert decl
    params = [p for p in re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",") if p.strip()]
    restype, argtypes = _capi.SIGNATURES["pw_step_push_mask"]
    assert restype is ctypes.c_int and len(argtypes) == len(params) == 23
    for p, t in zip(params, argtypes):
        want = ctypes.c_void_p if "*" in p else (ctypes.c_uint32 if "uint32_t" in p else ctypes.c_int32)
        assert t is want, p
    names = [p.split()[-1].lstrip("*") for p in params]
    assert names[12:18] == ["push_mask", "num_pushes", "walk_map", "region_size", "view_pos", "view_id"]
    assert names[18:] == ["map_h", "map_w", "batch", "flags", "stream"]
    assert hasattr(_capi.lib, "pw_step_push_mask")


def test_include_order_and_build_headers():
    with open(os.path.join(ROOT, "pushworld_amd", "csrc", "pw_kernels.hip")) as f:
        unit = f.read()
    assert unit.index('#include "pw_push_step.inc"') < unit.index('#include "pw_push_env.inc"')
    assert unit.count('#include "pw_push_env.inc"') == 1
    assert "pw_push_env.inc" in build.HEADERS
    assert os.path.exists(os.path.join(ROOT, "pushworld_amd", "csrc", "pw_push_env.inc"))


ARGS = ["e", "ids", "frm", "act", "pos", "steps", "reward", "dgoals", "term", "trunc", "moves", "status", "mask", "count", "wmap",
        "size", "vpos", "vid"]


def _call(map_h=8, map_w=8, batch=4, flags=0, **kw):
    ptrs = [kw.get(k, None if k in ("reward", "dgoals", "moves", "status") else P) for k in ARGS]
    return _capi.lib.pw_step_push_mask(*ptrs, map_h, map_w, batch, flags, None)


@pytest.mark.parametrize("kw, words", [
    (dict(e=None), "null engine"),
    (dict(ids=None), "null puzzle_id"),
    (dict(frm=None), "null push_from"),
    (dict(act=None), "null push_action"),
    (dict(pos=None), "null pos"),
    (dict(steps=None), "null steps"),
    (dict(term=None), "null terminated"),
    (dict(trunc=None), "null truncated"),
    (dict(mask=None), "null push_mask"),
    (dict(count=None), "null num_pushes"),
    (dict(wmap=None), "null walk_map"),
    (dict(size=None), "null region_size"),
    (dict(vpos=None), "null view_pos"),
    (dict(vid=None), "null view_id"),
    (dict(batch=0), "batch must be"),
    (dict(batch=-5), "batch must be"),
    (dict(map_h=0), "map_h"),
    (dict(map_h=65), "map_h"),
    (dict(map_w=0), "map_w"),
    (dict(map_w=65), "map_w"),
])
def test_argument_checks(kw, words):
    assert _call(**kw) == _capi.PW_EINVAL
    msg = _capi.last_error()
    assert words in msg and "pw_step_push_mask" in msg


def test_wrapper_input_checks():
    vec = VecPushWorld.__new__(VecPushWorld)  # the checks come before anything of the engine is used
    vec._has_reset = False
    with pytest.raises(RuntimeError, match="reset"):
        vec.step_push_mask(torch.zeros((3, 2), dtype=torch.int8), torch.zeros(3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="reset"):
        vec.observe_pushes()
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
            vec.step_push_mask(end_stuck=True, **kw)
    vec.device = torch.device("cuda", 0)
    with pytest.raises(ValueError, match="push_from"):
        vec.step_push_mask(frm, act)
    assert PushStep._fields == ("obs", "reward", "terminated", "truncated", "moves", "status", "mask", "num_pushes")


def test_restatement_by_hand_on_sealed():
    """With its border SEALED is 7 x 3: the agent at (1, 1) between the border and a wall, M0 at (3, 1)."""
    cp = c_oracle.COraclePuzzle(SEALED)
    assert (cp.width, cp.height, cp.num_movables) == (7, 3, 2) and cp.initial_state == ((1, 1), (3, 1))
    view = ER.view_of(cp, 0, cp.initial_state)
    assert view == ER.View({}, 0, {(1, 1): 0}, 1, ((1, 1), (3, 1)), 0)
    mask, wmap = ER.dense(view, 3, 7)
    assert not mask.any() and wmap[1, 1] == 0 and (wmap.reshape(-1) == ER.OUTSIDE).sum() == 20
    env = SR.Env(cp.initial_state, 0, 0, 0)
    # every choice is refused; with the stuck rule the environment is truncated at once, without it nothing happens
    for frm, a in (((1, 1), 1), ((1, 1), 0xFF), ((3, 1), 1)):
        assert ER.lookup(view, frm, a) is None
        off = ER.step(cp, 0, env, frm, a, max_steps=50)
        assert off == ER.Step(SR.Result(cp.initial_state, 0, 0.0, 0, 0, 0, 0, SR.REFUSED), view, False)
        on = ER.step(cp, 0, env, frm, a, max_steps=50, end_stuck=True)
        assert on == ER.Step(SR.Result(cp.initial_state, 0, 0.0, 0, 0, 1, 0, SR.REFUSED), view, True)
    counts = ER.Counts()
    counts.add_step(on)
    counts.add_step(off)
    assert (counts.env_steps, counts.ended, counts.solved) == (0, 1, 0)
    # the next call resets it (the stuck rule fires again on the initial state: truncated once more)
    again = ER.step(cp, 0, SR.Env(on.result.state, 0, 0, 1), (1, 1), 1, autoreset=True, end_stuck=True)
    assert again.result.status == SR.RESET and again.result.truncated == 1 and again.stuck
    # a flag that is set already keeps the rule off
    assert not ER.step(cp, 0, SR.Env(cp.initial_state, 3, 1, 0), (1, 1), 1, end_stuck=True).stuck


def test_restatement_by_hand_on_the_hand_puzzle():
    """test_walk_host.test_restatement_by_hand's region: R = {(1, 2): 0, (1, 1): 1 by UP, (2, 1): 2 by RIGHT}; ((2, 1), RIGHT)
    pushes M2 and ((1, 2), RIGHT) pushes M0 onto its goal."""
    cp = c_oracle.COraclePuzzle(HAND)
    s = cp.initial_state
    m0, m2 = cp.py.names.index("m0"), cp.py.names.index("m2")
    view = ER.view_of(cp, 5, s)
    assert view.mask == {(2, 1): 2, (1, 2): 2} and view.num_pushes == 2 and view.region_size == 3
    assert view.walk_map == {(1, 2): 0, (1, 1): 1 | 2 << 12, (2, 1): 2 | 1 << 12}
    assert view.pos == s and view.pid == 5
    assert ER.lookup(view, (2, 1), 1) == 2 and ER.lookup(view, (1, 2), 1) == 0
    assert ER.lookup(view, (2, 1), 3) is None and ER.lookup(view, (1, 1), 1) is None and ER.lookup(view, (2, 2), 1) is None
    assert ER.lookup(view, (2, 1), 4) is None and ER.lookup(view, (2, 1), 0xFF) is None
    # the currency rule
    assert ER.is_current(view, 5, s, 6, 4) and not ER.is_current(view, 4, s, 6, 4) and not ER.is_current(view, 5, s, 5, 4)
    assert ER.is_current(view, 5, s + ((9, 9),), 6, 4)  # nothing beyond N is compared
    assert not ER.is_current(view, 5, ((1, 1),) + s[1:], 6, 4) and not ER.is_current(ER.SKIPPED, -1, s, 6, 4)
    # M2 pushed: three primitive steps, and the view of the state that is left
    st = ER.step(cp, 5, SR.Env(s, 0, 0, 0), (2, 1), 1, end_stuck=True)
    after = tuple((3, 1) if k == 0 else ((5, 1) if k == m2 else xy) for k, xy in enumerate(s))
    assert st.result == SR.Result(after, 3, (C + C) + C, 0, 0, 0, 3, SR.DONE) and not st.stuck
    assert st.view == ER.view_of(cp, 5, after) and st.view.pos == after and st.view.walk_map[(3, 1)] == 0
    # cut at max_steps 2: the agent stands at (2, 1), nothing was pushed
    cut = ER.step(cp, 5, SR.Env(s, 0, 0, 0), (2, 1), 1, max_steps=2)
    assert cut.result == SR.Result(((2, 1),) + s[1:], 2, C + C, 0, 0, 1, 2, SR.CUT)
    assert cut.view.walk_map == {(2, 1): 0, (1, 1): 1 | 0 << 12, (1, 2): 2 | 3 << 12} and cut.view.mask == view.mask
    # M0 onto its goal: terminated, the view of the goal state is written all the same
    goal = ER.step(cp, 5, SR.Env(s, 0, 0, 0), (1, 2), 1, end_stuck=True)
    assert goal.result.terminated == 1 and goal.result.reward == 10.0 and not goal.stuck
    assert goal.view == ER.view_of(cp, 5, goal.result.state) and goal.result.state[m0] == (4, 2)
    # a skipped item
    assert ER.view_of(None, 9, s) == ER.SKIPPED and ER.view_of(cp, 0, ((6, 2),) + s[1:]) == ER.SKIPPED
    mask, wmap = ER.dense(ER.SKIPPED, 5, 7)
    assert not mask.any() and (wmap == ER.OUTSIDE).all()
    skipped = ER.step(None, 9, SR.Env(s, 4, 0, 0), (2, 1), 1, end_stuck=True)
    assert skipped.result.status == SR.REFUSED and skipped.stuck and skipped.view == ER.SKIPPED


def test_action_spaces_of_the_facades():
    single, batched = push_action_spaces(5, 7, 3)
    assert single.n == 4 * 5 * 7 == 140 and batched.shape == (3,)
    assert single.contains(0) and single.contains(139) and not single.contains(140) and not single.contains(-1)
    assert batched.contains(np.asarray([0, 139, 95])) and not batched.contains(np.asarray([0, 140, 95]))
    assert not batched.contains(np.asarray([0, 1])) and not batched.contains(np.asarray([0.0, 1.0, 2.0]))
    assert not batched.contains(np.asarray([0, -1, 2]))
    assert batched.sample().shape == (3,) and batched.contains(batched.sample())
    for cls in (PushWorldPushVectorEnv, PushWorldPushDmVectorEnv):
        assert {"reset", "step", "check_actions", "close"} <= set(dir(cls))
    assert {"step_async", "step_wait", "render"} <= set(dir(PushWorldPushVectorEnv))
    assert PushWorldPushVectorEnv.metadata["autoreset_mode"] == "next_step"

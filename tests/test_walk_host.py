"""Host side of the walk regions and push moves: the argument checks of ``pw_walk_regions`` /
``pw_walk_pushes`` that return before any launch, the input checks of the Python wrappers, and the restatement
(tests/walk_restatement.py) against values worked out by hand and against the pinned counts of the search over pushes."""
import ctypes
import os

import pytest
import torch

import deep_puzzles
import walk_restatement as WR
from oracle import c_oracle
from pushworld_amd import _capi
from pushworld_amd.search import PushMoves, PushSearch, WalkRegions, _walk_inputs, walk_regions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVEL1 = os.path.join(ROOT, "pushworld_amd", "data", "puzzles", "level1")

# stand-ins for device pointers (and for the engine): every check below returns before anything is read through them
P = ctypes.c_void_p(4096)

# A 2-cell agent, one agent wall, a box that can be pushed onto its goal (M0), a box that can be pushed (M2) and one whose push
# is stopped transitively (M0 pushed down onto M1, which stands against the border).  With the border the board is 7 x 5.
HAND = """
 .  .  . M2  .
 A  A M0 G0  .
AW  . M1  .  .
""".lstrip("\n")


def _regions(e=P, ids=P, pos=None, npad=8, mask=None, n=4, region_size=P, canon=None, offset=P, walk_map=None, map_h=0,
             map_w=0):
    return _capi.lib.pw_walk_regions(e, ids, pos, npad, mask, n, region_size, canon, offset, walk_map, map_h, map_w, None)


def _pushes(e=P, ids=P, pos=None, npad=8, mask=None, n=4, offset=P, cap=16):
    return _capi.lib.pw_walk_pushes(e, ids, pos, npad, mask, n, offset, cap, None, None, None, None, None, None, None, None,
                                    None)


CASES = [
    (dict(e=None), "null engine"),
    (dict(ids=None), "null puzzle_id"),
    (dict(offset=None), "null offset"),
    (dict(n=0), "n must be"),
    (dict(n=-3), "n must be"),
    (dict(npad=0), "npad"),
    (dict(npad=12), "npad"),
    (dict(npad=64), "npad"),
]


@pytest.mark.parametrize("kw, words", CASES + [
    (dict(region_size=None), "null region_size"),
    (dict(walk_map=P, map_h=0, map_w=8), "map_h"),
    (dict(walk_map=P, map_h=65, map_w=8), "map_h"),
    (dict(walk_map=P, map_h=8, map_w=0), "map_w"),
    (dict(walk_map=P, map_h=8, map_w=65), "map_w"),
])
def test_regions_argument_checks(kw, words):
    assert _regions(**kw) == _capi.PW_EINVAL
    msg = _capi.last_error()
    assert words in msg and "pw_walk_regions" in msg


@pytest.mark.parametrize("kw, words", CASES + [(dict(cap=-1), "cap must be")])
def test_pushes_argument_checks(kw, words):
    assert _pushes(**kw) == _capi.PW_EINVAL
    msg = _capi.last_error()
    assert words in msg and "pw_walk_pushes" in msg


def test_abi_version_unchanged():
    assert _capi.lib.pw_abi_version() == 4


def test_wrapper_arguments():
    with pytest.raises(ValueError, match="engine_or_vec"):
        walk_regions(object(), None)
    with pytest.raises(ValueError, match="engine_or_vec"):
        walk_regions(None, None)
    assert PushMoves().item is None and PushMoves().dropped is None
    regions = WalkRegions(None, None, None, None)
    assert regions.walk_map is None and regions.offset is None
    with pytest.raises(ValueError, match="not requested"):
        regions.path(0, (1, 1))
    regions.walk_map = torch.full((1, 3, 4), 0xFFFF, dtype=torch.int32)
    regions.walk_map[0, 1, 1] = 0
    regions.walk_map[0, 1, 2] = 1 | 1 << 12   # reached from (1, 1) by RIGHT
    regions.walk_map[0, 2, 2] = 2 | 3 << 12   # reached from (2, 1) by DOWN
    assert regions.path(0, (1, 1)) == [] and regions.path(0, (2, 2)) == [1, 3]
    for xy in ((0, 0), (3, 2), (4, 1), (1, 3), (-1, 1)):
        with pytest.raises(ValueError, match="not in the walk region"):
            regions.path(0, xy)
    with pytest.raises(ValueError, match="item index"):
        regions.path(1, (1, 1))
    assert callable(PushSearch)


def test_walk_input_checks():
    cpu = torch.device("cpu")
    ids = torch.zeros(5, dtype=torch.int32)
    pos = torch.zeros((5, 8, 2), dtype=torch.int8)
    assert _walk_inputs(ids, None, None, 8, cpu) == 5
    assert _walk_inputs(ids, pos, torch.ones(5, dtype=torch.uint8), 8, cpu) == 5
    assert _walk_inputs(ids, pos, torch.ones(5, dtype=torch.bool), 8, cpu) == 5
    bad = [
        (ids.long(), pos, None, "puzzle_id"),
        (ids.view(5, 1), pos, None, "puzzle_id"),
        (torch.zeros(0, dtype=torch.int32), None, None, "items"),
        (ids, pos.to(torch.uint8), None, "pos"),
        (ids, pos[:, :4], None, "pos"),
        (ids, pos.view(5, 16), None, "pos"),
        (ids, pos, torch.ones(5, dtype=torch.int32), "mask"),
        (ids, pos, torch.ones(4, dtype=torch.uint8), "mask"),
        (torch.zeros(10, dtype=torch.int32)[::2], pos, None, "contiguous"),
        (ids, pos.transpose(1, 2).contiguous().transpose(1, 2), None, "contiguous"),
    ]
    for a, b, m, words in bad:
        with pytest.raises(ValueError, match=words):
            _walk_inputs(a, b, m, 8, cpu)
    with pytest.raises(ValueError, match="live on"):
        _walk_inputs(ids, None, None, 8, torch.device("cuda", 0))


def test_restatement_by_hand():
    p = c_oracle.COraclePuzzle(HAND)
    assert (p.width, p.height, p.num_movables, p.num_goals) == (7, 5, 4, 1) and p.py.has_agent_walls
    assert p.py.sizes[0] == (2, 1)
    m0, m1, m2 = (p.py.names.index(k) for k in ("m0", "m1", "m2"))
    assert m0 == 1
    s = p.initial_state
    assert s[0] == (1, 2) and s[m0] == (3, 2) and s[m1] == (3, 3) and s[m2] == (4, 1)
    reg = WR.region(p, s)
    # (1, 2): LEFT border, UP walks, DOWN agent wall, RIGHT pushes M0 onto its goal.  (1, 1): RIGHT walks.  (2, 1): RIGHT pushes
    # M2, DOWN would push M0 onto M1 against the border: stopped transitively, nothing moves.
    assert reg.dist == {(1, 2): 0, (1, 1): 1, (2, 1): 2}
    assert reg.parent == {(1, 1): 2, (2, 1): 1}
    assert reg.canon == (1, 1) and WR.canon(p, s)[0] == (1, 1) and WR.canon(p, s)[1:] == s[1:]
    assert WR.path(reg, (2, 1)) == [2, 1] and WR.path(reg, (1, 2)) == []
    assert p.get_next_state_moved(((2, 1),) + s[1:], 3) == (((2, 1),) + s[1:], [])  # the transitive stop
    after_m2 = tuple((3, 1) if k == 0 else ((5, 1) if k == m2 else xy) for k, xy in enumerate(s))
    after_m0 = tuple((2, 2) if k == 0 else ((4, 2) if k == m0 else xy) for k, xy in enumerate(s))
    assert reg.pushes == [
        WR.Push((2, 1), 1, 2, 1 | 1 << m2, False, after_m2),
        WR.Push((1, 2), 1, 0, 1 | 1 << m0, True, after_m0),
    ]
    res = WR.push_search(p)
    assert res.plan == [1] and res.pushes == 1 and res.layer_states == [] and res.num_states == 3
    assert (res.push_rows, res.largest_region) == (2, 3)
    assert WR.push_search(p, start=after_m0).plan == []
    assert WR.in_grid(p, s) and not WR.in_grid(p, ((6, 2),) + s[1:])


def test_pinned_counts():
    """The exhausted push-level space of `big` (against its 42 832 states move by move), and `2 Obstacle` up to its goal."""
    big = WR.push_search(c_oracle.COraclePuzzle(deep_puzzles.big()), stop_at_goal=False)
    assert big.plan is None
    assert (big.num_states, big.push_rows, big.largest_region) == (1260, 6464, 34)
    assert big.layer_states == [8, 36, 100, 220, 296, 278, 168, 96, 40, 12, 4, 1, 0] and 1 + sum(big.layer_states) == 1260
    p = c_oracle.COraclePuzzle(open(os.path.join(LEVEL1, "2 Obstacle.pwp")).read())
    two = WR.push_search(p)
    assert two.pushes == 11 and len(two.plan) == 45
    assert two.layer_states == [5, 13, 24, 36, 49, 58, 63, 61, 50, 35]
    assert (two.num_states, two.push_rows, two.largest_region) == (416, 6394, 86)
    # the count of a FIFO search that takes a state's pushes in the order a flood of its region meets them
    assert WR.fifo_states_closed(p) == (408, 11)
    for name, fifo, layered in (("Two Goals", (61, 4), 60), ("Single Obstacle", (9, 3), 11)):
        q = c_oracle.COraclePuzzle(open(os.path.join(LEVEL1, name + ".pwp")).read())
        assert WR.fifo_states_closed(q) == fifo and WR.push_search(q).num_states == layered

"""Plain-Python restatement of ``pw_step_push_mask`` over ``push_step_restatement.macro_step`` and
``walk_restatement.region``: the macro step, then the region of the state that is left -- push mask, number of push moves, walk
map and region size.  It carries the currency rule of the view and the stuck rule.  A helper, not a test.

Definitions:
  view       ``View(mask, num_pushes, walk_map, region_size, pos, pid)`` of one state: ``mask`` {(x, y): bits} (bit a set when
             ((x, y), a) is a push move), ``walk_map`` {(x, y): dist | parent << 12} over the walk region, ``pos`` the first N
             positions, ``pid`` the puzzle id.  A skipped item (a puzzle id outside the set: ``cp`` None; a movable outside its
             grid) has the empty mask and map, 0 push moves, region size -1, id -1 and no positions.
  current    the view's id is the environment's, an index into the set, and its positions are the environment's first N.
  step       ``push_step_restatement.macro_step`` unchanged (reset, refusals, cuts, reward sum); then the view of the state that
             is left; then, with ``end_stuck``, an environment with 0 push moves and neither flag gets ``truncated`` 1 and counts
             as an ended episode -- status, reward and moves stay.
``dense`` turns a view into the arrays the device writes (every entry: 0 in the mask and 0xFFFF in the map outside the region)."""
from collections import namedtuple

import numpy as np

import push_step_restatement as SR
import walk_restatement as WR

OUTSIDE = 0xFFFF
View = namedtuple("View", "mask num_pushes walk_map region_size pos pid")
SKIPPED = View({}, 0, {}, -1, (), -1)
Step = namedtuple("Step", "result view stuck")


def view_of(cp, pid, state, region_of=None):
    """The view of ``state`` of puzzle ``cp`` with id ``pid`` (``region_of``: the caller's ``walk_restatement.region`` of a
    state of ``cp``, e.g. one that keeps what it computed)."""
    state = tuple(tuple(xy) for xy in state)
    if cp is None or not WR.in_grid(cp, state):
        return SKIPPED
    reg = WR.region(cp, state) if region_of is None else region_of(state)
    mask = {}
    for pm in reg.pushes:
        mask[pm.frm] = mask.get(pm.frm, 0) | (1 << pm.action)
    walk_map = {q: d | (reg.parent.get(q, 0) << 12) for q, d in reg.dist.items()}
    return View(mask, len(reg.pushes), walk_map, len(reg.dist), state[:cp.num_movables], pid)


def is_current(view, pid, state, num_puzzles, num_movables):
    """The currency rule: nothing beyond the puzzle's N movables is compared."""
    if view.pid != pid or not 0 <= pid < num_puzzles:
        return False
    return tuple(map(tuple, view.pos[:num_movables])) == tuple(map(tuple, state[:num_movables]))


def lookup(view, frm, action):
    """What a current view says of the choice: dist(frm) when it is valid, else None."""
    frm = (int(frm[0]), int(frm[1]))
    if action not in (0, 1, 2, 3) or frm not in view.walk_map or not (view.mask.get(frm, 0) >> action) & 1:
        return None
    return view.walk_map[frm] & 0xFFF


def step(cp, pid, env, frm, action, max_steps=None, autoreset=False, end_stuck=False, initial=None, reg=None, region_of=None):
    """``Step(result, view, stuck)`` of one environment: ``result`` the macro step's ``Result`` with the stuck rule applied,
    ``view`` the view of the state that is left, ``stuck`` whether the stuck rule fired."""
    res = SR.macro_step(cp, env, frm, action, max_steps=max_steps, autoreset=autoreset, initial=initial, reg=reg)
    view = view_of(cp, pid, res.state, region_of)
    stuck = bool(end_stuck and view.num_pushes == 0 and not res.terminated and not res.truncated)
    if stuck:
        res = res._replace(truncated=1)
    return Step(res, view, stuck)


def dense(view, map_h, map_w):
    """``(mask uint8 [map_h, map_w], walk_map uint16 [map_h, map_w])`` of a view."""
    mask = np.zeros((map_h, map_w), np.uint8)
    wmap = np.full((map_h, map_w), OUTSIDE, np.uint16)
    for (x, y), bits in view.mask.items():
        mask[y, x] = bits
    for (x, y), entry in view.walk_map.items():
        wmap[y, x] = entry
    return mask, wmap


class Counts(SR.Counts):
    """``push_step_restatement.Counts`` with the stuck rule: an environment it truncates ended an episode."""

    def add_step(self, st):
        if st.stuck:
            self.ended += 1
            self.add(st.result._replace(truncated=0))  # (the macro step's own flags: neither was set)
        else:
            self.add(st.result)

"""Plain-Python restatement of the best-first search over pushes (``pw_push_planner_*``) over
``walk_restatement.region`` / ``canon`` / ``in_grid`` and ``rgd_restatement.RecursiveGraphDistance``.  A helper of
tests/test_push_planner_host.py and tests/test_gpu_push_planner.py, not a test.

A node is a canonical state; the store keeps the state as reached, its canon and its links (``push_search_restatement.Link``).
The key of a state is the RGD cost (fewest tools) of the state as reached, as float32: ``GiveUp`` (more than ``rgd_budget``
calls) gives NaN and counts as an overrun, a movable off its movement graph gives NaN without one.  The queue pops the lowest
finite key first, then +inf, then NaN; within one key the newest entry, which is the highest store index.

A round: pop up to K states; T = the sum of their push moves; when states + T > max_states the round ends with ``limit`` and
appends nothing; otherwise the rows of the popped states in pop order, a state's push moves in (y, x, action) order; a
successor is appended when it lies inside its grid, its canonical state is not closed and it is the first such row; the
successor of the first row into a goal state is appended whatever else holds, ends the store and the search; otherwise every
new state is keyed and pushed in store order."""
import math
from collections import namedtuple

import numpy as np

import rgd_restatement as R
import walk_restatement as WR
from push_search_restatement import ROOT_ACTION, Link

KEY_RANGE = 1 << 22
DEFAULT_BUDGET = 1 << 12  # PW_RGD_DEFAULT_BUDGET

Info = namedtuple("Info", "status rounds expanded states open goal_index rgd_exceeded push_rows largest_region largest_key")


def _order(key):
    if key != key:
        return (2, 0)
    if math.isinf(key):
        return (1, 0)
    return (0, int(key))


class PushPlannerRestatement:
    """``p``: an ``oracle.c_oracle.COraclePuzzle``; ``oz``: the ``oracle.pw_oracle.OraclePuzzle`` of the same text (with its
    collision tables, for the movement graphs)."""

    def __init__(self, p, oz, batch=1, max_states=1 << 20, rgd_budget=None, graphs=None):
        self.p, self.K, self.max_states = p, batch, max_states
        self.rgd = R.RecursiveGraphDistance(oz, fewest_tools=True, max_calls=DEFAULT_BUDGET if rgd_budget is None else rgd_budget,
                                            graphs=graphs)

    def key(self, state):
        try:
            return float(np.float32(self.rgd.estimate(state)))
        except R.GiveUp:
            self.rgd_exceeded += 1
            return math.nan
        except KeyError:
            return math.nan

    def begin(self, start=None):
        p = self.p
        start = tuple(tuple(xy) for xy in (p.initial_state if start is None else start))
        if not WR.in_grid(p, start):
            raise ValueError("start has a movable outside the grid")
        goal = bool(p.py.is_goal_state(start))
        self.states, self.canons, self.links = [start], [WR.region(p, start).canon], [Link(-1, (0, 0), ROOT_ACTION, 0, goal)]
        self.closed, self.buckets = set(), {}
        self.rounds = self.expanded = self.open = self.push_rows = self.largest_region = self.rgd_exceeded = 0
        self.largest_key, self.goal_index = -1, -1
        if goal:
            self.status, self.goal_index = "solved", 0
            return
        self.status = "running"
        self.closed.add(WR.canon(p, start))
        self._push([0])

    def _push(self, fresh):
        for idx in fresh:
            self.largest_region = max(self.largest_region, len(WR.region(self.p, self.states[idx]).dist))
        for idx in fresh:
            key = self.key(self.states[idx])
            if key == key and not math.isinf(key):
                if key >= KEY_RANGE:
                    raise ValueError("an RGD cost does not fit the bucket range")
                self.largest_key = max(self.largest_key, int(key))
            self.buckets.setdefault(_order(key), []).append(idx)
            self.open += 1

    def run(self, max_rounds=None):
        p, done = self.p, 0
        while self.status == "running" and (max_rounds is None or done < max_rounds):
            done += 1
            if self.open == 0:
                self.status = "exhausted"
                break
            pops = []
            while len(pops) < self.K and self.open:
                b = min(self.buckets)
                pops.append(self.buckets[b].pop())
                if not self.buckets[b]:
                    del self.buckets[b]
                self.open -= 1
            self.rounds += 1
            self.expanded += len(pops)
            regs = [WR.region(p, self.states[k]) for k in pops]
            T = sum(len(r.pushes) for r in regs)
            self.push_rows += T
            if len(self.states) + T > self.max_states:
                self.status = "limit"
                break
            first = len(self.states)
            for k, reg in zip(pops, regs):
                for pm in reg.pushes:
                    inside = WR.in_grid(p, pm.next_state)
                    c = WR.canon(p, pm.next_state) if inside else None
                    if (inside and c not in self.closed) or pm.goal:
                        self.closed.add(c)
                        self.states.append(pm.next_state)
                        self.canons.append(c[0] if inside else (0, 0))
                        self.links.append(Link(k, pm.frm, pm.action, pm.walk, bool(pm.goal)))
                    if pm.goal:
                        self.status, self.goal_index = "solved", len(self.states) - 1
                        break
                if self.status == "solved":
                    break
            if self.status == "solved":
                break
            self._push(range(first, len(self.states)))
        return self.info()

    def info(self):
        return Info(self.status, self.rounds, self.expanded, len(self.states), self.open, self.goal_index, self.rgd_exceeded,
                    self.push_rows, self.largest_region, self.largest_key)

    def plan(self):
        """(primitive actions, pushes) when solved, else None."""
        if self.status != "solved":
            return None
        plan, pushes, index = [], 0, self.goal_index
        while self.links[index].parent >= 0:
            ln = self.links[index]
            plan = WR.path(WR.region(self.p, self.states[ln.parent]), ln.frm) + [ln.action] + plan
            index, pushes = ln.parent, pushes + 1
        return plan, pushes

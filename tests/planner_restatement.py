"""Plain-Python restatement of the GPU planner's semantics (``pw_planner_create`` in include/pushworld_amd.h): the reference's
best_first_search (cpp/include/search/best_first_search.h:45-98) with a bucket queue, popping K states per round.

Successors come from ``oracle.pw_oracle.OraclePuzzle.get_next_state_moved``, novelty from ``OracleNovelty`` and RGD from
``rgd_restatement.RecursiveGraphDistance`` (``GiveUp`` -> NaN).  ``heuristic`` may also be any callable
``(state, moved) -> float`` (the reference's C++ search tests use Manhattan distances)."""
import math
import os
import sys

import numpy as np

from oracle import pw_oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rgd_restatement as R  # noqa: E402


def _order(key):
    """Queue order of a key: finite keys ascending, then +inf, then NaN."""
    if key != key:
        return (2, 0.0)
    if math.isinf(key):
        return (1, 0.0)
    return (0, key)


class PlannerRestatement:
    def __init__(self, pz, heuristic="N+RGD", batch=1, max_states=1 << 20, groups=None, rgd_max_calls=None):
        self.pz = pz
        self.K = batch
        self.max_states = max_states
        self.groups = groups  # None: fixed L R U D
        self.mode = heuristic
        if callable(heuristic):
            self.h = heuristic
        else:
            rgd = R.RecursiveGraphDistance(pz, fewest_tools=True, max_calls=rgd_max_calls)
            self.rgd = rgd
            self.rgd_exceeded = 0

            def rgd_cost(state):
                try:
                    return float(np.float32(rgd.estimate(state)))
                except R.GiveUp:
                    self.rgd_exceeded += 1
                    return math.nan

            if heuristic == "RGD":
                self.h = lambda state, moved: rgd_cost(state)
            else:
                nov = pw_oracle.OracleNovelty(pz.num_movables)
                self.h = lambda state, moved: float(np.float32(np.float32(nov.estimate(state, moved) * 1e6)
                                                               + np.float32(rgd_cost(state))))

    def begin(self, start=None):
        start = tuple(map(tuple, start if start is not None else self.pz.initial_state))
        self.store, self.parent, self.action = [start], [-1], [-1]
        self.index = {start: 0}
        self.buckets = {}  # order -> stack of store indices
        self.open = 0
        self.rounds = self.expanded = 0
        self.goal = -1
        self.visited = 1
        if self.pz.is_goal_state(start):
            self.status, self.goal = "solved", 0
            return
        self.status = "running"
        self._push(0, self.h(start, list(range(len(start)))))

    def _push(self, idx, key):
        self.buckets.setdefault(_order(key), []).append(idx)
        self.open += 1

    def run(self, max_rounds=None):
        done = 0
        while self.status == "running" and (max_rounds is None or done < max_rounds):
            done += 1
            if len(self.store) + 4 * self.K > self.max_states:
                self.status = "limit"
                break
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
            cands = []
            for s in pops:
                grp = self.groups[(self.expanded + 1) % 1000] if self.groups is not None else (0, 1, 2, 3)
                self.expanded += 1
                for a in grp:
                    nxt, moved = self.pz.get_next_state_moved(self.store[s], a)
                    cands.append((s, a, nxt, moved))
            self.rounds += 1
            new = []
            for s, a, nxt, moved in cands:
                if nxt in self.index:
                    continue
                idx = len(self.store)
                self.store.append(nxt)
                self.parent.append(s)
                self.action.append(a)
                self.index[nxt] = idx
                if self.pz.is_goal_state(nxt):
                    self.status, self.goal, self.visited = "solved", idx, idx
                    return self.info()
                new.append((idx, moved))
            self.visited = len(self.store)
            if self.mode == "N+RGD":  # novelty of all new states first (tables in order), then RGD
                keys = [self._nrgd(idx, moved) for idx, moved in new]
            else:
                keys = [self.h(self.store[idx], moved) for idx, moved in new]
            for (idx, _), key in zip(new, keys):
                self._push(idx, key)
        return self.info()

    def _nrgd(self, idx, moved):
        return self.h(self.store[idx], moved)

    def info(self):
        return dict(status=self.status, rounds=self.rounds, expanded=self.expanded, visited=self.visited, open=self.open,
                    goal=self.goal)

    def plan(self):
        if self.status != "solved":
            return None
        out, i = [], self.goal
        while i > 0:
            out.append(self.action[i])
            i = self.parent[i]
        return out[::-1]

"""Plain-Python restatement of the reference's recursive graph distance (RGD) heuristic, the test oracle of
``pw_puzzle_movement_graph`` / ``pw_rgd_*``.

Works on an ``oracle.pw_oracle.OraclePuzzle`` (its ``static`` / ``dynamic`` collision tables are the reference's
``ObjectCollisions``, pushworld_puzzle.cc:123-172, 327-359).  Three parts, each following the reference's own procedure:

* ``movement_graphs``: the frontier-and-waiting-transitions growth of ``build_feasible_movement_graphs``
  (cpp/src/heuristics/domain_transition_graph.cc:113-216);
* ``PathDistances``: one lazily grown breadth-first search per target over the reversed graph
  (domain_transition_graph.cc:218-300);
* ``RecursiveGraphDistance``: ``estimate_cost_to_goal`` and the functions below it
  (cpp/src/heuristics/recursive_graph_distance.cc:43-252), with float costs and ``math.inf``.

Positions are ``(x, y)`` tuples.  Successors are visited in action order L, R, U, D and pushers in index order, the order
the HIP kernel uses, so ``calls`` (calls of the recursive pushing cost) counts the same frames as the kernel's budget.
"""
from __future__ import annotations

import math

INF = math.inf
DISPLACEMENTS = ((-1, 0), (1, 0), (0, -1), (0, 1))  # L, R, U, D


def _add(p, d):
    return (p[0] + d[0], p[1] + d[1])


def movement_graphs(pz):
    """``[{position: {end positions}}]`` per movable, every node a key (start positions included)."""
    n, W, H = pz.num_movables, pz.width, pz.height
    graphs = [dict() for _ in range(n)]
    waiting = {}  # pusher transition (i, start, end) -> object transitions it would make feasible
    frontier = []
    for j, p in enumerate(pz.initial_state):
        graphs[j].setdefault(p, set())  # an edgeless start position is a node too (:125-134)
        frontier.append((j, p))

    def inside(j, p):
        w, h = pz.sizes[j]
        return 0 <= p[0] <= W - w and 0 <= p[1] <= H - h

    def add_transition(j, start, end):
        todo = [(j, start, end)]
        while todo:
            j, start, end = todo.pop()
            succ = graphs[j][start]
            if end in succ:
                continue
            succ.add(end)
            todo.extend(waiting.pop((j, start, end), ()))
            if end not in graphs[j]:
                graphs[j][end] = set()
                frontier.append((j, end))

    while frontier:
        j, p = frontier.pop()
        for a in range(4):
            if p in pz.static[a][j]:
                continue
            end = _add(p, DISPLACEMENTS[a])
            if not inside(j, end):  # only from a start overlapping a wall, where the reference would run off the grid
                continue
            if j == 0:
                add_transition(0, p, end)
                continue
            pushed = False
            for i in range(n):
                if i == j or pushed:
                    continue
                for r in pz.dynamic[a][i][j]:
                    s = _add(p, r)
                    t = _add(s, DISPLACEMENTS[a])
                    if t in graphs[i].get(s, ()):
                        add_transition(j, p, end)
                        pushed = True
                        break
                    waiting.setdefault((i, s, t), []).append((j, p, end))
    return graphs


class _SingleSource:
    """Breadth-first search from ``start`` grown one layer at a time until the asked position is found."""

    def __init__(self, graph, start):
        self.graph = graph
        self.depth = 0
        self.frontier = [start]
        self.dist = {start: 0.0}

    def get(self, target):
        if target in self.dist:
            return self.dist[target]
        found = False
        while self.frontier:
            self.depth += 1
            nxt = []
            for p in self.frontier:
                for q in self.graph[p]:
                    if q not in self.dist:
                        nxt.append(q)
                        self.dist[q] = float(self.depth)
                        found = found or q == target
            self.frontier = nxt
            if found:
                return float(self.depth)
        return INF


class PathDistances:
    """``get(src, dst)``: edges on a shortest path from ``src`` to ``dst``; inf when ``dst`` is no node or unreachable."""

    def __init__(self, graph):
        rev = {p: set() for p in graph}
        for p, succ in graph.items():
            for q in succ:
                rev.setdefault(q, set()).add(p)
        self.by_target = {t: _SingleSource(rev, t) for t in rev}

    def get(self, src, dst):
        s = self.by_target.get(dst)
        return INF if s is None else s.get(src)


class GiveUp(Exception):
    """More calls than ``max_calls``."""


class RecursiveGraphDistance:
    def __init__(self, pz, fewest_tools=True, max_calls=None, graphs=None):
        """``graphs``: movement graphs computed before (``movement_graphs(pz)``, or the library's host-built ones where a
        host test has pinned them equal), to spare the slowest step of this class."""
        self.pz = pz
        self.fewest_tools = fewest_tools
        self.max_calls = max_calls
        self.graphs = movement_graphs(pz) if graphs is None else graphs
        self.dist = [PathDistances(g) for g in self.graphs]
        self.calls = 0

    def estimate(self, state):
        """estimate_cost_to_goal (:43-66).  ``KeyError`` when a movable is off its graph (the reference's ``.at()``)."""
        state = tuple(tuple(p) for p in state)
        for j, p in enumerate(state):
            if p not in self.graphs[j]:
                raise KeyError((j, p))
        self.calls = 0
        cost = 0.0
        n = len(state)
        for k, goal in enumerate(self.pz.goal_state):
            obj = k + 1  # goal k belongs to movable k + 1 (:48-56)
            if self.fewest_tools:
                cost += self.fewest_tools_goal_cost(state, obj, goal)
            else:
                cost += self.goal_cost(state, obj, goal, n - 2)
            if cost == INF:
                break
        return cost

    def fewest_tools_goal_cost(self, state, obj, goal):
        """:100-112: the first pushing depth with a finite cost."""
        for depth in range(len(state) - 1):
            c = self.goal_cost(state, obj, goal, depth)
            if c != INF:
                return c
        return INF

    def _successors(self, obj, p):
        succ = self.graphs[obj][p]
        return [q for q in (_add(p, d) for d in DISPLACEMENTS) if q in succ]

    def goal_cost(self, state, obj, goal, depth):
        """:68-98."""
        cur = state[obj]
        if cur == goal:
            return 0.0
        best = INF
        for eff in self._successors(obj, cur):
            gd = self.dist[obj].get(eff, goal)
            if gd >= best:
                continue
            best = gd + self.pushing_cost(state, obj, cur, eff, frozenset(), depth, best - gd)
        return best

    def pushing_cost(self, state, obj, cur, eff, skipped, depth, bound):
        """get_recursive_pushing_cost (:114-188)."""
        self.calls += 1
        if self.max_calls is not None and self.calls > self.max_calls:
            raise GiveUp()
        best = bound
        skipped = skipped | {obj}
        pushers = [0] if depth == 0 else range(1, len(state))  # the agent only at depth 0, never deeper (:129-135)
        for p in pushers:
            if p in skipped:
                continue
            pos = state[p]
            for nxt, c in self.pushing_costs(p, pos, obj, cur, eff):
                if c >= best:
                    continue
                if p == 0:
                    best = min(best, c + 1.0)  # the agent's own pushing move (:154-161)
                else:
                    best = c + self.pushing_cost(state, p, pos, nxt, skipped, depth - 1, best - c)
        return best

    def pushing_costs(self, pusher, pos, pushee, start, end):
        """get_pushing_costs (:190-252): [(next position of the pusher, cost)] in action order."""
        d = (end[0] - start[0], end[1] - start[1])
        a = DISPLACEMENTS.index(d)
        graph = self.graphs[pusher]
        costs = {}
        for r in self.pz.dynamic[a][pusher][pushee]:
            s = _add(start, r)
            t = _add(s, d)
            if t not in graph.get(s, ()):
                continue
            for nxt in graph[pos]:
                if s == pos and t == nxt:
                    c = 0.0  # simultaneous push
                else:
                    c = self.dist[pusher].get(nxt, s)
                    if c == INF:
                        continue
                    c += 1.0
                if nxt not in costs or c < costs[nxt]:
                    costs[nxt] = c
        return [(q, costs[q]) for q in (_add(pos, dd) for dd in DISPLACEMENTS) if q in costs]

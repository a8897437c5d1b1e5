"""Plain-Python restatement of the walk region, the push moves and the search over pushes, over nothing but the
step function of the compiled C oracle (``oracle.c_oracle.COraclePuzzle.get_next_state_moved``).  The only reference of the
walk tests.

Definitions, for a state ``s`` with agent position ``q0`` (positions are bounding-box origins):
  walk move (q, a)  stepping ``s`` with the agent placed at ``q`` by action ``a`` moves the agent and nothing else
  R(s)              the agent positions reachable from ``q0`` by walk moves; ``dist`` is the breadth-first distance.  A position
                    at which the agent leaves its grid is not part of R.
  parent(q)         the lowest action ``a`` with ``q - d_a`` in R one layer nearer and ``(q - d_a, a)`` a walk move
  push move (q, a)  ``q`` in R and the step moves the agent and at least one other movable
  canon(s)          the position of R smallest in (y, x) order
"""
from collections import namedtuple

DISPLACEMENTS = ((-1, 0), (1, 0), (0, -1), (0, 1))  # LEFT, RIGHT, UP, DOWN

Push = namedtuple("Push", "frm action walk moved goal next_state")
Region = namedtuple("Region", "dist parent pushes canon")


def _placed(state, q):
    return (tuple(q),) + tuple(tuple(xy) for xy in state[1:])


def in_grid(p, state):
    """The range test of the entry points: every movable's bounding box inside the grid."""
    return all(0 <= x and 0 <= y and x + w <= p.width and y + h <= p.height
               for (x, y), (w, h) in zip(state, p.py.sizes))


def _steps(p, others):
    """{(q, a): step result} of puzzle ``p`` with the other movables at ``others`` -- a walk or push verdict depends on nothing
    else.  Kept on the puzzle object, so it lives and dies with it."""
    cache = p.__dict__.setdefault("_walk_steps", {})
    return cache.setdefault(others, {})


def region(p, state):
    """``Region`` of ``state``: ``dist`` {q: int}, ``parent`` {q: action} (no entry for q0), ``pushes`` in (y, x, action)
    order of their starting position, and ``canon``."""
    state = tuple(tuple(xy) for xy in state)
    q0 = state[0]
    aw, ah = p.py.sizes[0]
    found = _steps(p, state[1:])
    dist, parent = {q0: 0}, {}
    layer, d = [q0], 0
    while layer:
        nxt = []
        for a in range(4):  # action-major: the first discovery of a position carries its lowest parent action
            dx, dy = DISPLACEMENTS[a]
            for q in layer:
                key = (q, a)
                if key not in found:
                    found[key] = p.get_next_state_moved(_placed(state, q), a)
                succ, moved = found[key]
                if moved != [0]:
                    continue
                r = (q[0] + dx, q[1] + dy)
                if r in dist or not (0 <= r[0] and 0 <= r[1] and r[0] + aw <= p.width and r[1] + ah <= p.height):
                    continue
                dist[r] = d + 1
                parent[r] = a
                nxt.append(r)
        layer, d = nxt, d + 1
    pushes = []
    for q in sorted(dist, key=lambda xy: (xy[1], xy[0])):
        for a in range(4):
            succ, moved = found[(q, a)]
            if len(moved) > 1:
                mask = sum(1 << k for k in moved)
                pushes.append(Push(q, a, dist[q], mask, bool(p.py.is_goal_state(succ)), succ))
    return Region(dist, parent, pushes, min(dist, key=lambda xy: (xy[1], xy[0])))


def canon(p, state):
    """The canonical state: ``state`` with the agent at the smallest position of its walk region."""
    return _placed(state, region(p, state).canon)


def path(reg, xy):
    """The walk actions from q0 to ``xy`` along the parent actions."""
    acts, q = [], tuple(xy)
    while q in reg.parent:
        a = reg.parent[q]
        acts.append(a)
        q = (q[0] - DISPLACEMENTS[a][0], q[1] - DISPLACEMENTS[a][1])
    assert reg.dist[q] == 0
    return acts[::-1]


SearchResult = namedtuple("SearchResult", "plan pushes layer_states num_states push_rows largest_region")


def push_search(p, start=None, max_pushes=None, stop_at_goal=True):
    """Breadth-first search over canonical states, one layer of pushes per round.  It ends with the layer in which a push into a
    goal state appears; the plan goes through the first such row (frontier order, then row order).  ``layer_states``: the new
    canonical states of every completed layer before that one.  ``num_states``: the canonical states closed -- when a goal was
    found, those closed up to and including the goal row's successor (a FIFO search's count at its first goal), else all of them.
    ``plan``: primitive actions, [] for a start that is a goal, None when the space (or ``max_pushes``) is exhausted.
    ``stop_at_goal=False`` searches on through goal states until the space is exhausted."""
    start = tuple(tuple(xy) for xy in (p.initial_state if start is None else start))
    if stop_at_goal and p.py.is_goal_state(start):
        return SearchResult([], 0, [], 1, 0, 0)
    closed = {canon(p, start): None}  # canonical state -> (the state the push started from, Push)
    frontier = [start]
    layers, rows, largest, depth = [], 0, 0, 0
    while frontier and (max_pushes is None or depth < max_pushes):
        depth += 1
        fresh, goal, at_goal = [], None, 0
        for s in frontier:
            reg = region(p, s)
            largest = max(largest, len(reg.dist))
            rows += len(reg.pushes)
            for pm in reg.pushes:
                if in_grid(p, pm.next_state):
                    c = canon(p, pm.next_state)
                    if c not in closed:
                        closed[c] = (s, pm)
                        fresh.append(pm.next_state)
                if stop_at_goal and pm.goal and goal is None:
                    goal, at_goal = (s, pm), len(closed)
        if goal is not None:
            plan = []
            s, pm = goal
            while True:
                plan = path(region(p, s), pm.frm) + [pm.action] + plan
                link = closed[canon(p, s)]
                if link is None:
                    break
                s, pm = link
            return SearchResult(plan, depth, layers, at_goal, rows, largest)
        layers.append(len(fresh))
        frontier = fresh
    return SearchResult(None, None, layers, len(closed), rows, largest)


def fifo_states_closed(p, start=None):
    """(canonical states closed, pushes) of a FIFO search over pushes up to its first goal: a popped state's pushes are taken in
    the order in which a flood of its walk region with a queue of cells meets them (cells in queue order, then the action), the
    search stops at the first push into a goal state, and the count is what was closed before that successor."""
    from collections import deque

    start = tuple(tuple(xy) for xy in (p.initial_state if start is None else start))
    closed = {canon(p, start): 0}
    queue = deque([start])
    while queue:
        s = queue.popleft()
        reg = region(p, s)
        steps = _steps(p, s[1:])
        order, cells = {s[0]: 0}, deque([s[0]])
        while cells:
            q = cells.popleft()
            for a in range(4):
                succ, moved = steps[(q, a)]
                if moved == [0] and succ[0] in reg.dist and succ[0] not in order:
                    order[succ[0]] = len(order)
                    cells.append(succ[0])
        depth = closed[canon(p, s)]
        for pm in sorted(reg.pushes, key=lambda m: (order[m.frm], m.action)):
            if pm.goal:
                return len(closed), depth + 1
            c = canon(p, pm.next_state)
            if c not in closed:
                closed[c] = depth + 1
                queue.append(pm.next_state)
    return len(closed), None

"""Plain-Python restatement of the store of the search over pushes (``pw_push_search_*``) over
``walk_restatement.region`` and ``walk_restatement.canon``: for every layer the states as reached, their canon and their
links, in store order.  A helper of tests/test_push_search_host.py and tests/test_gpu_push_search.py, not a test.

Store order: state 0 is the start; layer d + 1 holds the successors of the push moves of layer d's states, the states in
store order, a state's push moves in (y, x, action) order; a successor is appended when it lies inside its grid, its
canonical state is not closed, and it is the first such row.  With ``stop_at_goal`` the successor of the first row into a
goal state is the last state of the store; the rest of that layer is counted (rows, regions) but not expanded."""
from collections import namedtuple

import walk_restatement as WR

ROOT_ACTION = 0xFF

Link = namedtuple("Link", "parent frm action walk goal")
Store = namedtuple("Store", "states canons links layers layer_states num_states goal_index pushes push_rows largest_region")


def search_store(p, start=None, max_pushes=None, stop_at_goal=True):
    """``Store`` of the search from ``start``: ``states`` / ``canons`` / ``links`` per state in store order, ``layers``
    [(first index, count)] per depth, and the counters of ``walk_restatement.push_search``."""
    start = tuple(tuple(xy) for xy in (p.initial_state if start is None else start))
    is_goal = bool(p.py.is_goal_state(start))
    states, canons, links = [start], [WR.region(p, start).canon], [Link(-1, (0, 0), ROOT_ACTION, 0, is_goal)]
    layers = [(0, 1)]
    if stop_at_goal and is_goal:
        return Store(states, canons, links, layers, [], 1, 0, 0, 0, 0)
    closed = {WR.canon(p, start)}
    frontier, layer_states, rows, largest, depth = [0], [], 0, 0, 0
    while frontier and (max_pushes is None or depth < max_pushes):
        depth += 1
        first, goal_index = len(states), -1
        for k in frontier:
            reg = WR.region(p, states[k])
            largest = max(largest, len(reg.dist))
            rows += len(reg.pushes)
            if goal_index >= 0:
                continue
            for pm in reg.pushes:
                inside = WR.in_grid(p, pm.next_state)
                c = WR.canon(p, pm.next_state) if inside else None
                at_goal = stop_at_goal and pm.goal
                if (inside and c not in closed) or at_goal:
                    closed.add(c)
                    states.append(pm.next_state)
                    canons.append(c[0] if inside else (0, 0))
                    links.append(Link(k, pm.frm, pm.action, pm.walk, bool(pm.goal)))
                if at_goal:
                    goal_index = len(states) - 1
                    break
        fresh = list(range(first, len(states)))
        if fresh:
            layers.append((first, len(fresh)))
        if goal_index >= 0:
            return Store(states, canons, links, layers, layer_states, len(states), goal_index, depth, rows, largest)
        layer_states.append(len(fresh))
        frontier = fresh
    return Store(states, canons, links, layers, layer_states, len(states), -1, None, rows, largest)


def plan_of(p, store, index):
    """The primitive actions from the start to state ``index``: the parent actions of the walk regions between the pushes."""
    plan = []
    while store.links[index].parent >= 0:
        ln = store.links[index]
        plan = WR.path(WR.region(p, store.states[ln.parent]), ln.frm) + [ln.action] + plan
        index = ln.parent
    return plan

"""Plain-Python restatement of drawing from the BATCHED cost-to-go tables over pushes (``pw_push_solve_batch_index`` / ``_sample``
/ ``_plans`` / ``_emit``) over ``push_table_restatement.Table`` plus the packed keys of its states
(``push_solution_batch_restatement.pack_key``).  A helper of tests/test_push_batch_sample_host.py and
tests/test_gpu_push_batch_sample.py, not a test.

Only the index is new: the STATES grouped by cost, the dead ends last, in ascending 64-BIT KEY inside a bucket -- the batched
kernel numbers the states of a layer as its schedule has it, the key (the canonical state) is the same in every run.  The
draw, both tie rules and the rows are ``push_table_sample_restatement``'s; a state of the batch is its canonical state (the agent
at the canon of its walk region), and the emitted states come from the C oracle alone (``states_along``), never from the store."""
import push_solution_batch_restatement as BR
import push_table_sample_restatement as SR
from push_table_sample_restatement import Row, Step, draw_state, plan, states_along  # noqa: F401  (the shared parts)


def keys_of_table(t):
    """The packed key of every state of a ``Table``, as a list of Python ints."""
    return [BR.pack_key(c, s) for s, c in zip(t.store.states, t.store.canons)]


def cost_index(t, keys):
    """(states_by_cost, cost_start) of a ``Table`` whose state i has the key ``keys[i]``: cost_start has max_cost + 3 words,
    [0, S] when no cost is finite; ascending key inside every bucket."""
    mc = t.info[4]
    buckets = [[] for _ in range(mc + 2)]
    for i in sorted(range(len(t.cost)), key=lambda i: int(keys[i])):
        c = t.cost[i]
        buckets[c if c >= 0 else mc + 1].append(i)
    start = [0]
    for b in buckets:
        start.append(start[-1] + len(b))
    return [i for b in buckets for i in b], start


def canonical(t, node):
    """The state a key unpacks to: the movables of the stored state with the agent at the canon of its walk region."""
    return (tuple(t.store.canons[node]),) + tuple(tuple(xy) for xy in t.store.states[node][1:])


def rows(cp, t, item, start, steps):
    """The emitted rows of one item whose live state is ``start`` (None: the canonical state of its first node)."""
    if not steps:
        return []
    return SR.rows(cp, t, item, canonical(t, steps[0].node) if start is None else start, steps)

"""Plain-Python restatement of pushes unrolled into primitive actions (``pw_push_unroll_count`` / ``_write`` / ``_plans``,
DESIGN.md K21) over ``walk_restatement.region`` / ``path`` and ``push_step_restatement.is_valid``.  The only reference of the
unroll tests.  A helper, not a test.

Definitions, for an item with state ``s`` and a choice ``(frm, a)``:
  valid     ``push_step_restatement.is_valid``: ``a`` in 0..3, ``frm`` in the walk region R(s), ``(frm, a)`` a push move
  L         ``walk_restatement.path(R(s), frm) + [a]``: ``dist(frm) + 1`` actions
  refused   a masked item, a puzzle id outside the set (``cp`` None), a movable outside its grid, a choice that is not valid:
            length -1 and no actions
  offset    the exclusive scan of ``max(length, 0)``; ``actions`` is every item's L, one after the other
  plans     rows ``item_offset[j] : item_offset[j + 1]`` are the pushes of plan j: its actions are the rows' L concatenated,
            ``plan_len`` their number, -1 when a row is refused, 0 without rows; a plan array holds the first ``plan_cap``."""
import push_step_restatement as SR
import walk_restatement as WR


def unroll(cp, state, frm, action, masked=False, reg=None):
    """L of one item, or None when it is refused.  ``reg``: ``walk_restatement.region(cp, state)`` if the caller has it."""
    if masked or cp is None:
        return None
    state = tuple(tuple(xy) for xy in state)
    frm = (int(frm[0]), int(frm[1]))
    reg = SR.is_valid(cp, state, frm, int(action), reg)
    if reg is None:
        return None
    seq = WR.path(reg, frm) + [int(action)]
    assert len(seq) == reg.dist[frm] + 1
    return seq


def flatten(seqs):
    """(length, offset, actions) of the items' sequences (None: refused)."""
    length = [-1 if s is None else len(s) for s in seqs]
    offset = [0]
    for n in length:
        offset.append(offset[-1] + max(n, 0))
    return length, offset, [a for s in seqs if s is not None for a in s]


def plans(item_offset, seqs, plan_cap):
    """(plans, plan_len): ``plans[j]`` the first ``plan_cap`` actions of plan j (a list; [] when there is no plan)."""
    out, lens = [], []
    for j in range(len(item_offset) - 1):
        rows = seqs[item_offset[j]:item_offset[j + 1]]
        if any(s is None for s in rows):
            out.append([])
            lens.append(-1)
            continue
        acts = [a for s in rows for a in s]
        out.append(acts[:plan_cap])
        lens.append(len(acts))
    return out, lens

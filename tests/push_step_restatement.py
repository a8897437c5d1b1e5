"""Plain-Python restatement of the macro step over pushes (``pw_step_push``) over ``walk_restatement.region`` /
``path`` and the environment step of the compiled C oracle (``oracle.c_oracle.COraclePuzzle.env_step``).  The only reference
of the push-step tests.  A helper, not a test.

Definitions, for a live environment with state ``s`` and a choice ``(frm, a)``:
  valid        ``a`` in 0..3, ``frm`` in the walk region R(s) and ``(frm, a)`` a push move of ``s``: the step moves the agent and at
               least one other movable.  Anything else is refused, and so is an environment the walk regions would skip (a
               puzzle id outside the set: ``cp`` None; a movable outside its grid).
  macro step   the primitive step applied with ``path(R(s), frm) + [a]`` in turn, without autoreset inside, ended by the first
               step that returns terminated | truncated.  ``reward`` is the sum of the executed steps' rewards in execution
               order, ``dgoals`` the sum of theirs, ``moves`` their number; ``status`` DONE when the push itself was executed,
               CUT when the macro step ended during the walk.
  refused      everything stays as it was; reward 0.0, dgoals 0, moves 0, status REFUSED.
  autoreset    an environment whose terminated | truncated is set on entry returns to the initial state with steps 0, flags 0,
               reward 0.0: moves 0, status RESET, the choice is not read.
The device counters advance by what the executed primitive steps add: ``Counts`` sums env-steps, episodes ended and solved."""
from collections import namedtuple

import walk_restatement as WR

REFUSED, DONE, CUT, RESET = 0, 1, 2, 3

Env = namedtuple("Env", "state steps terminated truncated")
Result = namedtuple("Result", "state steps reward dgoals terminated truncated moves status")


def goals_met(cp, state):
    return sum(1 for g, xy in enumerate(cp.py.goal_state) if tuple(state[1 + g]) == tuple(xy))


def primitive(cp, state, steps, action, max_steps):
    """One environment step: (next state, steps, reward, dgoals, terminated, truncated)."""
    nxt, reward, terminated = cp.env_step(state, action)
    steps += 1
    truncated = max_steps is not None and steps >= max_steps
    return nxt, steps, reward, goals_met(cp, nxt) - goals_met(cp, state), bool(terminated), bool(truncated)


def is_valid(cp, state, frm, action, reg=None):
    """The walk region of ``state`` when ``(frm, action)`` is a valid choice, else None (``reg``: that region, if the caller has
    it already)."""
    if cp is None or not WR.in_grid(cp, state) or action not in (0, 1, 2, 3):
        return None
    reg = WR.region(cp, state) if reg is None else reg
    frm = (int(frm[0]), int(frm[1]))
    if frm not in reg.dist:
        return None
    _, moved = cp.get_next_state_moved((frm,) + tuple(state[1:]), action)
    return reg if len(moved) > 1 else None


def macro_step(cp, env, frm, action, max_steps=None, autoreset=False, initial=None, reg=None):
    """``Result`` of one macro step of ``env`` (an ``Env``) of puzzle ``cp`` (None: a puzzle id outside the set; ``initial``
    is then the state an autoreset returns to).  ``reg``: ``walk_restatement.region(cp, env.state)`` if the caller has it."""
    state = tuple(tuple(xy) for xy in env.state)
    if autoreset and (env.terminated or env.truncated):
        return Result(tuple(initial if initial is not None else cp.initial_state), 0, 0.0, 0, 0, 0, 0, RESET)
    reg = is_valid(cp, state, frm, action, reg)
    if reg is None:
        return Result(state, env.steps, 0.0, 0, env.terminated, env.truncated, 0, REFUSED)
    actions = WR.path(reg, (int(frm[0]), int(frm[1]))) + [int(action)]
    assert len(actions) == reg.dist[(int(frm[0]), int(frm[1]))] + 1
    steps, total, dgoals, moves = env.steps, None, 0, 0
    terminated = truncated = False
    for a in actions:
        state, steps, r, dg, terminated, truncated = primitive(cp, state, steps, a, max_steps)
        total = r if total is None else total + r  # ((r1 + r2) + r3) + ...
        dgoals += dg
        moves += 1
        if terminated or truncated:
            break
    status = DONE if moves == len(actions) else CUT
    return Result(state, steps, total, dgoals, int(terminated), int(truncated), moves, status)


class Counts:
    """What the device counters gain: every executed primitive step is an env-step; a macro step whose last step returned
    terminated | truncated ended an episode, terminated solved it.  A reset and a refusal execute no step."""

    def __init__(self):
        self.env_steps = self.ended = self.solved = 0

    def add(self, res):
        self.env_steps += res.moves
        if res.moves and (res.terminated or res.truncated):
            self.ended += 1
        if res.moves and res.terminated:
            self.solved += 1

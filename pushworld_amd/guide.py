"""Cost-to-go guidance inside the step (``pw_guide_step``).

A ``ValueGuide`` holds, per environment of a ``VecPushWorld``, the exact cost-to-go of its current state, the optimal and
safe action bits, the dead-end flag and the potential-shaped reward of the last step, plus counts per puzzle of guided /
optimal / dead-entering / unknown steps.  ``VecPushWorld.set_guide`` puts one launch behind every ``step`` / ``step_push`` /
``step_push_mask`` that keeps them current; with ``end_dead`` that launch truncates an environment that has just entered a
dead end, so that autoreset restarts it instead of stepping a lost state until ``max_steps``.
"""
from __future__ import annotations

import math
from collections import namedtuple
from typing import Optional

import numpy as np
import torch

from . import _capi

GuideStats = namedtuple("GuideStats", "guided optimal dead_entered unknown optimal_rate")
GuideStats.__doc__ = """What ``ValueGuide.stats`` returns: numpy arrays [P], int64 counts and ``optimal_rate`` = optimal / guided
(NaN for a puzzle without a guided step)."""

_MOVE, _PUSH = "move", "push"


def _level(table) -> str:
    from .search import PushSolutionTable, PushSolutionTableBatch, SolutionTable, SolutionTableBatch

    if isinstance(table, (SolutionTable, SolutionTableBatch)):
        return _MOVE
    if isinstance(table, (PushSolutionTable, PushSolutionTableBatch)):
        return _PUSH
    raise ValueError("tables must be SolutionTable / SolutionTableBatch (moves) or PushSolutionTable / PushSolutionTableBatch "
                     f"(pushes) objects, not {type(table).__name__}")


def _table_engine(table):
    return table.engine if hasattr(table, "engine") else table.search._engine


def check_guide_options(gamma, scale, dead_cost, end_dead, autoreset) -> None:
    """The refusals of ``ValueGuide`` that need neither tables nor an engine."""
    for name, v in (("gamma", gamma), ("scale", scale)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
            raise ValueError(f"{name} must be a finite number, not {v!r}")
    if dead_cost is not None and (isinstance(dead_cost, bool) or not isinstance(dead_cost, (int, np.integer))
                                  or not 0 <= int(dead_cost) < 1 << 31):
        raise ValueError(f"dead_cost must be None or an int in 0 .. 2^31 - 1, not {dead_cost!r}")
    if end_dead and not autoreset:
        raise ValueError("end_dead needs autoreset=True: a cut episode is restarted by the next step's autoreset")


class ValueGuide:
    """Exact cost-to-go guidance for the environments of ``source``, kept current by one launch per step.

    Args:
        source: the ``VecPushWorld`` whose states are looked up.
        tables: ONE ``SolutionTableBatch`` -- the fused form: the launch does the hashed lookup itself -- or a list of tables
            of one level -- the applied form: the guide calls each table's own ``query`` into its buffers before the launch.
            ``SolutionTable`` / ``SolutionTableBatch`` are move-level; ``PushSolutionTable`` / ``PushSolutionTableBatch`` are
            push-level: their costs are in pushes and every query costs a flood.  Mixed levels are refused.  The tables must
            be made on the environment's engine, as ``cost_to_go`` demands.
        gamma, scale: the shaped reward is ``reward + gamma * phi(s') - phi(s)`` with ``phi(s) = -scale * cost(s)``.
        dead_cost: the cost that stands for a dead end in ``phi``: an int for every puzzle, or None = per puzzle the largest
            finite cost of its table plus 1 (0 without a table); None reads the tables' summaries and may wait.
        end_dead: truncate an environment that has just entered a dead end (needs ``autoreset``).
        shaping, counts: leave out the shaped reward / the counts per puzzle.

    Device tensors, allocated here and never again: ``cost`` int32 [B] (-1 dead end, -2 unknown), ``acts`` uint8 [B], ``dead``
    uint8 [B], ``seen`` uint8 [B], ``shaped`` float64 [B] or None, ``counts`` int64 [P, 4] or None, ``dead_cost`` int32 [P].
    """

    def __init__(self, source, tables, gamma: float = 1.0, scale: float = 1.0, dead_cost: Optional[int] = None,
                 end_dead: bool = False, shaping: bool = True, counts: bool = True):
        from .search import SolutionTableBatch
        from .vec_env import VecPushWorld

        if not isinstance(source, VecPushWorld):
            raise ValueError("expected a VecPushWorld")
        autoreset = bool(source.flags & _capi.STEP_AUTORESET)
        check_guide_options(gamma, scale, dead_cost, end_dead, autoreset)
        fused = isinstance(tables, SolutionTableBatch)
        tables = [tables] if fused else list(tables) if isinstance(tables, (list, tuple)) else None
        if not tables:
            raise ValueError("tables must be one SolutionTableBatch or a non-empty list of cost-to-go tables")
        levels = {_level(t) for t in tables}
        if len(levels) != 1:
            raise ValueError("tables of mixed levels (moves and pushes) cannot guide one environment: their costs do not compare")
        for t in tables:
            if _table_engine(t) is not source.engine:
                raise ValueError("the tables must be made on this environment (VecPushWorld.solution_table(s) / push_table(s))")
        self.vec, self.engine, self.device = source, source.engine, source.device
        self.tables, self.fused, self.level = tables, fused, levels.pop()
        self.gamma, self.scale, self.end_dead = float(gamma), float(scale), bool(end_dead)
        B, P, dev = source.num_envs, source.num_puzzles, source.device
        self.num_puzzles = P
        self.cost = torch.full((B,), -2, dtype=torch.int32, device=dev)
        self.acts = torch.zeros((B,), dtype=torch.uint8, device=dev)
        self.dead = torch.zeros((B,), dtype=torch.uint8, device=dev)
        self.seen = torch.zeros((B,), dtype=torch.uint8, device=dev)
        self.shaped = torch.zeros((B,), dtype=torch.float64, device=dev) if shaping else None
        self.counts = torch.zeros((P, _capi.GUIDE_COUNTS), dtype=torch.int64, device=dev) if counts else None
        self.dead_cost = torch.zeros((P,), dtype=torch.int32, device=dev)
        if dead_cost is None:
            self._default_dead_cost()
        else:
            self.dead_cost.fill_(int(dead_cost))
        # the applied form's own buffers: what the tables' queries write and the launch reads and clears
        self._query = self._cost_in = self._acts_in = None
        if not fused:
            if self.level == _MOVE:
                from .search import _query_outputs

                self._query = _query_outputs(None, B, dev)
                self._cost_in, self._acts_in = self._query[1], self._query[2]
            else:
                from .search import _push_query_outputs

                self._query = _push_query_outputs(None, B, dev)
                self._cost_in = self._query.cost
        self._flags = (_capi.GUIDE_AUTORESET if autoreset else 0) | (_capi.GUIDE_END_DEAD if self.end_dead else 0)
        self._call = self.engine.bind_guide_step(*self._args(None, self._flags))

    def _default_dead_cost(self) -> None:
        """Per puzzle the largest finite cost of its table + 1 (the highest over the tables that hold it), 0 without one."""
        host = np.zeros((self.num_puzzles,), dtype=np.int64)
        for t in self.tables:
            if hasattr(t, "puzzles"):  # a batch: the items with a stored table
                status, mc = t.status.cpu().numpy(), t.max_cost.cpu().numpy()
                for item, p in enumerate(t.puzzles):
                    if status[item] == 0:
                        host[p] = max(host[p], int(mc[item]) + 1)
            else:
                host[t.puzzle_index] = max(host[t.puzzle_index], int(t.max_cost) + 1)
        self.dead_cost.copy_(torch.as_tensor(host.astype(np.int32)))

    def _args(self, mask, flags):
        v = self.vec
        return (self.tables[0].handle if self.fused else None, self._cost_in, self._acts_in, v.puzzle_id, v.pos,
                v.reward if self.shaped is not None else None, v.terminated, v.truncated, mask, self.cost, self.acts, self.seen,
                self.dead, self.shaped, self.dead_cost, self.gamma, self.scale, self.counts, flags)

    def _lookups(self, mask=None) -> None:
        """The applied form's queries: every table answers for its own puzzles into the guide's buffers."""
        if self.fused:
            return
        v = self.vec
        for t in self.tables:
            if self.level == _MOVE:
                t.query(v.puzzle_id, v.pos, mask=mask, out=self._query)
            else:
                t.query(v.puzzle_id, v.pos, mask=mask, out=self._query, actions=False)

    def step(self) -> None:
        """What ``VecPushWorld`` calls behind a step launch: the lookups (applied form) and the one guide launch."""
        self._lookups()
        self._call()

    def refresh(self, mask: Optional[torch.Tensor] = None) -> None:
        """Looks the (masked) environments' current states up again without counting or shaping anything
        (``PW_GUIDE_REFRESH``): what ``reset``, ``set_states`` and the like call.  No wait."""
        if mask is not None:
            mask = mask.to(device=self.device, dtype=torch.uint8)
        self._lookups(mask)
        self.engine.guide_step(*self._args(mask, _capi.GUIDE_REFRESH))

    def stats(self) -> GuideStats:
        """The counts per puzzle as numpy arrays with ``optimal_rate``; waits for the stream."""
        if self.counts is None:
            raise RuntimeError("this ValueGuide keeps no counts (counts=False)")
        c = self.counts.cpu().numpy()
        guided, optimal = c[:, _capi.GUIDE_GUIDED], c[:, _capi.GUIDE_OPTIMAL]
        with np.errstate(divide="ignore", invalid="ignore"):
            rate = np.where(guided > 0, optimal / np.maximum(guided, 1), np.nan)
        return GuideStats(guided, optimal, c[:, _capi.GUIDE_DEAD_ENTERED], c[:, _capi.GUIDE_UNKNOWN], rate)

    @property
    def optimal_actions(self) -> torch.Tensor:
        """uint8 [B]: bit a = action a is optimal (``acts & 15``)."""
        return self.acts & 15

    @property
    def safe_actions(self) -> torch.Tensor:
        """uint8 [B]: bit a = action a does not enter a dead end (``acts >> 4``); meaningful for move-level tables only."""
        return self.acts >> 4

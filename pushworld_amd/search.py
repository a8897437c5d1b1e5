"""Breadth-first search with the frontier and the closed set on the GPU.

The reference planner (cpp/include/search/best_first_search.h:72-93) pops one node at a time and
calls ``getNextState`` four times; ``BreadthFirstSearch`` expands a whole layer per call through the
``pw_search_*`` entry points.  State numbering is deterministic: it is the numbering of a sequential
FIFO search that tries the actions in the order LEFT, RIGHT, UP, DOWN, so plans are the first
shortest plan in that order.
"""
from __future__ import annotations

import ctypes
from collections import namedtuple
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _capi
from .puzzle import PushWorldPuzzle

POSITION_LIMIT = 10000  # pushworld_puzzle.h:37


class LayerInfo(tuple):
    """(depth, new_states, total_states, goal_index) of one ``expand`` call."""

    depth = property(lambda self: self[0])
    new_states = property(lambda self: self[1])
    total_states = property(lambda self: self[2])
    goal_index = property(lambda self: self[3])


class BreadthFirstSearch:
    """Layer-synchronous BFS over the states of one puzzle.

    Args:
        puzzle: a ``PushWorldPuzzle`` (object order as parsed: Python order by default).
        max_states: capacity of the state store (device memory ~ ``max_states * (2 N + 21)`` bytes).
        chunk: parents per expansion pass (default 2^20; tests use small values to force many passes per layer).
        novelty_width: 0 = breadth-first search; 1 or 2 = width-limited search IW(k): new states whose
            novelty (reference ``NoveltyHeuristic``, novelty.cc:30-77) exceeds the width are closed but
            never expanded.  Incomplete but usually far smaller; plans are no longer guaranteed shortest.
    """

    def __init__(self, puzzle: PushWorldPuzzle, max_states: int = 1 << 22, novelty_width: int = 0,
                 chunk: Optional[int] = None):
        self.puzzle = puzzle
        self._engine = puzzle._engine()
        self.device = self._engine.device
        self.num_objects = puzzle.num_movables
        self.max_states = int(max_states)
        h = ctypes.c_void_p()
        self.novelty_width = int(novelty_width)
        self._engine.set_option("search_chunk", 0 if chunk is None else int(chunk))
        try:
            _capi.check(_capi.lib.pw_search_create(self._engine.handle, int(getattr(puzzle, "puzzle_index", 0)),
                                                   self.max_states, self.novelty_width, ctypes.byref(h)))
        finally:
            self._engine.set_option("search_chunk", 0)
        self.handle = h
        self.total_states = 0
        self.layers: List[Tuple[int, int]] = []  # (first index, count) per depth
        self.goal_index = -1
        self.exhausted = False

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def begin(self, start: Optional[Sequence[Tuple[int, int]]] = None) -> None:
        """Starts a search from ``start`` (a reference-style state, default: the initial state)."""
        arr = None
        if start is not None:
            if len(start) != self.num_objects:
                raise ValueError("start must hold one (x, y) pair per movable")
            arr = (ctypes.c_int32 * self.num_objects)(*[int(x) * POSITION_LIMIT + int(y) for x, y in start])
        _capi.check(_capi.lib.pw_search_begin(self.handle, arr, self._stream()))
        self.total_states = 1
        self.layers = [(0, 1)]
        state0 = tuple(start) if start is not None else self.puzzle.initial_state
        self.goal_index = 0 if self.puzzle.is_goal_state(state0) else -1
        self.exhausted = False

    def expand(self) -> LayerInfo:
        """Expands the newest layer; raises ``ValueError`` when the store is full."""
        info = (ctypes.c_int64 * 4)()
        rc = _capi.lib.pw_search_expand(self.handle, info, self._stream())
        depth, new, total, goal = (int(v) for v in info)
        if rc == _capi.PW_ELIMIT and total > self.total_states:  # store full: the last layer is incomplete
            self.layers.append((total - new, new))
            self.total_states = total
            self.goal_index = goal
        _capi.check(rc)
        if new:
            self.layers.append((total - new, new))
        else:
            self.exhausted = True
        self.total_states = total
        self.goal_index = goal
        return LayerInfo((depth, new, total, goal))

    def states(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """int array [count, N, 2] of (x, y) positions of states ``first .. first + count - 1``."""
        count = self.total_states - first if count is None else count
        out = torch.empty((count, self.num_objects), dtype=torch.int32, device=self.device)
        _capi.check(_capi.lib.pw_search_read_states(self.handle, first, count, _capi._ptr(out), self._stream()))
        v = out.cpu().numpy()
        return np.stack([v // POSITION_LIMIT, v % POSITION_LIMIT], axis=-1)

    def links(self, first: int = 0, count: Optional[int] = None):
        """(parent int32 [count], action uint8 [count]); the start state has parent -1."""
        count = self.total_states - first if count is None else count
        par = torch.empty((count,), dtype=torch.int32, device=self.device)
        act = torch.empty((count,), dtype=torch.uint8, device=self.device)
        _capi.check(_capi.lib.pw_search_read_links(self.handle, first, count, _capi._ptr(par), _capi._ptr(act),
                                                   self._stream()))
        return par.cpu().numpy(), act.cpu().numpy()

    def pruned(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """bool [count]: states cut by the novelty width (closed, never expanded)."""
        count = self.total_states - first if count is None else count
        out = torch.empty((count,), dtype=torch.uint8, device=self.device)
        _capi.check(_capi.lib.pw_search_read_flags(self.handle, first, count, _capi._ptr(out), self._stream()))
        return out.cpu().numpy().astype(bool)

    def plan(self, index: int) -> List[int]:
        """Actions leading from the start state to state ``index``."""
        cap = 256
        while True:
            buf = (ctypes.c_uint8 * cap)()
            n = _capi.check(_capi.lib.pw_search_plan(self.handle, int(index), buf, cap, self._stream()))
            if n <= cap:
                return [int(buf[i]) for i in range(n)]
            cap = n

    def solve(self, max_depth: Optional[int] = None) -> Optional[List[int]]:
        """A shortest plan (first in L, R, U, D order), or None if the reachable space holds no goal
        state within ``max_depth``.  ``ValueError`` if ``max_states`` is exhausted first."""
        if not self.layers:
            self.begin()
        while self.goal_index < 0 and not self.exhausted:
            if max_depth is not None and len(self.layers) - 1 >= max_depth:
                return None
            self.expand()
        return self.plan(self.goal_index) if self.goal_index >= 0 else None

    def close(self) -> None:
        h = getattr(self, "handle", None)
        if h and _capi.lib is not None:
            _capi.lib.pw_search_destroy(h)
            self.handle = None

    __del__ = close


class SetPuzzle:
    """Puzzle ``index`` of a packed ``_capi.PuzzleSet`` as ``BreadthFirstSearch`` needs it (number of movables,
    initial state, goal test, a state-only engine shared by all puzzles of the set) -- for sets that never existed
    as text (``generate.generate_level0_set``).  Reads the packed header (csrc/pw_format.h)."""

    def __init__(self, pset: "_capi.PuzzleSet", index: int, engine: Optional["_capi.Engine"] = None):
        hdr = pset.headers()[320 * index:320 * (index + 1)]
        self.puzzle_index = int(index)
        self.num_movables, n_goals = hdr[6], hdr[7]
        i8 = np.frombuffer(hdr, dtype=np.int8)
        self.initial_state = tuple((int(i8[256 + 2 * j]), int(i8[257 + 2 * j])) for j in range(self.num_movables))
        self.goal_state = tuple((int(i8[192 + 2 * g]), int(i8[193 + 2 * g])) for g in range(n_goals))
        self._eng = engine if engine is not None else _capi.Engine(pset, None, 3, 1, _capi.OBS_U8)

    def _engine(self):
        return self._eng

    def is_goal_state(self, state) -> bool:
        return tuple(tuple(int(v) for v in p) for p in state[1:1 + len(self.goal_state)]) == self.goal_state


class NoveltyTables:
    """Batched ``NoveltyHeuristic`` (cpp/src/heuristics/novelty.cc:30-77): ``evaluate`` returns, for an
    array of states, the values the reference would return when fed the states one by one in order."""

    def __init__(self, state_size: int, width: int, height: int, device: Optional[int] = None):
        from .puzzle import default_device_index

        self.device_index = default_device_index() if device is None else int(device)
        self.device = torch.device("cuda", self.device_index)
        self.state_size = int(state_size)
        h = ctypes.c_void_p()
        _capi.check(_capi.lib.pw_novelty_create(self.device_index, self.state_size, int(width), int(height),
                                                ctypes.byref(h)))
        self.handle = h

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def reset(self) -> None:
        _capi.check(_capi.lib.pw_novelty_reset(self.handle, self._stream()))

    def evaluate(self, states: torch.Tensor, moved: torch.Tensor) -> torch.Tensor:
        """``states`` int32 [F, N] Position2D (x * 10000 + y), ``moved`` int32/uint32-bit masks [F];
        returns uint8 [F] novelties (1, 2 or 3)."""
        if states.dtype != torch.int32 or states.dim() != 2 or states.shape[1] != self.state_size or \
                not states.is_contiguous() or states.device != self.device:
            raise ValueError("states must be a contiguous int32 tensor [F, state_size] on the tables' device")
        if moved.shape != (states.shape[0],) or moved.dtype not in (torch.int32, torch.uint32) or moved.device != self.device:
            raise ValueError("moved must be an int32 tensor [F] of bit masks on the tables' device")
        out = torch.empty((states.shape[0],), dtype=torch.uint8, device=self.device)
        _capi.check(_capi.lib.pw_novelty_eval(self.handle, _capi._ptr(states), _capi._ptr(moved), _capi._ptr(out),
                                              states.shape[0], self._stream()))
        return out

    def close(self) -> None:
        h = getattr(self, "handle", None)
        if h and _capi.lib is not None:
            _capi.lib.pw_novelty_destroy(h)
            self.handle = None

    __del__ = close


class RecursiveGraphDistance:
    """Batched ``RecursiveGraphDistanceHeuristic`` (cpp/src/heuristics/recursive_graph_distance.cc:43-252) of one puzzle:
    ``evaluate`` returns for every state what ``estimate_cost_to_goal`` returns (+inf: provably no way to the goal).

    Args:
        puzzle: a ``PushWorldPuzzle`` (or a ``SetPuzzle``).
        fewest_tools: True (the reference default, what ``run_planner`` uses): the cost of the fewest tools that gives a
            finite cost; False: every goal is searched with up to N - 2 tools.
        budget: recursion frames one state may take (None: ``pw_rgd_create``'s default, 4 096).  States that need more
            get NaN and count in ``exceeded``.

    States with a movable off its own movement graph get NaN too (the reference throws); reachable states never do.
    """

    def __init__(self, puzzle, fewest_tools: bool = True, budget: Optional[int] = None):
        self.puzzle = puzzle
        self._engine = puzzle._engine()
        self.device = self._engine.device
        self.num_objects = puzzle.num_movables
        self.fewest_tools = bool(fewest_tools)
        if budget is not None and int(budget) <= 0:
            raise ValueError("budget must be a positive number of frames (or None for the default)")
        h = ctypes.c_void_p()
        _capi.check(_capi.lib.pw_rgd_create(self._engine.handle, int(getattr(puzzle, "puzzle_index", 0)),
                                            1 if self.fewest_tools else 0, 0 if budget is None else int(budget),
                                            ctypes.byref(h)))
        self.handle = h

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def evaluate(self, states: torch.Tensor) -> torch.Tensor:
        """``states`` int32 [F, N] Position2D (x * 10000 + y) on the puzzle's device, e.g. ``expand4``'s successors
        reshaped to [F * 4, N]; returns float32 [F] costs, computed on the current stream."""
        if not isinstance(states, torch.Tensor) or states.dtype != torch.int32 or states.dim() != 2 or \
                states.shape[1] != self.num_objects or not states.is_contiguous() or states.device != self.device:
            raise ValueError("states must be a contiguous int32 tensor [F, num_movables] on the puzzle's device")
        out = torch.empty((states.shape[0],), dtype=torch.float32, device=self.device)
        if states.shape[0]:
            _capi.check(_capi.lib.pw_rgd_eval(self.handle, _capi._ptr(states), _capi._ptr(out), states.shape[0],
                                              self._stream()))
        return out

    def movement_graph(self, obj: int):
        """``{(x, y): {(x, y), ...}}``: the feasible-movement graph of movable ``obj`` (host computed)."""
        return self.puzzle.movement_graph(obj)

    def distance(self, obj: int, src, dst):
        """Graph distance of movable ``obj`` (``PathDistances::getDistance``).  ``src`` / ``dst`` are (x, y) pairs (a float
        comes back) or int32 tensors [K] of Position2D on the device (a float32 tensor [K] comes back)."""
        if not 0 <= int(obj) < self.num_objects:
            raise ValueError("obj must be a movable index of the puzzle")
        scalar = not isinstance(src, torch.Tensor)
        if scalar:
            src = torch.tensor([int(src[0]) * POSITION_LIMIT + int(src[1])], dtype=torch.int32, device=self.device)
            dst = torch.tensor([int(dst[0]) * POSITION_LIMIT + int(dst[1])], dtype=torch.int32, device=self.device)
        for t in (src, dst):
            if t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous() or t.device != self.device:
                raise ValueError("src and dst must be contiguous int32 tensors [K] on the puzzle's device")
        if src.shape != dst.shape:
            raise ValueError("src and dst must have the same shape")
        out = torch.empty(src.shape, dtype=torch.float32, device=self.device)
        if src.shape[0]:
            _capi.check(_capi.lib.pw_rgd_distances(self.handle, int(obj), _capi._ptr(src), _capi._ptr(dst), _capi._ptr(out),
                                                   src.shape[0], self._stream()))
        return float(out.item()) if scalar else out

    @property
    def exceeded(self) -> int:
        """States that ran out of budget since this object was created (synchronises the current stream)."""
        return _capi.check(_capi.lib.pw_rgd_exceeded(self.handle, self._stream()))

    def close(self) -> None:
        h = getattr(self, "handle", None)
        if h and _capi.lib is not None:
            _capi.lib.pw_rgd_destroy(h)
            self.handle = None

    __del__ = close


VERDICT_UNSOLVABLE, VERDICT_SOLVED, VERDICT_UNKNOWN, VERDICT_NOT_SEARCHED = 0, 1, 2, 3


def search_batch(engine, puzzle_indices=None, max_states: int = 1 << 16, plan_cap: int = 0):
    """``pw_search_batch``: breadth-first search of MANY small puzzles of ``engine``'s set in one launch (persistent workgroups,
    the whole search loop inside the kernel).  Returns numpy arrays ``(verdict uint8 [n], plan_len int32 [n], num_states
    int32 [n])``: verdict 1 solved (``plan_len`` = length of a shortest plan), 0 unsolvable, 2 unknown (more than
    ``max_states`` states), 3 not searched (beyond 16 x 16 cells / 8 movables: use ``BreadthFirstSearch``).  With
    ``plan_cap`` > 0 a fourth value: the list of plans (lists of actions; None where there is none or it is longer)."""
    dev = engine.device
    if puzzle_indices is None:
        n = len(engine.pset)
        idx = None
    else:
        idx = torch.as_tensor(np.asarray(puzzle_indices), dtype=torch.int32).to(dev)
        n = int(idx.shape[0])
    verdict = torch.empty((n,), dtype=torch.uint8, device=dev)
    plan_len = torch.empty((n,), dtype=torch.int32, device=dev)
    states = torch.empty((n,), dtype=torch.int32, device=dev)
    plans = torch.zeros((n, plan_cap), dtype=torch.uint8, device=dev) if plan_cap > 0 else None
    if n:
        _capi.check(_capi.lib.pw_search_batch(engine.handle, _capi._ptr(idx), n, int(max_states), 0, _capi._ptr(verdict),
                                              _capi._ptr(plan_len), _capi._ptr(states), _capi._ptr(plans), int(plan_cap),
                                              engine._stream()))
    v, pl, ns = verdict.cpu().numpy(), plan_len.cpu().numpy(), states.cpu().numpy()
    if plan_cap <= 0:
        return v, pl, ns
    ph = plans.cpu().numpy()
    return v, pl, ns, [ph[i, :pl[i]].tolist() if v[i] == VERDICT_SOLVED and 0 <= pl[i] <= plan_cap else None for i in range(n)]


def shortest_plan(puzzle, max_states: int = 1 << 20, plan_cap: int = 4096):
    """``(plan, verdict)`` of ONE puzzle from a single launch (``pw_search_batch`` with n = 1): the whole breadth-first search
    runs inside the kernel, so a search of a few dozen states costs one launch and one readback instead of a handful of
    launches and a readback per layer.  ``plan`` is a shortest plan (list of actions) or None; verdict as ``search_batch``.
    Puzzles beyond the kernel's limits (verdict 3) and searches beyond ``max_states`` (2) are ``BreadthFirstSearch``'s."""
    eng = puzzle._engine()
    v, pl, ns, plans = search_batch(eng, [int(getattr(puzzle, "puzzle_index", 0))], max_states=max_states, plan_cap=plan_cap)
    return plans[0], int(v[0])


PLAN_RUNNING, PLAN_SOLVED, PLAN_EXHAUSTED, PLAN_LIMIT = 0, 1, 2, 3
PLAN_STATUS = {PLAN_RUNNING: "running", PLAN_SOLVED: "solved", PLAN_EXHAUSTED: "exhausted", PLAN_LIMIT: "limit"}
PLAN_MODES = {"RGD": 0, "N+RGD": 1}
PLAN_ACTION_ORDERS = {"reference": 0, "fixed": 1}


class PlannerInfo(tuple):
    """(status, rounds, expanded, visited, open, goal_index, rgd_exceeded, stored) of a ``BestFirstSearch``."""

    status = property(lambda self: PLAN_STATUS[self[0]])
    rounds = property(lambda self: self[1])
    expanded = property(lambda self: self[2])
    visited = property(lambda self: self[3])
    open = property(lambda self: self[4])
    goal_index = property(lambda self: self[5])
    rgd_exceeded = property(lambda self: self[6])
    stored = property(lambda self: self[7])


def action_groups() -> List[Tuple[int, int, int, int]]:
    """The reference's 1000 action groups (``RandomActionIterator``, std::shuffle with std::default_random_engine(42))."""
    buf = (ctypes.c_uint8 * 4000)()
    _capi.check(_capi.lib.pw_planner_action_groups(buf))
    return [tuple(buf[4 * g: 4 * g + 4]) for g in range(1000)]


class BestFirstSearch:
    """The reference planner (``run_planner``: best-first search over a bucket queue, best_first_search.h:45-98) on the
    GPU, popping ``batch`` = K states per round (K = 1 is the reference algorithm).  See ``pw_planner_create`` in
    include/pushworld_amd.h for the exact semantics.

    Args:
        puzzle: a ``PushWorldPuzzle`` (parse with ``order="cpp"`` for the reference binary's object order).
        heuristic: ``"RGD"`` or ``"N+RGD"`` (novelty first, then RGD).
        batch: states popped per round.
        max_states: capacity of the state store; a round is not started when it could overflow (status ``limit``).
        action_order: ``"reference"`` (RandomActionIterator groups) or ``"fixed"`` (L, R, U, D).
        rgd_budget: RGD recursion frames per state (None: the default); states beyond it get NaN keys and pop last.
    """

    def __init__(self, puzzle: PushWorldPuzzle, heuristic: str = "N+RGD", batch: int = 1, max_states: int = 1 << 22,
                 action_order: str = "reference", rgd_budget: Optional[int] = None):
        if heuristic not in PLAN_MODES:
            raise ValueError("heuristic must be 'RGD' or 'N+RGD'")
        if action_order not in PLAN_ACTION_ORDERS:
            raise ValueError("action_order must be 'reference' or 'fixed'")
        self.puzzle = puzzle
        self._engine = puzzle._engine()
        self.device = self._engine.device
        self.num_objects = puzzle.num_movables
        self.heuristic, self.batch, self.max_states, self.action_order = heuristic, int(batch), int(max_states), action_order
        h = ctypes.c_void_p()
        _capi.check(_capi.lib.pw_planner_create(self._engine.handle, int(getattr(puzzle, "puzzle_index", 0)),
                                                PLAN_MODES[heuristic], self.max_states, self.batch,
                                                PLAN_ACTION_ORDERS[action_order], 0 if rgd_budget is None else int(rgd_budget),
                                                ctypes.byref(h)))
        self.handle = h
        self.info: Optional[PlannerInfo] = None

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def set_sync_rounds(self, rounds: int) -> None:
        """Rounds enqueued per status read (0: the default); the result does not depend on it."""
        _capi.check(_capi.lib.pw_planner_set_sync_rounds(self.handle, int(rounds)))

    def begin(self, start: Optional[Sequence[Tuple[int, int]]] = None) -> None:
        """Starts a search from ``start`` (a reference-style state, default: the initial state)."""
        arr = None
        if start is not None:
            if len(start) != self.num_objects:
                raise ValueError("start must hold one (x, y) pair per movable")
            arr = (ctypes.c_int32 * self.num_objects)(*[int(x) * POSITION_LIMIT + int(y) for x, y in start])
        _capi.check(_capi.lib.pw_planner_begin(self.handle, arr, self._stream()))
        self.info = None

    def run(self, max_rounds: Optional[int] = None) -> PlannerInfo:
        """Runs at most ``max_rounds`` rounds (None: until the search is solved, exhausted or at its limit)."""
        info = (ctypes.c_int64 * 8)()
        rounds = 0 if max_rounds is None else int(max_rounds)
        if max_rounds is not None and rounds <= 0:
            raise ValueError("max_rounds must be positive (or None)")
        _capi.check(_capi.lib.pw_planner_run(self.handle, rounds, info, self._stream()))
        self.info = PlannerInfo(int(v) for v in info)
        return self.info

    def max_key(self) -> float:
        """The largest finite key pushed since ``begin``."""
        v = ctypes.c_float()
        _capi.check(_capi.lib.pw_planner_max_key(self.handle, ctypes.byref(v), self._stream()))
        return float(v.value)

    def plan(self) -> Optional[List[int]]:
        """The plan (list of actions 0..3) when the search is solved, else None."""
        if self.info is None or self.info.status != "solved":
            return None
        cap = 4096
        while True:
            buf = (ctypes.c_uint8 * cap)()
            n = _capi.check(_capi.lib.pw_planner_plan(self.handle, buf, cap, self._stream()))
            if n <= cap:
                return list(buf[:n])
            cap = n

    def close(self) -> None:
        h = getattr(self, "handle", None)
        if h and _capi.lib is not None:
            _capi.lib.pw_planner_destroy(h)
            self.handle = None

    __del__ = close


def solve(puzzle: PushWorldPuzzle, mode: str = "N+RGD", batch: int = 1, max_states: int = 1 << 24,
          action_order: str = "reference") -> Optional[List[int]]:
    """``run_planner``'s ``solve()``: the plan found by best-first search with ``mode`` ("RGD" or "N+RGD"), or None when
    there is none.  Raises ``RuntimeError`` when ``max_states`` runs out first."""
    bfs = BestFirstSearch(puzzle, heuristic=mode, batch=batch, max_states=max_states, action_order=action_order)
    try:
        bfs.begin()
        info = bfs.run()
        if info.status == "limit":
            raise RuntimeError(f"best-first search stopped at max_states = {max_states} without an answer")
        return bfs.plan()
    finally:
        bfs.close()


PLAN_TIMEOUT, PLAN_RANGE = 4, 5
PLAN_STATUS.update({PLAN_TIMEOUT: "timeout", PLAN_RANGE: "range"})
PLAN_BATCH_INFO = 9  # PW_PLAN_BATCH_INFO: the eight PlannerInfo values, then the search time on the device in nanoseconds


class PlanBatch:
    """Best-first search (``BestFirstSearch``'s semantics) of MANY puzzles in ONE launch (``pw_plan_batch_*``): persistent
    workgroups of one wavefront run each puzzle's whole search inside the kernel.  Item i's ``PlannerInfo`` and plan equal
    ``BestFirstSearch(puzzles[i], heuristic, batch, max_states, action_order, rgd_budget)`` + ``begin()`` + ``run(max_rounds)``
    as long as no finite RGD cost reaches ``cost_range``; two statuses are new: ``timeout`` (past ``time_limit``) and
    ``range`` (a cost at or above ``cost_range``).

    Args:
        puzzles: ``PushWorldPuzzle`` objects (each in its own object order), all on one device.
        batch: K, states popped per round (1 .. 64).
        max_states: states per puzzle; every workgroup owns a slab of that many (see ``pw_plan_batch_create``).
        cost_range: finite costs with a bucket (None: 65536).
    """

    def __init__(self, puzzles: Sequence[PushWorldPuzzle], heuristic: str = "N+RGD", batch: int = 1,
                 max_states: int = 1 << 20, action_order: str = "reference", rgd_budget: Optional[int] = None,
                 cost_range: Optional[int] = None):
        if heuristic not in PLAN_MODES:
            raise ValueError("heuristic must be 'RGD' or 'N+RGD'")
        if action_order not in PLAN_ACTION_ORDERS:
            raise ValueError("action_order must be 'reference' or 'fixed'")
        self.puzzles = list(puzzles)
        if not self.puzzles:
            raise ValueError("puzzles must not be empty")
        from .puzzle import default_device_index

        dev = default_device_index()
        self._pset = _capi.PuzzleSet([p._parsed for p in self.puzzles], dev)
        self._engine = _capi.Engine(self._pset, None, 3, 1, _capi.OBS_U8)
        self.device = self._engine.device
        self.n = len(self.puzzles)
        self.heuristic, self.batch, self.max_states, self.action_order = heuristic, int(batch), int(max_states), action_order
        h = ctypes.c_void_p()
        _capi.check(_capi.lib.pw_plan_batch_create(self._engine.handle, None, self.n, PLAN_MODES[heuristic], self.max_states,
                                                   self.batch, PLAN_ACTION_ORDERS[action_order],
                                                   0 if rgd_budget is None else int(rgd_budget),
                                                   0 if cost_range is None else int(cost_range), ctypes.byref(h)))
        self.handle = h
        self._out = None

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def run(self, max_rounds: Optional[int] = None, time_limit: Optional[float] = None, plan_cap: int = 4096) -> None:
        """Starts the searches (one launch on the current stream; returns at once).  ``max_rounds`` per puzzle (None: no
        limit), ``time_limit`` seconds per puzzle on the device's clock (None: none); ``results`` waits for them."""
        if max_rounds is not None and int(max_rounds) <= 0:
            raise ValueError("max_rounds must be positive (or None)")
        if time_limit is not None and not float(time_limit) > 0:
            raise ValueError("time_limit must be positive seconds (or None)")
        if int(plan_cap) < 1:
            raise ValueError("plan_cap must be >= 1")
        info = torch.empty((self.n, PLAN_BATCH_INFO), dtype=torch.int64, device=self.device)
        plans = torch.empty((self.n, int(plan_cap)), dtype=torch.uint8, device=self.device)
        plan_len = torch.empty((self.n,), dtype=torch.int32, device=self.device)
        _capi.check(_capi.lib.pw_plan_batch_run(self.handle, 0 if max_rounds is None else int(max_rounds),
                                                0.0 if time_limit is None else float(time_limit), _capi._ptr(info),
                                                _capi._ptr(plans), _capi._ptr(plan_len), int(plan_cap), self._stream()))
        self._out = (info, plans, plan_len)

    def cancel(self) -> None:
        """Stops the searches of every ``run`` so far soon (their status stays ``running``)."""
        _capi.check(_capi.lib.pw_plan_batch_cancel(self.handle))

    def results(self) -> List[Tuple[Optional[List[int]], PlannerInfo, float]]:
        """``(plan or None, PlannerInfo, device seconds)`` per puzzle of the last ``run`` (waits for it).  A plan longer than
        ``plan_cap`` is None."""
        if self._out is None:
            raise RuntimeError("run() has not been called")
        info, plans, plan_len = (t.cpu().numpy() for t in self._out)
        out = []
        for i in range(self.n):
            pi = PlannerInfo(int(v) for v in info[i, :8])
            n = int(plan_len[i])
            plan = plans[i, :n].tolist() if pi.status == "solved" and 0 <= n <= plans.shape[1] else None
            out.append((plan, pi, float(info[i, 8]) * 1e-9))
        return out

    def validate(self) -> torch.Tensor:
        """int8 [n] on the device: the ``is_valid_plan`` verdict (``REPLAY_VERDICT``) of every plan of the last ``run``, from
        one replay launch on the current stream (``replay_plans``; no wait).  Items without a plan are ``REPLAY_NONE``, plans
        cut at ``plan_cap`` ``REPLAY_CUT``."""
        if self._out is None:
            raise RuntimeError("run() has not been called")
        _, plans, plan_len = self._out
        ids = torch.arange(self.n, dtype=torch.int32, device=self.device)
        return replay_plans(self._engine, ids, plans, plan_len, rows=False).verdict

    def close(self) -> None:
        h = getattr(self, "handle", None)
        if h and _capi.lib is not None:
            try:  # (a launch in flight still uses the slabs)
                torch.cuda.current_stream(self.device).synchronize()
            except Exception:
                pass
            _capi.lib.pw_plan_batch_destroy(h)
            self.handle = None

    __del__ = close


def solve_many(puzzles: Sequence[PushWorldPuzzle], mode: str = "N+RGD", batch: int = 1, max_states: int = 1 << 20,
               action_order: str = "reference", time_limit: Optional[float] = None, rgd_budget: Optional[int] = None,
               cost_range: Optional[int] = None) -> List[Tuple[Optional[List[int]], PlannerInfo, float]]:
    """``solve`` for many puzzles in one launch (``PlanBatch``): ``(plan or None, PlannerInfo, device seconds)`` per puzzle.
    Unlike ``solve`` nothing is raised for a puzzle that ends at ``max_states``, ``time_limit`` or ``cost_range``: its
    ``PlannerInfo.status`` says so."""
    pb = PlanBatch(puzzles, heuristic=mode, batch=batch, max_states=max_states, action_order=action_order,
                   rgd_budget=rgd_budget, cost_range=cost_range)
    try:
        pb.run(time_limit=time_limit)
        return pb.results()
    finally:
        pb.close()


PLAN_SKIPPED = 6
PLAN_STATUS[PLAN_SKIPPED] = "skipped"


def _state_inputs(puzzle_id, pos, mask, npad: int, device) -> int:
    """The checks of ``StatePlanner.plan`` on its device arrays; returns n."""
    if not isinstance(puzzle_id, torch.Tensor) or puzzle_id.dtype != torch.int32 or puzzle_id.dim() != 1:
        raise ValueError("puzzle_id must be an int32 tensor [n]")
    n = int(puzzle_id.shape[0])
    if n < 1 or n >= 1 << 31:
        raise ValueError("puzzle_id must hold 1 .. 2^31 - 1 items")
    if not isinstance(pos, torch.Tensor) or pos.dtype != torch.int8 or tuple(pos.shape) != (n, npad, 2):
        raise ValueError(f"pos must be an int8 tensor [n, {npad}, 2] (the engine's state layout)")
    if mask is not None and (not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.uint8, torch.bool)
                             or tuple(mask.shape) != (n,)):
        raise ValueError("mask must be a uint8 or bool tensor [n] (or None)")
    for name, t in (("puzzle_id", puzzle_id), ("pos", pos), ("mask", mask)):
        if t is None:
            continue
        if t.device != device:
            raise ValueError(f"{name} must live on {device}")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
    return n


class StatePlanner:
    """Best-first search (``BestFirstSearch``'s semantics) from given states of a puzzle set, MANY in ONE launch
    (``pw_plan_batch_run_states``): typically the live states of a ``VecPushWorld``.  Item i's ``PlannerInfo`` and plan equal
    ``BestFirstSearch(puzzle puzzle_id[i], heuristic, batch, max_states, action_order, rgd_budget)`` + ``begin(start=pos[i])``
    + ``run(max_rounds)`` as long as no finite RGD cost reaches ``cost_range``.  Items that are masked out, name a puzzle
    outside ``puzzles`` or hold a movable outside its grid are ``skipped``.

    Args:
        source: a ``VecPushWorld`` or an ``_capi.Engine``: the planner uses its puzzle set (object order, ``NP``).
        puzzles: the set indices to prepare (None: every puzzle of the set).  Construction builds one RGD table set per
            puzzle -- for a pool of 14 000 puzzles that is 14 000 builds and their device memory; list the ones you plan on.
        batch: K, states popped per round (1 .. 64).
        max_states: states per item; every workgroup owns a slab of that many (see ``pw_plan_batch_create``).
        cost_range: finite costs with a bucket (None: 65536).
    """

    def __init__(self, source, puzzles: Optional[Sequence[int]] = None, heuristic: str = "N+RGD", batch: int = 1,
                 max_states: int = 1 << 16, action_order: str = "reference", rgd_budget: Optional[int] = None,
                 cost_range: Optional[int] = None):
        if heuristic not in PLAN_MODES:
            raise ValueError("heuristic must be 'RGD' or 'N+RGD'")
        if action_order not in PLAN_ACTION_ORDERS:
            raise ValueError("action_order must be 'reference' or 'fixed'")
        engine = source if isinstance(source, _capi.Engine) else getattr(source, "engine", None)
        if not isinstance(engine, _capi.Engine):
            raise ValueError("source must be a VecPushWorld or an _capi.Engine")
        self.engine = engine
        self.device = engine.device
        self.npad = int(engine.np)
        count = len(engine.pset)
        self.puzzles = list(range(count)) if puzzles is None else [int(p) for p in puzzles]
        if not self.puzzles:
            raise ValueError("puzzles must not be empty")
        if min(self.puzzles) < 0 or max(self.puzzles) >= count:
            raise ValueError(f"puzzles must be indices into the set (0 .. {count - 1})")
        self.heuristic, self.batch, self.max_states, self.action_order = heuristic, int(batch), int(max_states), action_order
        ids = (ctypes.c_int32 * len(self.puzzles))(*self.puzzles)
        h = ctypes.c_void_p()
        _capi.check(_capi.lib.pw_plan_batch_create(engine.handle, ids, len(self.puzzles), PLAN_MODES[heuristic],
                                                   self.max_states, self.batch, PLAN_ACTION_ORDERS[action_order],
                                                   0 if rgd_budget is None else int(rgd_budget),
                                                   0 if cost_range is None else int(cost_range), ctypes.byref(h)))
        self.handle = h
        self._out = None

    def plan(self, puzzle_id: torch.Tensor, pos: torch.Tensor, mask: Optional[torch.Tensor] = None,
             max_rounds: Optional[int] = None, time_limit: Optional[float] = None, plan_cap: int = 1024):
        """Starts the searches from ``pos`` (int8 [n, NP, 2], the engine's layout) of puzzles ``puzzle_id`` (int32 [n]), both
        on the device, on the current stream; does not wait.  ``mask`` (uint8 / bool [n]): 0 skips an item.  ``max_rounds``
        per item (None: no limit), ``time_limit`` seconds per item on the device's clock (None: none).

        Returns device tensors ``(info int64 [n, 9], plans uint8 [n, plan_cap], plan_len int32 [n], first_action int8 [n])``:
        ``info`` as ``PlanBatch`` (the eight ``PlannerInfo`` values, then device nanoseconds); ``plan_len`` -1 without a
        plan (a plan longer than ``plan_cap`` is cut); ``first_action`` the plan's first action, -1 without a non-empty
        plan.  ``plan_cap`` 0: no plans are written."""
        n = _state_inputs(puzzle_id, pos, mask, self.npad, self.device)
        if max_rounds is not None and int(max_rounds) <= 0:
            raise ValueError("max_rounds must be positive (or None)")
        if time_limit is not None and not float(time_limit) > 0:
            raise ValueError("time_limit must be positive seconds (or None)")
        if int(plan_cap) < 0:
            raise ValueError("plan_cap must be >= 0")
        info = torch.empty((n, PLAN_BATCH_INFO), dtype=torch.int64, device=self.device)
        plans = torch.empty((n, int(plan_cap)), dtype=torch.uint8, device=self.device)
        plan_len = torch.empty((n,), dtype=torch.int32, device=self.device)
        first_action = torch.empty((n,), dtype=torch.int8, device=self.device)
        stream = ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        _capi.check(_capi.lib.pw_plan_batch_run_states(
            self.handle, _capi._ptr(puzzle_id), _capi._ptr(pos), self.npad, _capi._ptr(mask), n,
            0 if max_rounds is None else int(max_rounds), 0.0 if time_limit is None else float(time_limit), _capi._ptr(info),
            _capi._ptr(plans) if int(plan_cap) > 0 else None, _capi._ptr(plan_len), int(plan_cap), _capi._ptr(first_action),
            stream))
        # (the inputs stay referenced until the results are read: the launch reads them on the device)
        self._out = (info, plans, plan_len, first_action, puzzle_id, pos, mask)
        return info, plans, plan_len, first_action

    def results(self) -> List[Tuple[Optional[List[int]], PlannerInfo, float]]:
        """``(plan or None, PlannerInfo, device seconds)`` per item of the last ``plan`` (waits for it), as
        ``PlanBatch.results``.  A plan longer than ``plan_cap`` (or any plan with ``plan_cap`` 0) is None."""
        if self._out is None:
            raise RuntimeError("plan() has not been called")
        info, plans, plan_len = (t.cpu().numpy() for t in self._out[:3])
        out = []
        for i in range(info.shape[0]):
            pi = PlannerInfo(int(v) for v in info[i, :8])
            n = int(plan_len[i])
            plan = plans[i, :n].tolist() if pi.status == "solved" and 0 <= n <= plans.shape[1] else None
            out.append((plan, pi, float(info[i, 8]) * 1e-9))
        return out

    def validate(self) -> torch.Tensor:
        """int8 [n] on the device: the ``is_valid_plan`` verdict (``REPLAY_VERDICT``) of every plan of the last ``plan``
        call, taken from that call's start states, from one replay launch on the current stream (``replay_plans``; no
        wait)."""
        if self._out is None:
            raise RuntimeError("plan() has not been called")
        _, plans, plan_len, _, puzzle_id, pos, mask = self._out
        if plans.shape[1] < 1:
            raise ValueError("the last plan() call kept no plans (plan_cap 0)")
        return replay_plans(self.engine, puzzle_id, plans, plan_len, pos=pos, mask=mask, rows=False).verdict

    def cancel(self) -> None:
        """Stops the searches of every ``plan`` so far soon (their status stays ``running``)."""
        _capi.check(_capi.lib.pw_plan_batch_cancel(self.handle))

    def close(self) -> None:
        h = getattr(self, "handle", None)
        if h and _capi.lib is not None:
            try:  # (a launch in flight still uses the slabs)
                torch.cuda.synchronize(self.device)
            except Exception:
                pass
            _capi.lib.pw_plan_batch_destroy(h)
            self.handle = None

    __del__ = close


# ---- exact cost-to-go tables (pw_search_solve / pw_search_table_query) ------------------------------------------
COST_DEAD_END, COST_UNKNOWN = -1, -2  # ``SolutionTable.query``'s cost of a dead end / of a state that is not in the table
TABLE_DEAD_END = 0xFFFF               # the same in the table's own uint16 costs


def _query_outputs(out, n: int, device):
    """The ``(index, cost, acts)`` triple a table query fills: fresh (-1 / ``COST_UNKNOWN`` / 0) or the checked ``out``."""
    if out is None:
        return (torch.full((n,), -1, dtype=torch.int32, device=device),
                torch.full((n,), COST_UNKNOWN, dtype=torch.int32, device=device),
                torch.zeros((n,), dtype=torch.uint8, device=device))
    if not isinstance(out, (tuple, list)) or len(out) != 3:
        raise ValueError("out must be the (index, cost, acts) triple of an earlier query")
    for name, t, dtype in (("index", out[0], torch.int32), ("cost", out[1], torch.int32), ("acts", out[2], torch.uint8)):
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != (n,) or t.device != device \
                or not t.is_contiguous():
            raise ValueError(f"out: {name} must be a contiguous {dtype} tensor [n] on {device}")
    return tuple(out)


# ---- drawing from the tables (pw_*_index / pw_*_sample / pw_*_plans) --------------------------------------------
TABLE_K_SAMPLE, TABLE_K_PLAN = 0xA0761D6478BD642F, 0xE7037ED1A0B428DB  # PW_TABLE_K_SAMPLE / PW_TABLE_K_PLAN
TABLE_TIES = {"lowest": 0, "uniform": 1}
PLANS_NONE, PLANS_CUT = -1, -2  # ``plans``' plan_len: no plan from there (dead end, not in a table) / longer than plan_cap
_COST_MAX = (1 << 31) - 1


def _dev_tensor(name: str, t, dtype, shape, device, optional: bool = False):
    """One device array of a table call: dtype, shape, device and contiguity, in the words of ``_state_inputs``."""
    if t is None and optional:
        return None
    dtypes = dtype if isinstance(dtype, tuple) else (dtype,)
    if not isinstance(t, torch.Tensor) or t.dtype not in dtypes or tuple(t.shape) != tuple(shape):
        kind = " or ".join(str(d).replace("torch.", "") for d in dtypes)
        raise ValueError(f"{name} must be a {kind} tensor {list(shape)}" + (" (or None)" if optional else ""))
    if t.device != device:
        raise ValueError(f"{name} must live on {device}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return t


def _pos_inputs(puzzle_id, pos, mask, npad: int, device, ids_optional: bool) -> int:
    """``_state_inputs``, with ``puzzle_id`` None allowed for the one-puzzle tables; returns n."""
    if puzzle_id is not None or not ids_optional:
        return _state_inputs(puzzle_id, pos, mask, npad, device)
    if not isinstance(pos, torch.Tensor) or pos.dtype != torch.int8 or pos.dim() != 3 or \
            tuple(pos.shape[1:]) != (npad, 2) or not 1 <= pos.shape[0] < 1 << 31:
        raise ValueError(f"pos must be an int8 tensor [n, {npad}, 2] (the engine's state layout), n >= 1")
    n = int(pos.shape[0])
    _dev_tensor("pos", pos, torch.int8, (n, npad, 2), device)
    _dev_tensor("mask", mask, (torch.uint8, torch.bool), (n,), device, optional=True)
    return n


def _sample_call(table, ids_optional: bool, puzzle_id, pos, steps, terminated, truncated, cost, mask, seed, counter, out):
    """The checks and the one launch of ``SolutionTable.sample`` / ``SolutionTableBatch.sample``."""
    npad, device = table.npad, table.device
    n = _pos_inputs(puzzle_id, pos, mask, npad, device, ids_optional)
    _dev_tensor("steps", steps, torch.int32, (n,), device)
    _dev_tensor("terminated", terminated, (torch.uint8, torch.bool), (n,), device, optional=True)
    _dev_tensor("truncated", truncated, (torch.uint8, torch.bool), (n,), device, optional=True)
    if not isinstance(cost, (tuple, list)) or len(cost) != 2:
        raise ValueError("cost must be a (lo, hi) pair of ints (hi None: no upper limit) or of int32 tensors [n]")
    lo, hi = cost
    lo_n = hi_n = None
    if isinstance(lo, torch.Tensor) or isinstance(hi, torch.Tensor):
        lo_n = _dev_tensor("cost: lo", lo, torch.int32, (n,), device)
        hi_n = _dev_tensor("cost: hi", hi, torch.int32, (n,), device)
        lo = hi = 0
    else:
        lo, hi = int(lo), _COST_MAX if hi is None else int(hi)
        if not 0 <= lo <= hi <= _COST_MAX:
            raise ValueError("cost must be a band 0 <= lo <= hi")
    if counter is None:
        counter = torch.zeros((n,), dtype=torch.int32, device=device)
    # (uint32 counter bits; an int32 tensor holds them as well, like VecPushWorld.episode)
    _dev_tensor("counter", counter, (torch.int32, torch.uint32), (n,), device)
    if out is None:
        out = (torch.full((n,), -1, dtype=torch.int32, device=device), torch.full((n,), -1, dtype=torch.int32, device=device))
    if not isinstance(out, (tuple, list)) or len(out) != 2:
        raise ValueError("out must be the (row, cost) pair of an earlier sample")
    _dev_tensor("out: row", out[0], torch.int32, (n,), device)
    _dev_tensor("out: cost", out[1], torch.int32, (n,), device)
    fn, handle, stream = table._entry("sample")  # (the first call builds the cost index: not capturable)
    _capi.check(fn(handle, _capi._ptr(puzzle_id), _capi._ptr(mask), n, npad, int(seed) & 0xFFFFFFFFFFFFFFFF, _capi._ptr(counter),
                   lo, hi, _capi._ptr(lo_n), _capi._ptr(hi_n), _capi._ptr(pos), _capi._ptr(steps), _capi._ptr(terminated),
                   _capi._ptr(truncated), _capi._ptr(out[0]), _capi._ptr(out[1]), stream))
    return tuple(out)


def _plans_call(table, ids_optional: bool, index, puzzle_id, mask, tie, seed, plan_cap, out):
    """The checks and the one launch of ``SolutionTable.plans`` / ``SolutionTableBatch.plans``."""
    device = table.device
    if not isinstance(index, torch.Tensor) or index.dtype != torch.int32 or index.dim() != 1:
        raise ValueError("index must be an int32 tensor [n] (rows, as query returns them)")
    n = int(index.shape[0])
    if n < 1 or n >= 1 << 31:
        raise ValueError("index must hold 1 .. 2^31 - 1 items")
    _dev_tensor("index", index, torch.int32, (n,), device)
    _dev_tensor("puzzle_id", puzzle_id, torch.int32, (n,), device, optional=ids_optional)
    _dev_tensor("mask", mask, (torch.uint8, torch.bool), (n,), device, optional=True)
    if tie not in TABLE_TIES:
        raise ValueError("tie must be 'lowest' or 'uniform'")
    plan_cap = int(plan_cap)
    if not 1 <= plan_cap <= _capi.PLAN_MAX_ACTIONS:
        raise ValueError(f"plan_cap must be in 1 .. {_capi.PLAN_MAX_ACTIONS}")
    if out is None:
        out = (torch.zeros((n, plan_cap), dtype=torch.uint8, device=device),
               torch.full((n,), PLANS_NONE, dtype=torch.int32, device=device))
    if not isinstance(out, (tuple, list)) or len(out) != 2:
        raise ValueError("out must be the (plans, plan_len) pair of an earlier call")
    _dev_tensor("out: plans", out[0], torch.uint8, (n, plan_cap), device)
    _dev_tensor("out: plan_len", out[1], torch.int32, (n,), device)
    fn, handle, stream = table._entry("plans")
    _capi.check(fn(handle, _capi._ptr(index), _capi._ptr(puzzle_id), _capi._ptr(mask), n, TABLE_TIES[tie],
                   int(seed) & 0xFFFFFFFFFFFFFFFF, _capi._ptr(out[0]), plan_cap, _capi._ptr(out[1]), stream))
    return tuple(out)


_SAMPLE_DOC = """Draws one start state per environment from this table's states with a cost-to-go in ``cost`` -- ``(lo, hi)`` ints
        (``hi`` None: up to the table's ``max_cost``) or two int32 tensors [n], a band per environment -- uniformly over those
        states, and writes it as a reset would: the state into ``pos`` (int8 [n, NP, 2], zeros beyond the puzzle's movables),
        ``steps`` = 0, ``terminated`` = ``truncated`` = 0 (either may be None).  One launch on the current stream, no wait, no
        allocation when ``counter`` and ``out`` are given (capturable).  The band is clamped to ``0 .. max_cost``; dead ends are
        never drawn.  ``counter`` (int32 / uint32 [n], None: zeros) counts the draws of every environment and is advanced in
        place: draw = f(``seed``, environment, counter).  Returns ``(row, cost)`` int32 [n] (``out``, filled in place): the
        row drawn and its cost; -1 / -1 where the puzzle has no solvable state.  Masked environments and environments of
        puzzles without a stored table here keep everything they held, the counter included."""

_PLANS_DOC = """A shortest plan from every row of ``index`` (int32 [n], as ``query`` returns them) in one launch on the current
        stream, no wait: ``(plans uint8 [n, plan_cap], plan_len int32 [n])``.  ``tie`` "lowest" takes the lowest optimal
        action at every step (``optimal_plan``'s plan), "uniform" draws among the optimal actions (f(``seed``, item, step)).
        ``plan_len`` is the row's cost; ``PLANS_NONE`` -1 for ``index`` < 0, a dead end or a puzzle without a stored table
        here, ``PLANS_CUT`` -2 for a plan longer than ``plan_cap`` (``plans`` untouched in both cases).  Masked items keep
        what ``out`` -- the pair of an earlier call -- held."""


class SolutionTable:
    """The exact cost-to-go of EVERY state reachable in one puzzle: a ``BreadthFirstSearch`` run to exhaustion, then
    ``pw_search_solve``'s backward propagation from the goal states.  Row i belongs to state i of the search (the FIFO
    numbering of ``states()``):

    * ``successors()`` int32 [count, 4]: the index of the state each action (L, R, U, D) leads to, i itself where nothing moves;
    * ``costs()`` uint16 [count]: the length of a shortest plan from the state, 0 at goal states, 0xFFFF at dead ends --
      states from which no goal state can be reached any more (PushWorld is irreversible);
    * ``actions()`` uint8 [count]: bit a = action a is optimal (it moves and its successor costs one less; none at goal
      states and dead ends), bit 4 + a = action a is safe (its successor is no dead end).

    Args:
        puzzle: a ``PushWorldPuzzle`` or a ``SetPuzzle``.
        max_states: capacity of the search; ``ValueError`` ("the state store is full") when the space is larger.
        start: the state the space is explored from (default: the initial state).
        chunk: parents per pass, as ``BreadthFirstSearch``.

    Device memory: the search's, plus 19 bytes per state found.
    """

    def __init__(self, puzzle, max_states: int = 1 << 22, start: Optional[Sequence[Tuple[int, int]]] = None,
                 chunk: Optional[int] = None):
        self.puzzle = puzzle
        self.puzzle_index = int(getattr(puzzle, "puzzle_index", 0))
        self.search = BreadthFirstSearch(puzzle, max_states=max_states, chunk=chunk)
        self.device = self.search.device
        self.npad = int(self.search._engine.np)
        self._host = None  # (acts, succ, cost) on the host, fetched by the first optimal_plan
        try:
            self.search.begin(start)
            while not self.search.exhausted:
                self.search.expand()
            info = (ctypes.c_int64 * 4)()
            _capi.check(_capi.lib.pw_search_solve(self.search.handle, info, self.search._stream()))
            self.num_states, self.num_goal_states, self.num_dead_ends, self.max_cost = (int(v) for v in info)
            st = (ctypes.c_double * 5)()
            _capi.check(_capi.lib.pw_search_solve_stats(self.search.handle, st))
            self.solve_ms = tuple(float(v) for v in st[:3])  # device ms: successor pass, backward sweeps, action bits
            self.solve_passes, self.solve_lane_passes = int(st[3]), int(st[4])  # successor passes / one lane per parent
            c0 = int(self.costs(0, 1).cpu().numpy()[0])
            self.initial_cost = None if c0 == TABLE_DEAD_END else c0
        except Exception:
            self.search.close()
            raise

    def _read(self, which: int, first: int, count: Optional[int]) -> torch.Tensor:
        count = self.num_states - first if count is None else count
        shape, dtype = (((count, 4), torch.int32), ((count,), torch.uint16), ((count,), torch.uint8))[which]
        out = torch.empty(shape if count >= 0 else (0,), dtype=dtype, device=self.device)
        ptrs = [None, None, None]
        ptrs[which] = _capi._ptr(out)
        _capi.check(_capi.lib.pw_search_table_read(self.search.handle, int(first), int(count), *ptrs, self.search._stream()))
        return out

    def successors(self, first: int = 0, count: Optional[int] = None) -> torch.Tensor:
        """int32 [count, 4] on the device: successor indices of states ``first .. first + count - 1``."""
        return self._read(0, first, count)

    def costs(self, first: int = 0, count: Optional[int] = None) -> torch.Tensor:
        """uint16 [count] on the device: cost-to-go, 0xFFFF = dead end."""
        return self._read(1, first, count)

    def actions(self, first: int = 0, count: Optional[int] = None) -> torch.Tensor:
        """uint8 [count] on the device: optimal (bits 0..3) and safe (bits 4..7) actions."""
        return self._read(2, first, count)

    def states(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """``BreadthFirstSearch.states``: int array [count, N, 2] of (x, y) positions."""
        return self.search.states(first, count)

    def plan(self, index: int) -> List[int]:
        """``BreadthFirstSearch.plan``: actions from the start state to state ``index``."""
        return self.search.plan(index)

    def optimal_plan(self, index: int = 0) -> Optional[List[int]]:
        """A shortest plan from state ``index`` to a goal state (at every step the lowest optimal action), [] at a goal
        state, None for a dead end."""
        if not 0 <= int(index) < self.num_states:
            raise ValueError("state index out of bounds")
        if self._host is None:
            self._host = (self.actions().cpu().numpy(), self.successors().cpu().numpy(), self.costs().cpu().numpy())
        acts, succ, cost = self._host
        i = int(index)
        if cost[i] == TABLE_DEAD_END:
            return None
        plan = []
        while cost[i] != 0:
            a = int(acts[i] & 15)
            a = (a & -a).bit_length() - 1
            plan.append(a)
            i = int(succ[i, a])
        return plan

    def query(self, puzzle_id: Optional[torch.Tensor], pos: torch.Tensor, mask: Optional[torch.Tensor] = None, out=None):
        """Looks states up on the device, one launch on the current stream, no wait: ``pos`` int8 [n, NP, 2] (the engine's
        layout, e.g. ``VecPushWorld.pos``), ``puzzle_id`` int32 [n] (None: every item is this table's puzzle), ``mask`` uint8 /
        bool [n] (0 skips an item).  Returns device tensors ``(index int32 [n], cost int32 [n], acts uint8 [n])``: the row of
        each state, its cost (``COST_DEAD_END`` -1 for a dead end) and its action bits; a state that is not in the table
        (not reachable from the start, or outside the grid) gives -1 / ``COST_UNKNOWN`` -2 / 0.  Items of other puzzles and
        masked items keep what ``out`` -- the triple of an earlier call, filled in place -- held; without ``out`` they are
        -1 / -2 / 0 too."""
        if puzzle_id is None:  # the kernel takes NULL: no id array is made up
            if not isinstance(pos, torch.Tensor) or pos.dtype != torch.int8 or pos.dim() != 3 or \
                    tuple(pos.shape[1:]) != (self.npad, 2) or not 1 <= pos.shape[0] < 1 << 31:
                raise ValueError(f"pos must be an int8 tensor [n, {self.npad}, 2] (the engine's state layout), n >= 1")
            n = int(pos.shape[0])
            if mask is not None and (not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.uint8, torch.bool)
                                     or tuple(mask.shape) != (n,)):
                raise ValueError("mask must be a uint8 or bool tensor [n] (or None)")
            for name, t in (("pos", pos), ("mask", mask)):
                if t is not None and t.device != self.device:
                    raise ValueError(f"{name} must live on {self.device}")
                if t is not None and not t.is_contiguous():
                    raise ValueError(f"{name} must be contiguous")
        else:
            n = _state_inputs(puzzle_id, pos, mask, self.npad, self.device)
        out = _query_outputs(out, n, self.device)
        _capi.check(_capi.lib.pw_search_table_query(self.search.handle, _capi._ptr(puzzle_id), _capi._ptr(pos), self.npad,
                                                    _capi._ptr(mask), n, _capi._ptr(out[0]), _capi._ptr(out[1]),
                                                    _capi._ptr(out[2]), self.search._stream()))
        return out

    def _entry(self, what: str):
        """(function, handle, stream) of the sample / plans launch; the first sample builds the cost index."""
        if what == "sample" and not getattr(self, "_indexed", False):
            _capi.check(_capi.lib.pw_search_table_index(self.search.handle, self.search._stream()))
            self._indexed = True
        fn = _capi.lib.pw_search_table_sample if what == "sample" else _capi.lib.pw_search_table_plans
        return fn, self.search.handle, self.search._stream()

    def cost_index(self):
        """``(rows_by_cost int32 [count], cost_start uint32 [max_cost + 3])`` on the device: the rows grouped by cost-to-go,
        the dead ends last; bucket c is ``rows_by_cost[cost_start[c] : cost_start[c + 1]]``, the dead ends are bucket
        ``max_cost + 1``.  Built by the first call (three launches), kept until the search is restarted.  The order inside
        a bucket is whatever the build left."""
        _capi.check(_capi.lib.pw_search_table_index(self.search.handle, self.search._stream()))
        rows = torch.empty((self.num_states,), dtype=torch.int32, device=self.device)
        start = torch.empty((self.max_cost + 3,), dtype=torch.uint32, device=self.device)
        _capi.check(_capi.lib.pw_search_table_index_read(self.search.handle, _capi._ptr(rows), _capi._ptr(start),
                                                         self.search._stream()))
        return rows, start

    def sample(self, puzzle_id: Optional[torch.Tensor], pos: torch.Tensor, steps: torch.Tensor,
               terminated: Optional[torch.Tensor] = None, truncated: Optional[torch.Tensor] = None, cost=(1, None),
               mask: Optional[torch.Tensor] = None, seed: int = 0, counter: Optional[torch.Tensor] = None, out=None):
        return _sample_call(self, True, puzzle_id, pos, steps, terminated, truncated, cost, mask, seed, counter, out)

    sample.__doc__ = _SAMPLE_DOC

    def plans(self, index: torch.Tensor, puzzle_id: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None,
              tie: str = "lowest", seed: int = 0, plan_cap: int = 1024, out=None):
        return _plans_call(self, True, index, puzzle_id, mask, tie, seed, plan_cap, out)

    plans.__doc__ = _PLANS_DOC

    def covers(self, puzzle_id: torch.Tensor) -> torch.Tensor:
        """bool [n] on the device: the items of ``puzzle_id`` this table answers for."""
        return puzzle_id == self.puzzle_index

    def close(self) -> None:
        search = getattr(self, "search", None)
        if search is not None:
            search.close()

    __del__ = close


# ---- cost-to-go tables of many small puzzles in one launch (pw_solve_batch_*) -----------------------------------
TABLE_BUILT, TABLE_TOO_MANY, TABLE_NOT_SEARCHED, TABLE_SUMMARY_ONLY, TABLE_COST_RANGE, TABLE_INTERNAL = 0, 2, 3, 4, 5, 6


class SolutionTableBatch:
    """``SolutionTable``'s rows for MANY small puzzles of one set, built by ONE launch (``pw_solve_batch_run``: persistent
    workgroups, the breadth-first search, the successor pass and the backward sweeps of a puzzle inside the kernel) and
    queried for a mixed batch by one launch.  The kernel's limits are ``search_batch``'s: 16 x 16 cells with the border,
    8 movables; bigger puzzles (status 3) and bigger spaces (status 2) are ``SolutionTable``'s.

    Args:
        source: a ``VecPushWorld`` or an ``_capi.Engine``: the tables are of its puzzle set, in its object order.
        puzzles: set indices (item i is puzzle ``puzzles[i]``); None: every puzzle of the set.
        max_states_each: state cap per puzzle.
        rows: rows of the pool that holds the tables of all items together.  None: one summary-only pass sizes it, a
            second pass stores (nothing is left out); 0: summaries only.

    Device tensors, one entry per item: ``status`` uint8 (0 table stored, 2 more than ``max_states_each`` states, 3 not
    searched, 4 built but the pool was full -- summary only, 5 a cost beyond 65 534, 6 internal error), ``num_states``,
    ``num_goals``, ``dead_ends``, ``max_cost``, ``start_cost`` int32 (valid for status 0 and 4; ``start_cost`` -1: the start
    state is a dead end), ``row_offset`` int64 (-1: not stored).  ``rows_needed``: the pool that stores every built table.

    Row numbers inside one breadth-first layer, and which pool offset an item gets, depend on the schedule of the launch;
    row 0 is the start state, and everything is found by state (``states(i)`` / ``query``), never by a number across runs.
    Device memory: at most 43 bytes per row of the pool, see ``pw_solve_batch_create``.
    """

    def __init__(self, source, puzzles: Optional[Sequence[int]] = None, max_states_each: int = 1 << 16,
                 rows: Optional[int] = None):
        engine = source if isinstance(source, _capi.Engine) else getattr(source, "engine", None)
        if not isinstance(engine, _capi.Engine):
            raise ValueError("source must be a VecPushWorld or an _capi.Engine")
        self.engine, self.device, self.npad = engine, engine.device, int(engine.np)
        count = len(engine.pset)
        self.puzzles = list(range(count)) if puzzles is None else [int(p) for p in puzzles]
        if not self.puzzles:
            raise ValueError("puzzles must not be empty")
        if min(self.puzzles) < 0 or max(self.puzzles) >= count:
            raise ValueError(f"puzzles must be indices into the set (0 .. {count - 1})")
        if rows is not None and int(rows) < 0:
            raise ValueError("rows must be >= 0 (or None)")
        self.max_states_each = int(max_states_each)
        self.handle = None
        self._ids = None if puzzles is None else torch.as_tensor(np.asarray(self.puzzles, dtype=np.int32)).to(self.device)
        self._host = {}  # item -> (acts, succ, cost) on the host, fetched by its first optimal_plan
        if rows is None:
            self._run(0)
            rows = self.rows_needed
            self.close()
        self._run(int(rows))

    def _stream(self):
        return self.engine._stream()

    def _run(self, rows: int) -> None:
        h = ctypes.c_void_p()
        _capi.check(_capi.lib.pw_solve_batch_create(self.engine.handle, int(rows), ctypes.byref(h)))
        self.handle = h
        n = len(self.puzzles)
        try:
            _capi.check(_capi.lib.pw_solve_batch_run(h, _capi._ptr(self._ids), n, self.max_states_each, self._stream()))
            self.status = torch.empty((n,), dtype=torch.uint8, device=self.device)
            self.summary = torch.empty((n, 5), dtype=torch.int32, device=self.device)
            self.row_offset = torch.empty((n,), dtype=torch.int64, device=self.device)
            _capi.check(_capi.lib.pw_solve_batch_copy_results(h, _capi._ptr(self.status), _capi._ptr(self.summary),
                                                              _capi._ptr(self.row_offset), self._stream()))
            totals = (ctypes.c_int64 * 3)()
            _capi.check(_capi.lib.pw_solve_batch_totals(h, totals, self._stream()))
        except Exception:
            self.close()
            raise
        self.rows, self.rows_needed = int(rows), int(totals[0])
        self.num_states, self.num_goals, self.dead_ends, self.max_cost, self.start_cost = self.summary.unbind(1)
        self._counts = None
        self._indexed, self._max_costs, self._covered = False, None, None

    def __len__(self) -> int:
        return len(self.puzzles)

    def _item(self, item: int) -> Tuple[int, int]:
        """(item, its number of states); ``ValueError`` for an item without stored rows."""
        if not 0 <= int(item) < len(self.puzzles):
            raise ValueError("item out of bounds")
        if self._counts is None:
            self._counts = (self.status.cpu().numpy(), self.summary[:, 0].cpu().numpy())
        if self._counts[0][int(item)] != TABLE_BUILT:
            raise ValueError(f"item {int(item)} has no stored table (status {int(self._counts[0][int(item)])})")
        return int(item), int(self._counts[1][int(item)])

    def _read(self, which: int, item: int) -> torch.Tensor:
        item, count = self._item(item)
        shape, dtype = (((count,), torch.int64), ((count, 4), torch.int32), ((count,), torch.uint16),
                        ((count,), torch.uint8))[which]
        out = torch.empty(shape, dtype=dtype, device=self.device)
        ptrs = [None, None, None, None]
        ptrs[which] = _capi._ptr(out)
        _capi.check(_capi.lib.pw_solve_batch_read(self.handle, item, 0, count, *ptrs, self._stream()))
        return out

    def keys(self, item: int) -> torch.Tensor:
        """int64 [count] on the device: the state word of every row (movable j at bits 8 j: x | y << 4)."""
        return self._read(0, item)

    def states(self, item: int) -> np.ndarray:
        """int array [count, N, 2] of (x, y) positions, row by row (``SolutionTable.states``)."""
        keys = self.keys(item).cpu().numpy().astype(np.uint64)
        n_mov = self.engine.pset.headers()[320 * self.puzzles[int(item)] + 6]
        shifts = (np.arange(n_mov, dtype=np.uint64) * np.uint64(8))[None, :]
        byte = (keys[:, None] >> shifts) & np.uint64(0xFF)
        return np.stack([byte & np.uint64(15), byte >> np.uint64(4)], axis=-1).astype(np.int64)

    def successors(self, item: int) -> torch.Tensor:
        """int32 [count, 4] on the device: the row each action (L, R, U, D) leads to, the row itself where nothing moves."""
        return self._read(1, item)

    def costs(self, item: int) -> torch.Tensor:
        """uint16 [count] on the device: cost-to-go, 0xFFFF = dead end."""
        return self._read(2, item)

    def actions(self, item: int) -> torch.Tensor:
        """uint8 [count] on the device: optimal (bits 0..3) and safe (bits 4..7) actions."""
        return self._read(3, item)

    def optimal_plan(self, item: int, index: int = 0) -> Optional[List[int]]:
        """A shortest plan from row ``index`` of item ``item`` (row 0: the initial state) to a goal state, at every step the
        lowest optimal action; [] at a goal state, None for a dead end."""
        item, count = self._item(item)
        if not 0 <= int(index) < count:
            raise ValueError("state index out of bounds")
        if item not in self._host:
            self._host[item] = (self.actions(item).cpu().numpy(), self.successors(item).cpu().numpy(),
                                self.costs(item).cpu().numpy())
        acts, succ, cost = self._host[item]
        i = int(index)
        if cost[i] == TABLE_DEAD_END:
            return None
        plan = []
        while cost[i] != 0:
            a = int(acts[i] & 15)
            a = (a & -a).bit_length() - 1
            plan.append(a)
            i = int(succ[i, a])
        return plan

    def query(self, puzzle_id: torch.Tensor, pos: torch.Tensor, mask: Optional[torch.Tensor] = None, out=None):
        """``SolutionTable.query`` for a mixed batch, one launch on the current stream, no wait: ``puzzle_id`` int32 [n],
        ``pos`` int8 [n, NP, 2], ``mask`` uint8 / bool [n].  Returns ``(index, cost, acts)``; ``index`` is the row within the
        puzzle's table.  Items whose puzzle has no stored table here and masked items keep what ``out`` held."""
        n = _state_inputs(puzzle_id, pos, mask, self.npad, self.device)
        out = _query_outputs(out, n, self.device)
        _capi.check(_capi.lib.pw_solve_batch_query(self.handle, _capi._ptr(puzzle_id), _capi._ptr(pos), self.npad,
                                                   _capi._ptr(mask), n, _capi._ptr(out[0]), _capi._ptr(out[1]),
                                                   _capi._ptr(out[2]), self._stream()))
        return out

    def _index(self) -> None:
        if not self._indexed:  # (the first call builds the cost index of every stored table: not capturable)
            _capi.check(_capi.lib.pw_solve_batch_index(self.handle, self._stream()))
            self._indexed = True

    def _entry(self, what: str):
        """(function, handle, stream) of the sample / plans launch; the first sample builds the cost index."""
        if what == "sample":
            self._index()
        fn = _capi.lib.pw_solve_batch_sample if what == "sample" else _capi.lib.pw_solve_batch_plans
        return fn, self.handle, self._stream()

    def cost_index(self, item: int):
        """``SolutionTable.cost_index`` of item ``item``: ``(rows_by_cost int32 [count], cost_start uint32 [max_cost + 3])``
        on the device.  The first call builds the index of every stored table (three launches)."""
        item, count = self._item(item)
        self._index()
        if self._max_costs is None:
            self._max_costs = self.summary[:, 3].cpu().numpy()
        rows = torch.empty((count,), dtype=torch.int32, device=self.device)
        start = torch.empty((int(self._max_costs[item]) + 3,), dtype=torch.uint32, device=self.device)
        _capi.check(_capi.lib.pw_solve_batch_index_read(self.handle, item, _capi._ptr(rows), _capi._ptr(start), self._stream()))
        return rows, start

    def sample(self, puzzle_id: torch.Tensor, pos: torch.Tensor, steps: torch.Tensor,
               terminated: Optional[torch.Tensor] = None, truncated: Optional[torch.Tensor] = None, cost=(1, None),
               mask: Optional[torch.Tensor] = None, seed: int = 0, counter: Optional[torch.Tensor] = None, out=None):
        return _sample_call(self, False, puzzle_id, pos, steps, terminated, truncated, cost, mask, seed, counter, out)

    sample.__doc__ = _SAMPLE_DOC

    def plans(self, index: torch.Tensor, puzzle_id: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None,
              tie: str = "lowest", seed: int = 0, plan_cap: int = 1024, out=None):
        return _plans_call(self, False, index, puzzle_id, mask, tie, seed, plan_cap, out)

    plans.__doc__ = _PLANS_DOC

    def covers(self, puzzle_id: torch.Tensor) -> torch.Tensor:
        """bool [n] on the device: the items of ``puzzle_id`` whose puzzle has a stored table here."""
        if self._covered is None:
            has = torch.zeros((len(self.engine.pset),), dtype=torch.bool, device=self.device)
            ids = self._ids if self._ids is not None else torch.arange(len(self.puzzles), device=self.device)
            has[ids[self.status == TABLE_BUILT].long()] = True
            self._covered = has
        pid = puzzle_id.long()
        inside = (pid >= 0) & (pid < self._covered.shape[0])
        return inside & self._covered[pid.clamp(0, self._covered.shape[0] - 1)]

    def close(self) -> None:
        h = getattr(self, "handle", None)
        if h is not None and _capi.lib is not None:
            _capi.lib.pw_solve_batch_destroy(h)
        self.handle = None

    __del__ = close


# ---- plan replay (pw_plan_replay_check / pw_plan_replay_emit) ----------------------------------------------
REPLAY_VALID, REPLAY_NOT_GOAL, REPLAY_EARLY = _capi.REPLAY_VALID, _capi.REPLAY_NOT_GOAL, _capi.REPLAY_EARLY
REPLAY_NONE, REPLAY_CUT, REPLAY_SKIPPED = _capi.REPLAY_NONE, _capi.REPLAY_CUT, _capi.REPLAY_SKIPPED
REPLAY_VERDICT = {REPLAY_VALID: "valid", REPLAY_NOT_GOAL: "not_goal", REPLAY_EARLY: "early", REPLAY_NONE: "none",
                  REPLAY_CUT: "cut", REPLAY_SKIPPED: "skipped"}
REPLAY_INCLUDE = {"valid": _capi.REPLAY_INCLUDE_VALID, "replayed": _capi.REPLAY_INCLUDE_REPLAYED}


def _replay_inputs(puzzle_id, plans, plan_len, pos, mask, npad: int, device) -> int:
    """The checks of ``replay_plans`` on its device arrays; returns n."""
    if not isinstance(puzzle_id, torch.Tensor) or puzzle_id.dtype != torch.int32 or puzzle_id.dim() != 1:
        raise ValueError("puzzle_id must be an int32 tensor [n]")
    n = int(puzzle_id.shape[0])
    if n < 1 or n >= 1 << 31:
        raise ValueError("puzzle_id must hold 1 .. 2^31 - 1 items")
    if not isinstance(plans, torch.Tensor) or plans.dtype != torch.uint8 or plans.dim() != 2 or plans.shape[0] != n:
        raise ValueError("plans must be a uint8 tensor [n, plan_cap]")
    if not 1 <= int(plans.shape[1]) <= _capi.PLAN_MAX_ACTIONS:
        raise ValueError(f"plans must hold 1 .. {_capi.PLAN_MAX_ACTIONS} actions per item (plan_cap)")
    if not isinstance(plan_len, torch.Tensor) or plan_len.dtype != torch.int32 or tuple(plan_len.shape) != (n,):
        raise ValueError("plan_len must be an int32 tensor [n]")
    if pos is not None and (not isinstance(pos, torch.Tensor) or pos.dtype != torch.int8 or tuple(pos.shape) != (n, npad, 2)):
        raise ValueError(f"pos must be an int8 tensor [n, {npad}, 2] (the engine's state layout) or None")
    if mask is not None and (not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.uint8, torch.bool)
                             or tuple(mask.shape) != (n,)):
        raise ValueError("mask must be a uint8 or bool tensor [n] (or None)")
    for name, t in (("puzzle_id", puzzle_id), ("plans", plans), ("plan_len", plan_len), ("pos", pos), ("mask", mask)):
        if t is None:
            continue
        if t.device != device:
            raise ValueError(f"{name} must live on {device}")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
    return n


class PlanReplay:
    """What ``replay_plans`` returns; every tensor lives on the device.

    Per item: ``verdict`` int8 [n] (``REPLAY_*``), ``first_goal`` int32 [n] (index of the first goal state, 0 = the start, -1
    none), ``final_pos`` int8 [n, NP, 2], ``offset`` int64 [n + 1] (rows of item i: ``offset[i] : offset[i + 1]``).
    Per row (``num_rows`` of them, None when no rows were asked for): ``item``, ``t``, ``puzzle_id`` int32, ``pos`` int8
    [T, NP, 2] (the state before the action), ``action`` uint8, ``reward`` float64, ``done`` uint8, ``next_pos`` (on request);
    ``obs`` is filled in by ``VecPushWorld.demonstrations``; ``cost`` int32 [T] and ``acts`` uint8 [T] -- the cost-to-go and the
    optimal / safe action bits of the row's state -- by ``VecPushWorld.optimal_demonstrations``."""

    __slots__ = ("verdict", "first_goal", "final_pos", "offset", "num_rows", "item", "t", "puzzle_id", "pos", "action",
                 "reward", "done", "next_pos", "obs", "cost", "acts")

    def __init__(self):
        for name in self.__slots__:
            setattr(self, name, None)


def replay_plans(engine_or_vec, puzzle_id: torch.Tensor, plans: torch.Tensor, plan_len: torch.Tensor,
                 pos: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None, include: str = "valid",
                 rows: bool = True, next_pos: bool = False) -> PlanReplay:
    """Replays a batch of plans on the device (``pw_plan_replay_check`` / ``pw_plan_replay_emit``) on the current stream.

    ``puzzle_id`` int32 [n], ``plans`` uint8 [n, plan_cap] and ``plan_len`` int32 [n] in the formats ``PlanBatch.run`` /
    ``StatePlanner.plan`` leave on the device; ``pos`` int8 [n, NP, 2] start states (None: the puzzles' initial states);
    ``mask`` 0 skips an item.  Every item gets the reference's ``is_valid_plan`` verdict (``REPLAY_VERDICT``); every step of
    every included plan -- ``include`` "valid": the valid ones, "replayed": also those that miss the goal or reach it early --
    becomes one row of the returned ``PlanReplay``.  ``offset[n]`` is read back once to size the rows: the call's only wait.
    ``rows=False``: verdicts only, no wait."""
    engine = engine_or_vec if isinstance(engine_or_vec, _capi.Engine) else getattr(engine_or_vec, "engine", None)
    if not isinstance(engine, _capi.Engine):
        raise ValueError("engine_or_vec must be a VecPushWorld or an _capi.Engine")
    if include not in REPLAY_INCLUDE:
        raise ValueError("include must be 'valid' or 'replayed'")
    dev, npad = engine.device, int(engine.np)
    n = _replay_inputs(puzzle_id, plans, plan_len, pos, mask, npad, dev)
    inc = REPLAY_INCLUDE[include]
    out = PlanReplay()
    out.verdict = torch.empty((n,), dtype=torch.int8, device=dev)
    out.first_goal = torch.empty((n,), dtype=torch.int32, device=dev)
    out.final_pos = torch.empty((n, npad, 2), dtype=torch.int8, device=dev)
    out.offset = torch.empty((n + 1,), dtype=torch.int64, device=dev)
    engine.plan_replay_check(puzzle_id, pos, plans, plan_len, mask, inc, out.verdict, out.first_goal, out.final_pos, out.offset)
    if not rows:
        return out
    T = out.num_rows = int(out.offset[n].item())
    out.item = torch.empty((T,), dtype=torch.int32, device=dev)
    out.t = torch.empty((T,), dtype=torch.int32, device=dev)
    out.puzzle_id = torch.empty((T,), dtype=torch.int32, device=dev)
    out.pos = torch.empty((T, npad, 2), dtype=torch.int8, device=dev)
    out.action = torch.empty((T,), dtype=torch.uint8, device=dev)
    out.reward = torch.empty((T,), dtype=torch.float64, device=dev)
    out.done = torch.empty((T,), dtype=torch.uint8, device=dev)
    if next_pos:
        out.next_pos = torch.empty((T, npad, 2), dtype=torch.int8, device=dev)
    if T > 0:
        engine.plan_replay_emit(puzzle_id, pos, plans, plan_len, mask, inc, out.verdict, out.offset, T, out.item, out.t,
                                out.puzzle_id, out.pos, out.action, out.reward, out.done, out.next_pos)
    return out



# ---- walk regions and push moves (pw_walk_regions / pw_walk_pushes) ----------------------------------------------
WALK_OUTSIDE = 0xFFFF  # walk_map entry of a position outside the region
_WALK_D = ((-1, 0), (1, 0), (0, -1), (0, 1))


def _walk_inputs(puzzle_id, pos, mask, npad: int, device) -> int:
    """The checks of ``walk_regions`` on its device arrays; returns n."""
    if not isinstance(puzzle_id, torch.Tensor) or puzzle_id.dtype != torch.int32 or puzzle_id.dim() != 1:
        raise ValueError("puzzle_id must be an int32 tensor [n]")
    n = int(puzzle_id.shape[0])
    if n < 1 or n >= 1 << 31:
        raise ValueError("puzzle_id must hold 1 .. 2^31 - 1 items")
    if pos is not None and (not isinstance(pos, torch.Tensor) or pos.dtype != torch.int8 or tuple(pos.shape) != (n, npad, 2)):
        raise ValueError(f"pos must be an int8 tensor [n, {npad}, 2] (the engine's state layout) or None")
    if mask is not None and (not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.uint8, torch.bool)
                             or tuple(mask.shape) != (n,)):
        raise ValueError("mask must be a uint8 or bool tensor [n] (or None)")
    for name, t in (("puzzle_id", puzzle_id), ("pos", pos), ("mask", mask)):
        if t is None:
            continue
        if t.device != device:
            raise ValueError(f"{name} must live on {device}")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
    return n


class PushMoves:
    """The rows of ``WalkRegions.pushes``, on the device: ``item`` int32 [T], ``frm`` int8 [T, 2] (the agent position the push
    starts from), ``action`` uint8 [T], ``walk`` int32 [T] (walk distance to ``frm``), ``moved`` int32 [T] holding the 32 bits
    of the C ABI's uint32 mask (bit j: movable j moved; with 32 movables bit 31 makes the number negative: test bits, or take
    ``moved.to(torch.int64) & 0xFFFFFFFF``), ``goal`` uint8 [T], ``next_pos`` int8 [T, NP, 2]; ``dropped`` int64 [1]: rows
    beyond ``cap``."""

    __slots__ = ("num_rows", "item", "frm", "action", "walk", "moved", "goal", "next_pos", "dropped")

    def __init__(self):
        for name in self.__slots__:
            setattr(self, name, None)


class WalkRegions:
    """What ``walk_regions`` returns; every tensor lives on the device.  ``region_size`` int32 [n] (-1: skipped item),
    ``canon`` int8 [n, 2] (x, y), ``offset`` int64 [n + 1] (push rows of item i: ``offset[i] : offset[i + 1]``), ``walk_map``
    uint16 [n, map_h, map_w] or None (``WALK_OUTSIDE`` outside the region, else ``dist | parent << 12``)."""

    def __init__(self, engine, puzzle_id, pos, mask):
        self.engine, self.puzzle_id, self.pos, self.mask = engine, puzzle_id, pos, mask
        self.region_size = self.canon = self.offset = self.walk_map = None
        self._num_pushes = None
        self._host_maps = {}

    @property
    def num_pushes(self) -> int:
        """The total number of push moves (``offset[n]``; read back once: the object's only wait)."""
        if self._num_pushes is None:
            self._num_pushes = int(self.offset[-1].item())
        return self._num_pushes

    def pushes(self, cap: Optional[int] = None) -> PushMoves:
        """Every push move of every item as rows (``pw_walk_pushes``); ``cap`` rows at the most (default: all of them)."""
        T = self.num_pushes if cap is None else int(cap)
        if T < 0:
            raise ValueError("cap must be >= 0")
        dev, npad = self.engine.device, int(self.engine.np)
        out = PushMoves()
        out.num_rows = T
        out.item = torch.empty((T,), dtype=torch.int32, device=dev)
        out.frm = torch.empty((T, 2), dtype=torch.int8, device=dev)
        out.action = torch.empty((T,), dtype=torch.uint8, device=dev)
        out.walk = torch.empty((T,), dtype=torch.int32, device=dev)
        out.moved = torch.empty((T,), dtype=torch.int32, device=dev)
        out.goal = torch.empty((T,), dtype=torch.uint8, device=dev)
        out.next_pos = torch.empty((T, npad, 2), dtype=torch.int8, device=dev)
        out.dropped = torch.zeros((1,), dtype=torch.int64, device=dev)
        self.engine.walk_pushes(self.puzzle_id, self.pos, self.mask, self.offset, T, out.item, out.frm, out.action, out.walk,
                                out.moved, out.goal, out.next_pos, out.dropped)
        return out

    def path(self, i: int, xy) -> List[int]:
        """The walk actions from item ``i``'s agent position to ``xy`` along the parent actions of its walk map (on the host)."""
        if self.walk_map is None:
            raise ValueError("the walk maps were not requested (walk_regions(..., maps=True))")
        i = int(i)
        if not 0 <= i < self.walk_map.shape[0]:
            raise ValueError("item index out of range")
        m = self._host_maps.get(i)
        if m is None:
            m = self._host_maps[i] = self.walk_map[i].cpu().numpy()
        x, y = int(xy[0]), int(xy[1])
        acts: List[int] = []
        while True:
            if not (0 <= y < m.shape[0] and 0 <= x < m.shape[1]) or int(m[y, x]) == WALK_OUTSIDE:
                raise ValueError(f"({xy[0]}, {xy[1]}) is not in the walk region of item {i}")
            e = int(m[y, x])
            if e & 0xFFF == 0:
                return acts[::-1]
            if len(acts) > m.size:
                raise ValueError("the walk map holds a cycle")
            a = e >> 12
            acts.append(a)
            x, y = x - _WALK_D[a][0], y - _WALK_D[a][1]


def walk_regions(engine_or_vec, puzzle_id: torch.Tensor, pos: Optional[torch.Tensor] = None,
                 mask: Optional[torch.Tensor] = None, maps: bool = False) -> WalkRegions:
    """The agent's walk region of every state of a batch (``pw_walk_regions``) on the current stream, no wait: where the agent
    can go without displacing anything, the canonical agent position, and how many push moves are available anywhere in the
    region (``offset``; ``region_size > 0`` and ``offset[i + 1] > offset[i]`` is the "any push available" mask).
    ``puzzle_id`` int32 [n]; ``pos`` int8 [n, NP, 2] (None: the initial states); ``mask`` 0 skips an item; ``maps``: also the
    walk maps (2 bytes per cell of the set's largest board and item).  ``.pushes()`` lists the push moves."""
    engine = engine_or_vec if isinstance(engine_or_vec, _capi.Engine) else getattr(engine_or_vec, "engine", None)
    if not isinstance(engine, _capi.Engine):
        raise ValueError("engine_or_vec must be a VecPushWorld or an _capi.Engine")
    dev, npad = engine.device, int(engine.np)
    n = _walk_inputs(puzzle_id, pos, mask, npad, dev)
    out = WalkRegions(engine, puzzle_id, pos, mask)
    out.region_size = torch.empty((n,), dtype=torch.int32, device=dev)
    out.canon = torch.empty((n, 2), dtype=torch.int8, device=dev)
    out.offset = torch.empty((n + 1,), dtype=torch.int64, device=dev)
    if maps:
        out.walk_map = torch.empty((n, engine.pset.max_height, engine.pset.max_width), dtype=torch.uint16, device=dev)
    engine.walk_regions(puzzle_id, pos, mask, out.region_size, out.canon, out.offset, out.walk_map)
    return out


def push_mask(engine_or_vec, puzzle_id: torch.Tensor, pos: Optional[torch.Tensor] = None,
              mask: Optional[torch.Tensor] = None):
    """The dense push mask of every state of a batch (``pw_push_mask``) on the current stream, no wait: ``(push_mask,
    num_pushes)``, uint8 [n, map_h, map_w] and int32 [n] on the device.  Bit ``a`` of entry ``[y, x]`` is set exactly when
    ``((x, y), a)`` is a push move of item i -- a row of ``walk_regions(...).pushes()`` -- and ``num_pushes`` counts them;
    a skipped item (masked out, an id outside the set, a movable outside its grid) holds zeros.  ``map_h`` / ``map_w`` are the
    set's largest dimensions; inputs as ``walk_regions``."""
    engine = engine_or_vec if isinstance(engine_or_vec, _capi.Engine) else getattr(engine_or_vec, "engine", None)
    if not isinstance(engine, _capi.Engine):
        raise ValueError("engine_or_vec must be a VecPushWorld or an _capi.Engine")
    dev, npad = engine.device, int(engine.np)
    n = _walk_inputs(puzzle_id, pos, mask, npad, dev)
    out = torch.empty((n, engine.pset.max_height, engine.pset.max_width), dtype=torch.uint8, device=dev)
    count = torch.empty((n,), dtype=torch.int32, device=dev)
    engine.push_mask(puzzle_id, pos, mask, out, count)
    return out, count


def decode_push_choice(choice: torch.Tensor, map_h: int, map_w: int):
    """``(push_from int8 [B, 2], push_action uint8 [B])`` of ``choice``, int64 [B] flat indices into ``[4, map_h, map_w]`` (the
    expanded push mask's shape: ``(a * map_h + y) * map_w + x``), with torch ops on ``choice``'s device.  An index outside
    the shape decodes to an action outside 0..3, a choice that is no push move."""
    cells = int(map_h) * int(map_w)
    inside = (choice >= 0) & (choice < 4 * cells)
    c = torch.where(inside, choice, torch.zeros_like(choice))
    action = torch.where(inside, torch.div(c, cells, rounding_mode="floor"), torch.full_like(choice, PUSH_NONE)).to(torch.uint8)
    cell = c % cells
    frm = torch.stack((cell % int(map_w), torch.div(cell, int(map_w), rounding_mode="floor")), dim=1).to(torch.int8)
    return frm.contiguous(), action.contiguous()


class PushSearch:
    """Breadth-first search over pushes: the nodes are canonical states (the other movables, and the agent at the smallest
    position of its walk region), the successors of a node are the push moves available anywhere in the region.  One layer
    of pushes per round: ``pw_walk_regions`` + ``pw_walk_pushes`` on the frontier, ``pw_walk_regions`` on the successors for
    their canonical positions, an exact dedupe against the closed set on the device (``torch.unique`` over the packed rows).

    After ``solve``: ``layer_states`` -- the new canonical states of every completed layer before the one that met a goal;
    ``num_states`` -- the canonical states closed (when a goal was met: up to and including the goal row's successor, what a
    FIFO search has closed at its first goal); ``pushes`` -- the pushes of the plan (None without one); ``push_rows`` and
    ``largest_region`` -- push moves listed and the largest walk region seen."""

    def __init__(self, puzzle, max_states: int = 1 << 20):
        self.puzzle = puzzle
        self._engine = puzzle._engine()
        self.device = self._engine.device
        self.num_objects = puzzle.num_movables
        self.puzzle_index = int(getattr(puzzle, "puzzle_index", 0))
        self.max_states = int(max_states)
        if self.max_states < 1:
            raise ValueError("max_states must be >= 1")
        self.layer_states: List[int] = []
        self.num_states = 0
        self.pushes: Optional[int] = None
        self.push_rows = 0
        self.largest_region = 0

    def _ids(self, n: int) -> torch.Tensor:
        return torch.full((n,), self.puzzle_index, dtype=torch.int32, device=self.device)

    def _keys(self, pos: torch.Tensor, canon: torch.Tensor) -> torch.Tensor:
        """The packed canonical states: the rows of ``pos`` with the agent's slot replaced by ``canon``, as bytes."""
        k = pos.clone()
        k[:, 0, :] = canon
        return k.view(torch.uint8).reshape(pos.shape[0], -1)

    def solve(self, start: Optional[Sequence[Tuple[int, int]]] = None, max_pushes: Optional[int] = None,
              stop_at_goal: bool = True) -> Optional[List[int]]:
        """Primitive actions of a plan with the fewest pushes (the first goal row in frontier order, then row order; the walks
        between pushes are shortest), ``[]`` for a start that is a goal, or None when the space (or ``max_pushes``) is exhausted
        without one.  ``stop_at_goal=False`` searches on through goal states until the space is exhausted and returns None.
        ``ValueError`` beyond ``max_states`` closed states."""
        eng, dev, npad, N = self._engine, self.device, int(self._engine.np), self.num_objects
        state0 = tuple(tuple(int(v) for v in xy) for xy in (self.puzzle.initial_state if start is None else start))
        if len(state0) != N:
            raise ValueError("start must hold one (x, y) pair per movable")
        self.layer_states, self.pushes, self.push_rows, self.largest_region = [], None, 0, 0
        self.num_states = 1
        if any(not -128 <= v <= 127 for xy in state0 for v in xy):
            raise ValueError("start has a movable outside the grid")
        frontier = torch.zeros((1, npad, 2), dtype=torch.int8, device=dev)
        frontier[0, :N] = torch.tensor(state0, dtype=torch.int8)
        first = walk_regions(eng, self._ids(1), frontier)
        if int(first.region_size[0].item()) < 0:
            raise ValueError("start has a movable outside the grid")
        if stop_at_goal and self.puzzle.is_goal_state(state0):
            self.pushes = 0
            return []
        closed = self._keys(frontier, first.canon)
        # per closed state: the state as it was reached, and the push that reached it (parent index, from, action)
        real, parent = [frontier], [torch.full((1,), -1, dtype=torch.int64, device=dev)]
        frm, action = [torch.zeros((1, 2), dtype=torch.int8, device=dev)], [torch.zeros((1,), dtype=torch.uint8, device=dev)]
        base, depth, goal = 0, 0, None  # base: closed index of the frontier's first state
        while frontier.shape[0] > 0 and (max_pushes is None or depth < max_pushes):
            depth += 1
            F = frontier.shape[0]
            reg = walk_regions(eng, self._ids(F), frontier)
            rows = reg.pushes()
            T = rows.num_rows
            self.push_rows += T
            self.largest_region = max(self.largest_region, int(reg.region_size.max().item()))
            if T == 0:
                self.layer_states.append(0)
                break
            succ = walk_regions(eng, self._ids(T), rows.next_pos)
            ok = succ.region_size > 0
            keys = self._keys(rows.next_pos, succ.canon)
            C = closed.shape[0]
            _, inv = torch.unique(torch.cat([closed, keys]), dim=0, return_inverse=True)
            lowest = torch.full((int(inv.max().item()) + 1,), C + T, dtype=torch.int64, device=dev)
            # a successor outside its grid (canon (0, 0), which a successor inside can share) closes nothing: it takes no
            # part in the choice of the first row of a canonical state
            order = torch.arange(C + T, device=dev)
            order[C:][~ok] = C + T
            lowest.scatter_reduce_(0, inv, order, "amin")
            # a row is new when it is the first of its canonical state and no closed state holds it
            is_new = (lowest[inv[C:]] == torch.arange(C, C + T, device=dev)) & ok
            new_rows = torch.nonzero(is_new).reshape(-1)  # (ascending: frontier order, then row order)
            goal_rows = torch.nonzero(rows.goal != 0).reshape(-1) if stop_at_goal else new_rows[:0]
            if goal_rows.numel() > 0:
                g = int(goal_rows[0].item())
                self.num_states = C + int((new_rows <= g).sum().item())
                goal = (base + int(rows.item[g].item()), tuple(int(v) for v in rows.frm[g].tolist()), int(rows.action[g].item()))
                break
            M = int(new_rows.numel())
            if C + M > self.max_states:
                raise ValueError(f"PushSearch: more than max_states = {self.max_states} canonical states")
            self.layer_states.append(M)
            self.num_states = C + M
            frontier = rows.next_pos[new_rows].contiguous()
            closed = torch.cat([closed, keys[new_rows]])
            real.append(frontier)
            parent.append(base + rows.item[new_rows].to(torch.int64))
            frm.append(rows.frm[new_rows])
            action.append(rows.action[new_rows])
            base = C
        if goal is None:
            return None
        # the chain of pushes back to the start, then the walks between them from the walk maps of the states on the chain
        par, frs, acs = torch.cat(parent).cpu().numpy(), torch.cat(frm).cpu().numpy(), torch.cat(action).cpu().numpy()
        chain = [goal]
        while par[chain[-1][0]] >= 0:
            k = chain[-1][0]
            chain.append((int(par[k]), (int(frs[k][0]), int(frs[k][1])), int(acs[k])))
        chain.reverse()
        states = torch.cat(real)[torch.tensor([k for k, _, _ in chain], device=dev)].contiguous()
        maps = walk_regions(eng, self._ids(len(chain)), states, maps=True)
        plan: List[int] = []
        for i, (_, q, a) in enumerate(chain):
            plan += maps.path(i, q) + [a]
        self.pushes = len(chain)
        return plan


class PushLayerInfo(tuple):
    """(depth, new_states, total_states, goal_index, push_rows, largest_region) of one ``PushBreadthFirstSearch.expand``."""

    depth = property(lambda self: self[0])
    new_states = property(lambda self: self[1])
    total_states = property(lambda self: self[2])
    goal_index = property(lambda self: self[3])
    push_rows = property(lambda self: self[4])
    largest_region = property(lambda self: self[5])


class PushBreadthFirstSearch:
    """Breadth-first search over pushes with the closed set, the store and the links on the device (``pw_push_search_*``,
    DESIGN.md K16): ``PushSearch``'s nodes, numbering, plans and counters, shaped like ``BreadthFirstSearch``.  A layer is one
    ``expand``; the closed set is a hash table in HBM, exact at every number of movables.

    Args:
        puzzle: a ``PushWorldPuzzle`` or ``SetPuzzle``.
        max_states: capacity of the store (device memory ~ ``max_states * (2 NP + 22)`` bytes plus 16 .. 32 bytes of table).
        stop_at_goal: end in the first layer that holds a push into a goal state; False: search on until a layer is empty.
        chunk: parents per pass (default 2^16; tests use small values to force many passes per layer).

    After ``solve`` (or any ``expand``): ``layer_states``, ``num_states``, ``pushes``, ``push_rows``, ``largest_region`` with
    ``PushSearch``'s meaning; ``layers`` [(first index, count)] per depth, ``goal_index``, ``exhausted``."""

    def __init__(self, puzzle, max_states: int = 1 << 20, stop_at_goal: bool = True, chunk: Optional[int] = None):
        self._handle = None
        self.max_states = int(max_states)
        if not 1 <= self.max_states < 1 << 31:  # (before an engine is asked for)
            raise ValueError("max_states must be in 1 .. 2^31 - 1")
        if chunk is not None and int(chunk) < 1:
            raise ValueError("chunk must be >= 1")
        self.puzzle = puzzle
        self._engine = puzzle._engine()
        self.device = self._engine.device
        self.num_objects = puzzle.num_movables
        self.puzzle_index = int(getattr(puzzle, "puzzle_index", 0))
        self.stop_at_goal = bool(stop_at_goal)
        self._engine.set_option("search_chunk", 0 if chunk is None else int(chunk))
        try:
            self._handle = _capi.PushSearchHandle(self._engine, self.puzzle_index, self.max_states)
        finally:
            self._engine.set_option("search_chunk", 0)
        self._reset()
        self._begun = False

    def _reset(self) -> None:
        self.layer_states: List[int] = []
        self.layers: List[Tuple[int, int]] = []
        self.num_states = 0
        self.pushes: Optional[int] = None
        self.push_rows = 0
        self.largest_region = 0
        self.goal_index = -1
        self.exhausted = False

    def begin(self, start: Optional[Sequence[Tuple[int, int]]] = None) -> None:
        """Starts a search from ``start`` (a reference-style state, default: the initial state).  ``ValueError`` for a start
        with a movable outside the grid."""
        state0 = tuple(tuple(int(v) for v in xy) for xy in (self.puzzle.initial_state if start is None else start))
        if len(state0) != self.num_objects or any(len(xy) != 2 for xy in state0):
            raise ValueError("start must hold one (x, y) pair per movable")
        if self._handle is None:
            raise ValueError("the search is closed")
        if any(not -128 <= v <= 127 for xy in state0 for v in xy):
            raise ValueError("start has a movable outside the grid")
        self._begun = False
        self._reset()
        try:
            self._handle.begin(None if start is None else bytes(v & 0xFF for xy in state0 for v in xy), self.stop_at_goal)
        except ValueError as exc:
            raise ValueError(f"start has a movable outside the grid ({exc})") from None
        self._begun = True
        self.num_states = 1
        self.layers = [(0, 1)]
        if self.stop_at_goal and self.puzzle.is_goal_state(state0):
            self.goal_index, self.pushes = 0, 0

    def expand(self) -> PushLayerInfo:
        """One layer of pushes from the newest layer; ``ValueError`` when the store is full."""
        if not self._begun:
            raise ValueError("begin() has not been called")
        rc, info = self._handle.expand()
        if rc in (_capi.PW_OK, _capi.PW_ELIMIT):
            depth, new, total, goal, rows, largest = info
            if rc == _capi.PW_OK or total > self.num_states:
                self.push_rows += rows
                self.largest_region = largest
                self.num_states = total
                self.goal_index = goal
                if new:
                    self.layers.append((total - new, new))
        _capi.check(rc)
        if goal >= 0:
            self.pushes = depth
        else:
            self.layer_states.append(new)
            self.exhausted = new == 0
        return PushLayerInfo(info)

    def states(self, first: int = 0, count: Optional[int] = None):
        """(pos int8 [count, NP, 2] the states as reached, canon int8 [count, 2]) of states ``first .. first + count - 1``,
        on the device."""
        count = self.num_states - first if count is None else count
        pos = torch.empty((count, int(self._engine.np), 2), dtype=torch.int8, device=self.device)
        canon = torch.empty((count, 2), dtype=torch.int8, device=self.device)
        self._handle.read_states(first, count, pos, canon)
        return pos, canon

    def links(self, first: int = 0, count: Optional[int] = None):
        """(parent int32, from int8 [count, 2], action uint8, walk int32, goal uint8) device tensors; the start state has
        parent -1 and action 0xFF."""
        count = self.num_states - first if count is None else count
        parent = torch.empty((count,), dtype=torch.int32, device=self.device)
        frm = torch.empty((count, 2), dtype=torch.int8, device=self.device)
        action = torch.empty((count,), dtype=torch.uint8, device=self.device)
        walk = torch.empty((count,), dtype=torch.int32, device=self.device)
        goal = torch.empty((count,), dtype=torch.uint8, device=self.device)
        self._handle.read_links(first, count, parent, frm, action, walk, goal)
        return parent, frm, action, walk, goal

    def plan(self, index: int) -> List[int]:
        """Primitive actions from the start to state ``index``: shortest walks between the pushes of its chain of links."""
        if not self._begun:
            raise ValueError("begin() has not been called")
        return self._handle.plan(index)[0]

    def solve(self, max_pushes: Optional[int] = None) -> Optional[List[int]]:
        """As ``PushSearch.solve``: a plan with the fewest pushes, ``[]`` for a start that is a goal state, None when the space
        (or ``max_pushes``) is exhausted without one.  ``ValueError`` beyond ``max_states``."""
        if not self._begun:
            self.begin()
        while self.goal_index < 0 and not self.exhausted:
            if max_pushes is not None and len(self.layer_states) >= max_pushes:
                return None
            self.expand()
        return self.plan(self.goal_index) if self.goal_index >= 0 else None

    def close(self) -> None:
        h = getattr(self, "_handle", None)
        if h is not None:
            h.close()
        self._handle = None
        self._begun = False

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    __del__ = close


class PushPlannerInfo(tuple):
    """(status, rounds, expanded, states, open, goal_index, rgd_exceeded, push_rows, largest_region, largest_key) of a
    ``PushBestFirstSearch``."""

    status = property(lambda self: PLAN_STATUS[self[0]])
    rounds = property(lambda self: self[1])
    expanded = property(lambda self: self[2])
    states = property(lambda self: self[3])
    open = property(lambda self: self[4])
    goal_index = property(lambda self: self[5])
    rgd_exceeded = property(lambda self: self[6])
    push_rows = property(lambda self: self[7])
    largest_region = property(lambda self: self[8])
    largest_key = property(lambda self: self[9])


class PushBestFirstSearch:
    """Best-first search over pushes (``pw_push_planner_*``): ``PushBreadthFirstSearch``'s nodes, store,
    closed set and links, expanded in the order of the RGD heuristic (fewest tools) of the state as reached, ``batch`` = K
    states per round.  See ``pw_push_planner_create`` in include/pushworld_amd.h for the exact semantics.

    Args:
        puzzle: a ``PushWorldPuzzle`` or ``SetPuzzle``.
        batch: states popped per round, 1 .. 65536.
        max_states: capacity of the store; a round whose push rows could overflow it is not expanded (status ``limit``).
        rgd_budget: RGD recursion frames per state (None: the default); states beyond it get NaN keys and pop last.

    After ``run``: ``info`` (``PushPlannerInfo``), ``num_states``, ``goal_index``; after ``plan``: ``pushes``."""

    def __init__(self, puzzle, batch: int = 1, max_states: int = 1 << 20, rgd_budget: Optional[int] = None):
        self._handle = None
        self.batch, self.max_states = int(batch), int(max_states)
        if not 1 <= self.max_states < 1 << 31:  # (before an engine is asked for)
            raise ValueError("max_states must be in 1 .. 2^31 - 1")
        if not 1 <= self.batch <= 65536:
            raise ValueError("batch must be in 1 .. 65536")
        if rgd_budget is not None and int(rgd_budget) < 1:
            raise ValueError("rgd_budget must be >= 1 (or None)")
        self.puzzle = puzzle
        self._engine = puzzle._engine()
        self.device = self._engine.device
        self.num_objects = puzzle.num_movables
        self.puzzle_index = int(getattr(puzzle, "puzzle_index", 0))
        self._handle = _capi.PushPlannerHandle(self._engine, self.puzzle_index, self.max_states, self.batch,
                                               0 if rgd_budget is None else int(rgd_budget))
        self._reset()
        self._begun = False

    def _reset(self) -> None:
        self.info: Optional[PushPlannerInfo] = None
        self.num_states = 0
        self.goal_index = -1
        self.pushes: Optional[int] = None

    def begin(self, start: Optional[Sequence[Tuple[int, int]]] = None) -> None:
        """Starts a search from ``start`` (a reference-style state, default: the initial state).  ``ValueError`` for a start
        with a movable outside the grid."""
        state0 = tuple(tuple(int(v) for v in xy) for xy in (self.puzzle.initial_state if start is None else start))
        if len(state0) != self.num_objects or any(len(xy) != 2 for xy in state0):
            raise ValueError("start must hold one (x, y) pair per movable")
        if self._handle is None:
            raise ValueError("the search is closed")
        if any(not -128 <= v <= 127 for xy in state0 for v in xy):
            raise ValueError("start has a movable outside the grid")
        self._begun = False
        self._reset()
        try:
            self._handle.begin(None if start is None else bytes(v & 0xFF for xy in state0 for v in xy))
        except ValueError as exc:
            raise ValueError(f"start has a movable outside the grid ({exc})") from None
        self._begun = True
        self.num_states = 1

    def run(self, max_rounds: Optional[int] = None) -> PushPlannerInfo:
        """Runs at most ``max_rounds`` rounds (None: until the search is solved, exhausted or at its limit)."""
        rounds = 0 if max_rounds is None else int(max_rounds)
        if max_rounds is not None and rounds <= 0:
            raise ValueError("max_rounds must be positive (or None)")
        if not self._begun:
            raise ValueError("begin() has not been called")
        self.info = PushPlannerInfo(self._handle.run(rounds))
        self.num_states, self.goal_index = self.info.states, self.info.goal_index
        return self.info

    def states(self, first: int = 0, count: Optional[int] = None):
        """(pos int8 [count, NP, 2] the states as reached, canon int8 [count, 2]) of states ``first .. first + count - 1``,
        on the device."""
        count = self.num_states - first if count is None else count
        pos = torch.empty((count, int(self._engine.np), 2), dtype=torch.int8, device=self.device)
        canon = torch.empty((count, 2), dtype=torch.int8, device=self.device)
        self._handle.read_states(first, count, pos, canon)
        return pos, canon

    def links(self, first: int = 0, count: Optional[int] = None):
        """(parent int32, from int8 [count, 2], action uint8, walk int32, goal uint8) device tensors; the start state has
        parent -1 and action 0xFF."""
        count = self.num_states - first if count is None else count
        parent = torch.empty((count,), dtype=torch.int32, device=self.device)
        frm = torch.empty((count, 2), dtype=torch.int8, device=self.device)
        action = torch.empty((count,), dtype=torch.uint8, device=self.device)
        walk = torch.empty((count,), dtype=torch.int32, device=self.device)
        goal = torch.empty((count,), dtype=torch.uint8, device=self.device)
        self._handle.read_links(first, count, parent, frm, action, walk, goal)
        return parent, frm, action, walk, goal

    def plan(self) -> Optional[List[int]]:
        """The plan (list of actions 0..3) when the search is solved, else None."""
        if self.info is None or self.info.status != "solved":
            return None
        plan, self.pushes = self._handle.plan()
        return plan

    def solve(self) -> Optional[List[int]]:
        """The plan found, ``[]`` for a start that is a goal state, None when the space is exhausted without one.
        ``RuntimeError`` when ``max_states`` runs out first."""
        if not self._begun:
            self.begin()
        if self.run().status == "limit":
            raise RuntimeError(f"best-first search over pushes stopped at max_states = {self.max_states} without an answer")
        return self.plan()

    def close(self) -> None:
        h = getattr(self, "_handle", None)
        if h is not None:
            h.close()
        self._handle = None
        self._begun = False

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    __del__ = close


# ---- exact cost-to-go tables over pushes (pw_push_search_solve / pw_push_search_table_*) ------------------------
PUSH_NONE = 0xFF  # ``PushQuery.push_action`` where a state has no best row


PushQuery = namedtuple("PushQuery", "index cost action push_from push_action walk")
PushQuery.__doc__ = """What ``PushSolutionTable.query`` returns: device tensors [n] ([n, 2] for ``push_from``)."""


def _push_query_outputs(out, n: int, device) -> PushQuery:
    """The six tensors a push-table query fills: fresh (-1 / ``COST_UNKNOWN`` / -1 / (0, 0) / ``PUSH_NONE`` / -1) or the
    checked ``out``."""
    if out is None:
        return PushQuery(torch.full((n,), -1, dtype=torch.int32, device=device),
                         torch.full((n,), COST_UNKNOWN, dtype=torch.int32, device=device),
                         torch.full((n,), -1, dtype=torch.int8, device=device),
                         torch.zeros((n, 2), dtype=torch.int8, device=device),
                         torch.full((n,), PUSH_NONE, dtype=torch.uint8, device=device),
                         torch.full((n,), -1, dtype=torch.int32, device=device))
    if not isinstance(out, (tuple, list)) or len(out) != 6:
        raise ValueError("out must be the PushQuery of an earlier query")
    for name, t, dtype, shape in zip(PushQuery._fields, out, (torch.int32, torch.int32, torch.int8, torch.int8, torch.uint8,
                                                              torch.int32), ((n,), (n,), (n,), (n, 2), (n,), (n,))):
        _dev_tensor(f"out: {name}", t, dtype, shape, device)
    return PushQuery(*out)


PushPlans = namedtuple("PushPlans", "push_from push_action state length")
PushPlans.__doc__ = """What ``PushSolutionTable.plans`` returns: device tensors ``push_from`` int8 [n, plan_cap, 2], ``push_action``
uint8 [n, plan_cap], ``state`` int32 [n, plan_cap] (the node the t-th push is made from) and ``length`` int32 [n]."""

PushRows = namedtuple("PushRows", "item t state push_from push_action cost pos dropped num_rows")
PushRows.__doc__ = """What ``PushSolutionTable.demonstration_rows`` returns: one row per push of every plan -- device tensors
``item`` / ``t`` / ``state`` / ``cost`` int32 [T], ``push_from`` int8 [T, 2], ``push_action`` uint8 [T], ``pos`` int8 [T, NP, 2]
(the state the push is made from), ``dropped`` uint32 [1] (rows beyond the capacity) and ``num_rows``, T as an int."""


def _push_plans_outputs(out, n: int, plan_cap: int, device) -> PushPlans:
    """The four tensors a plans launch fills: fresh (zeros / zeros / -1 / ``PLANS_NONE``) or the checked ``out``."""
    if out is None:
        return PushPlans(torch.zeros((n, plan_cap, 2), dtype=torch.int8, device=device),
                         torch.zeros((n, plan_cap), dtype=torch.uint8, device=device),
                         torch.full((n, plan_cap), -1, dtype=torch.int32, device=device),
                         torch.full((n,), PLANS_NONE, dtype=torch.int32, device=device))
    if not isinstance(out, (tuple, list)) or len(out) != 4:
        raise ValueError("out must be the PushPlans of an earlier call")
    for name, t, dtype, shape in zip(PushPlans._fields, out, (torch.int8, torch.uint8, torch.int32, torch.int32),
                                     ((n, plan_cap, 2), (n, plan_cap), (n, plan_cap), (n,))):
        _dev_tensor(f"out: {name}", t, dtype, shape, device)
    return PushPlans(*out)


def encode_push_choice(push_from: torch.Tensor, push_action: torch.Tensor, map_h: int, map_w: int) -> torch.Tensor:
    """int64 [B] flat indices into ``[4, map_h, map_w]`` of the pushes ``push_from`` (int8 [B, 2]) / ``push_action`` (uint8 [B]):
    ``(a * map_h + y) * map_w + x``, the exact inverse of ``decode_push_choice``; -1 for a push outside the shape."""
    x, y, a = push_from[:, 0].to(torch.int64), push_from[:, 1].to(torch.int64), push_action.to(torch.int64)
    inside = (x >= 0) & (x < int(map_w)) & (y >= 0) & (y < int(map_h)) & (a < 4)
    return torch.where(inside, (a * int(map_h) + y) * int(map_w) + x, torch.full_like(a, -1))


def _push_plans_call(table, ids_optional: bool, index, puzzle_id, mask, tie, seed, plan_cap, out) -> PushPlans:
    """The checks and the one launch of ``PushSolutionTable.plans`` / ``PushSolutionTableBatch.plans``."""
    device = table.device
    if not isinstance(index, torch.Tensor) or index.dtype != torch.int32 or index.dim() != 1:
        raise ValueError("index must be an int32 tensor [n] (store indices, as query returns them)")
    n = int(index.shape[0])
    if n < 1 or n >= 1 << 31:
        raise ValueError("index must hold 1 .. 2^31 - 1 items")
    _dev_tensor("index", index, torch.int32, (n,), device)
    _dev_tensor("puzzle_id", puzzle_id, torch.int32, (n,), device, optional=ids_optional)
    _dev_tensor("mask", mask, (torch.uint8, torch.bool), (n,), device, optional=True)
    if tie not in TABLE_TIES:
        raise ValueError("tie must be 'lowest' or 'uniform'")
    plan_cap = int(plan_cap)
    if not 1 <= plan_cap <= _capi.PLAN_MAX_ACTIONS:
        raise ValueError(f"plan_cap must be in 1 .. {_capi.PLAN_MAX_ACTIONS}")
    out = _push_plans_outputs(out, n, plan_cap, device)
    table._plans_launch(index, puzzle_id, mask, n, TABLE_TIES[tie], seed, out.push_from, out.push_action, out.state, plan_cap,
                        out.length)
    return out


def _push_rows_call(table, ids_optional: bool, plans, pos, puzzle_id, mask, rows_cap, offset, out) -> PushRows:
    """The checks and the one launch of ``PushSolutionTable.demonstration_rows`` / ``PushSolutionTableBatch.demonstration_rows``."""
    device = table.device
    if not isinstance(plans, (tuple, list)) or len(plans) != 4 or not isinstance(plans[3], torch.Tensor) \
            or plans[3].dim() != 1 or not isinstance(plans[1], torch.Tensor) or plans[1].dim() != 2:
        raise ValueError("plans must be the PushPlans of a plans call")
    n, plan_cap = int(plans[3].shape[0]), int(plans[1].shape[1])
    if n < 1 or plan_cap < 1:
        raise ValueError("plans must hold at least one item and one step")
    plans = _push_plans_outputs(plans, n, plan_cap, device)
    _dev_tensor("pos", pos, torch.int8, (n, table.npad, 2), device, optional=True)
    _dev_tensor("puzzle_id", puzzle_id, torch.int32, (n,), device, optional=ids_optional)
    _dev_tensor("mask", mask, (torch.uint8, torch.bool), (n,), device, optional=True)
    if offset is None:
        lens = plans.length.clamp(min=0).to(torch.int64)
        if mask is not None:
            lens = lens * (mask != 0)
        if puzzle_id is not None:
            lens = lens * table.covers(puzzle_id)
        offset = torch.zeros((n + 1,), dtype=torch.int64, device=device)
        torch.cumsum(lens, 0, out=offset[1:])
    _dev_tensor("offset", offset, torch.int64, (n + 1,), device)
    if out is not None:
        if not isinstance(out, (tuple, list)) or len(out) != 9 or not isinstance(out[0], torch.Tensor) or out[0].dim() != 1:
            raise ValueError("out must be the PushRows of an earlier call")
        cap = int(out[0].shape[0])
        rows_cap = cap if rows_cap is None else int(rows_cap)
        if rows_cap > cap:
            raise ValueError("rows_cap must not exceed the rows of out")
    elif rows_cap is None:
        table._live()
        rows_cap = int(offset[n].cpu())  # the one wait: the number of rows
    rows_cap = int(rows_cap)
    if rows_cap < 0:
        raise ValueError("rows_cap must be >= 0")
    if out is None:
        cap = rows_cap
        out = PushRows(torch.full((cap,), -1, dtype=torch.int32, device=device),
                       torch.full((cap,), -1, dtype=torch.int32, device=device),
                       torch.full((cap,), -1, dtype=torch.int32, device=device),
                       torch.zeros((cap, 2), dtype=torch.int8, device=device),
                       torch.full((cap,), PUSH_NONE, dtype=torch.uint8, device=device),
                       torch.full((cap,), -1, dtype=torch.int32, device=device),
                       torch.zeros((cap, table.npad, 2), dtype=torch.int8, device=device),
                       torch.zeros((1,), dtype=torch.int32, device=device).view(torch.uint32), cap)
    for name, t, dtype, shape in zip(PushRows._fields[:8], out,
                                     (torch.int32, torch.int32, torch.int32, torch.int8, torch.uint8, torch.int32, torch.int8,
                                      (torch.uint32, torch.int32)),
                                     ((cap,), (cap,), (cap,), (cap, 2), (cap,), (cap,), (cap, table.npad, 2), (1,))):
        _dev_tensor(f"out: {name}", t, dtype, shape, device)
    out = PushRows(*out)
    table._emit_launch(puzzle_id, mask, n, table.npad, plans.push_from, plans.push_action, plans.state, plan_cap, plans.length, pos,
                       offset, rows_cap, out.item, out.t, out.state, out.push_from, out.push_action, out.cost, out.pos, out.dropped)
    return out


class PushSolutionTable:
    """The exact cost-to-go IN PUSHES of every canonical state reachable in one puzzle: a ``PushBreadthFirstSearch`` with
    ``stop_at_goal=False`` run to exhaustion, then ``pw_push_search_solve``.  State i of the search has the push rows
    ``offsets()[i] .. offsets()[i + 1] - 1``, in ``walk_pushes``' (y, x, action) order:

    * ``rows(first, count)``: ``(succ int32, from int8 [count, 2], action uint8, flags uint8)`` -- the store index of the row's
      successor (-1: it lies outside the grid), the push, and bit 0 goal row, bit 1 optimal, bit 2 safe;
    * ``costs()`` int32: pushes to go, 0 at goal states, -1 at dead ends (PushWorld is irreversible: a dead end is a property
      of the boxes alone);
    * ``best()`` int32: the state's lowest optimal row (relative to its first), -1 at goal states and dead ends.

    A cost in moves is not kept: a node holds one agent position for a whole walk region.

    The table is a data source too: ``cost_index`` groups the states by cost, ``sample`` draws start states k
    pushes from the goal for a batch, ``plans`` walks fewest-pushes plans and ``demonstration_rows`` turns them into flat rows.

    Args:
        puzzle: a ``PushWorldPuzzle`` or a ``SetPuzzle``.
        max_states: capacity of the search; ``ValueError`` ("the state store is full") when the space is larger.
        start: the state the space is explored from (default: the initial state).
        chunk: parents per pass, as ``PushBreadthFirstSearch``.

    ``info`` = (states, rows, goal states, dead ends, largest finite cost or -1); ``num_states``, ``num_rows``.
    Device memory: the search's, plus 16 bytes per state and 8 per row."""

    def __init__(self, puzzle, max_states: int = 1 << 20, start: Optional[Sequence[Tuple[int, int]]] = None,
                 chunk: Optional[int] = None):
        self.search = None
        self.puzzle = puzzle
        self.search = PushBreadthFirstSearch(puzzle, max_states=max_states, stop_at_goal=False, chunk=chunk)
        self.puzzle_index = self.search.puzzle_index
        self.device = self.search.device
        self.npad = int(self.search._engine.np)
        try:
            self.search.begin(start)
            self.start = tuple(tuple(int(v) for v in xy) for xy in (puzzle.initial_state if start is None else start))
            while not self.search.exhausted:
                self.search.expand()
            self.info = self.search._handle.solve()
            self.num_states, self.num_rows, self.num_goal_states, self.num_dead_ends, self.max_cost = self.info
        except Exception:
            self.search.close()
            raise

    def _handle(self):
        if self.search is None or self.search._handle is None:
            raise ValueError("the table is closed")
        return self.search._handle

    def states(self, first: int = 0, count: Optional[int] = None):
        """``PushBreadthFirstSearch.states``: (pos int8 [count, NP, 2] the states as reached, canon int8 [count, 2])."""
        self._handle()
        return self.search.states(first, count)

    def offsets(self, first: int = 0, count: Optional[int] = None) -> torch.Tensor:
        """int64 [count + 1] on the device: the first row of states ``first .. first + count`` (absolute row numbers)."""
        h = self._handle()
        count = self.num_states - first if count is None else count
        out = torch.empty((max(count, 0) + 1,), dtype=torch.int64, device=self.device)
        h.table_read(first, count, out, None, None)
        return out

    def costs(self, first: int = 0, count: Optional[int] = None) -> torch.Tensor:
        """int32 [count] on the device: pushes to go, -1 = dead end."""
        h = self._handle()
        count = self.num_states - first if count is None else count
        out = torch.empty((max(count, 0),), dtype=torch.int32, device=self.device)
        h.table_read(first, count, None, out, None)
        return out

    def best(self, first: int = 0, count: Optional[int] = None) -> torch.Tensor:
        """int32 [count] on the device: the lowest optimal row of each state, -1 where there is none."""
        h = self._handle()
        count = self.num_states - first if count is None else count
        out = torch.empty((max(count, 0),), dtype=torch.int32, device=self.device)
        h.table_read(first, count, None, None, out)
        return out

    def rows(self, first: int = 0, count: Optional[int] = None):
        """(succ int32 [count], from int8 [count, 2], action uint8 [count], flags uint8 [count]) of rows
        ``first .. first + count - 1``, on the device."""
        h = self._handle()
        count = self.num_rows - first if count is None else count
        n = max(count, 0)
        succ = torch.empty((n,), dtype=torch.int32, device=self.device)
        frm = torch.empty((n, 2), dtype=torch.int8, device=self.device)
        action = torch.empty((n,), dtype=torch.uint8, device=self.device)
        flags = torch.empty((n,), dtype=torch.uint8, device=self.device)
        h.table_rows(first, count, succ, frm, action, flags)
        return succ, frm, action, flags

    def query(self, puzzle_id: Optional[torch.Tensor], pos: torch.Tensor, mask: Optional[torch.Tensor] = None, out=None,
              actions: bool = True) -> PushQuery:
        """Looks live states up on the device, on the current stream, no wait once the workspace has its size: ``pos`` int8
        [n, NP, 2] (the engine's layout, e.g. ``VecPushWorld.pos``), ``puzzle_id`` int32 [n] (None: every item is this
        table's puzzle), ``mask`` uint8 / bool [n] (0 skips an item).  Returns a ``PushQuery`` of device tensors: the node of
        each state, its cost in pushes (``COST_DEAD_END`` -1), the first primitive action of "walk to ``push_from``, then
        push" (-1 where there is none: goal, dead end, not in the table), the best push ``push_from`` / ``push_action``
        ((0, 0) / ``PUSH_NONE``) and ``walk``, the length of the walk to it in the live state.  A state that is not in the
        table gives -1 / ``COST_UNKNOWN`` -2 / -1 / (0, 0) / 0xFF / -1.  Items of other puzzles and masked items keep what
        ``out`` -- the ``PushQuery`` of an earlier call, filled in place -- held.  ``actions=False`` makes no walk maps and
        leaves ``action`` and ``walk`` as they are.  One query at a time per table."""
        h = self._handle()
        n = _pos_inputs(puzzle_id, pos, mask, self.npad, self.device, True)
        out = _push_query_outputs(out, n, self.device)
        h.table_query(puzzle_id, pos, self.npad, mask, n, out.index, out.cost, out.push_from, out.push_action,
                                   out.walk if actions else None, out.action if actions else None)
        return out

    def optimal_plan(self, start: Optional[Sequence[Tuple[int, int]]] = None) -> Optional[List[int]]:
        """The primitive actions of a fewest-pushes plan from ``start`` (default: the table's start): at every step the
        query's action.  [] at a goal state, None at a dead end or from a state that is not in the table."""
        state = tuple(tuple(int(v) for v in xy) for xy in (self.start if start is None else start))
        if len(state) != self.search.num_objects or any(len(xy) != 2 for xy in state):
            raise ValueError("start must hold one (x, y) pair per movable")
        eng = self.search._engine
        n2 = 2 * self.search.num_objects
        pos = torch.zeros((1, self.npad, 2), dtype=torch.int8, device=self.device)
        host = np.zeros((1, self.npad, 2), np.int8)
        out = ctypes.create_string_buffer(64)
        view = memoryview(out).cast("b")
        plan: List[int] = []
        limit = None
        while True:
            host[0, :len(state)] = np.asarray(state, np.int64).astype(np.int8)
            pos.copy_(torch.from_numpy(host))
            q = self.query(None, pos)
            cost, action = int(q.cost.cpu()[0]), int(q.action.cpu()[0])
            if cost < 0:
                return None
            if cost == 0:
                return plan
            if limit is None:
                limit = cost * 4096
            if action < 0 or len(plan) >= limit:
                raise RuntimeError("the table gives no action from a live state (an internal error)")
            _capi.check(_capi.lib.pw_next_state(eng.handle, self.puzzle_index, bytes(host[0, :len(state)].tobytes()), action,
                                                out, None))
            state = tuple(zip(view[0:n2:2], view[1:n2:2]))
            plan.append(action)
            if self.puzzle.is_goal_state(state):  # (a goal row may carry a movable out of its grid: no node, and the goal)
                return plan

    # ---- drawing from the table (pw_push_search_table_index / _sample / _plans / _emit) --------------------------
    def _entry(self, what: str):
        """(function, handle, stream) of ``_sample_call``'s launch; the first sample builds the cost index (the call is
        idempotent: with the index in place it launches nothing)."""
        h = self._handle()
        h.table_index()
        return _capi.lib.pw_push_search_table_sample, h.handle, h.engine._stream()

    def cost_index(self):
        """``(states_by_cost int32 [num_states], cost_start uint32 [max_cost + 3])`` on the device: the STATES grouped by
        cost-to-go, the dead ends last, in ascending store index inside a bucket; bucket c is
        ``states_by_cost[cost_start[c] : cost_start[c + 1]]``, the dead ends are bucket ``max_cost + 1``.  Built by the first
        call (it allocates and waits once), kept until the search is restarted."""
        h = self._handle()
        h.table_index()
        states = torch.empty((self.num_states,), dtype=torch.int32, device=self.device)
        start = torch.empty((self.max_cost + 3,), dtype=torch.uint32, device=self.device)
        h.table_index_read(states, start)
        return states, start

    def sample(self, puzzle_id: Optional[torch.Tensor], pos: torch.Tensor, steps: torch.Tensor,
               terminated: Optional[torch.Tensor] = None, truncated: Optional[torch.Tensor] = None, cost=(1, None),
               mask: Optional[torch.Tensor] = None, seed: int = 0, counter: Optional[torch.Tensor] = None, out=None):
        """``SolutionTable.sample`` over this table's canonical states: one start state per environment, drawn uniformly from
        the states whose cost IN PUSHES lies in ``cost`` (``(lo, hi)`` ints, ``hi`` None: up to ``max_cost``, or two int32
        tensors [n]) and written as a reset would -- ``pos`` gets the state as the search reached it (the agent where the
        push left it), ``steps`` = 0, ``terminated`` = ``truncated`` = 0.  One launch on the current stream, no wait, no
        allocation when ``counter`` and ``out`` are given and the index exists (capturable).  The band is clamped to
        ``0 .. max_cost``; dead ends are never drawn.  Returns ``(state, cost)`` int32 [n] (``out``, filled in place): the
        store index drawn and its cost; -1 / -1 where the table has no solvable state or the band holds no state.  A draw
        is a function of (``seed``, environment, ``counter``) alone: the order inside a cost bucket is the store's.  Masked
        environments and environments of other puzzles keep everything they held, the counter included."""
        return _sample_call(self, True, puzzle_id, pos, steps, terminated, truncated, cost, mask, seed, counter, out)

    def plans(self, index: torch.Tensor, puzzle_id: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None,
              tie: str = "lowest", seed: int = 0, plan_cap: int = 256, out=None) -> PushPlans:
        """A fewest-pushes plan from every state of ``index`` (int32 [n] store indices, as ``query`` returns them) in one launch
        on the current stream, no wait: a ``PushPlans``.  ``tie`` "lowest" takes each state's ``best`` row, "uniform" draws
        among its optimal rows (f(``seed``, item, step)).  ``length`` is the state's cost; ``PLANS_NONE`` -1 for an index
        outside the table, a dead end or an item of another puzzle, ``PLANS_CUT`` -2 for a plan longer than ``plan_cap``
        (nothing else written in both cases).  Masked items keep what ``out`` -- the ``PushPlans`` of an earlier call -- held."""
        return _push_plans_call(self, True, index, puzzle_id, mask, tie, seed, plan_cap, out)

    # (what ``_push_plans_call`` / ``_push_rows_call`` launch)
    def _live(self) -> None:
        self._handle()

    def _plans_launch(self, *args) -> None:
        self._handle().table_plans(*args)

    def _emit_launch(self, *args) -> None:
        self._handle().table_emit(*args)

    def demonstration_rows(self, plans: PushPlans, pos: Optional[torch.Tensor] = None, puzzle_id: Optional[torch.Tensor] = None,
                           mask: Optional[torch.Tensor] = None, rows_cap: Optional[int] = None,
                           offset: Optional[torch.Tensor] = None, out: Optional[PushRows] = None) -> PushRows:
        """Every push of every plan of ``plans`` as one flat row (``pw_push_search_table_emit``, one launch, no flood and no
        step): a ``PushRows``.  Row ``offset[i] + t`` holds push t of item i, the node it is made from, the cost to go
        ``length[i] - t`` and the state the push is made from -- for t = 0 ``pos[i]`` (int8 [n, NP, 2] live states; None: the
        node's stored state), later the store's state of the node with the agent where the push before left it.  ``offset``
        (int64 [n + 1]) defaults to the exclusive scan of the lengths of the items that take part (not masked, of this
        table's puzzle, length > 0).  ``rows_cap`` None sizes the rows from ``offset[n]`` -- the one host wait; rows at or
        beyond a given ``rows_cap`` are dropped and counted in ``dropped``.  ``out``: the ``PushRows`` of an earlier call or
        of another table of the same batch, filled in place (``rows_cap`` defaults to its rows and must not exceed them)."""
        return _push_rows_call(self, True, plans, pos, puzzle_id, mask, rows_cap, offset, out)

    def primitive_plans(self, pos: torch.Tensor, puzzle_id: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None,
                        tie: str = "lowest", seed: int = 0, plan_cap: int = 1024, push_cap: int = 256):
        """A fewest-pushes plan IN PRIMITIVE ACTIONS from every live state of ``pos`` (int8 [n, NP, 2]; ``puzzle_id`` / ``mask``
        as ``query``): ``query``, ``plans`` (at most ``push_cap`` pushes), ``demonstration_rows`` and ``push_rows_to_plans``,
        all on the device with two host waits (the number of rows, the number of actions).  Returns ``(plans uint8 [n,
        plan_cap], plan_len int32 [n], pushes int32 [n])`` as ``replay_plans`` takes them: ``plan_len`` 0 at a goal state, -1
        at a dead end, for a state outside the table, an item of another puzzle, a masked item or a plan of more than
        ``push_cap`` pushes.  Unlike ``optimal_plan`` the walk to every push follows the parent actions of the walk region
        of the state the push is made from (``walk_regions``' maps)."""
        q = self.query(puzzle_id, pos, mask=mask, actions=False)
        n = int(q.index.shape[0])
        own = mask
        if puzzle_id is not None:
            own = self.covers(puzzle_id) if mask is None else self.covers(puzzle_id) & (mask != 0)
        plans = self.plans(q.index, puzzle_id, mask=own, tie=tie, seed=seed, plan_cap=push_cap)
        offset = torch.zeros((n + 1,), dtype=torch.int64, device=self.device)
        torch.cumsum(plans.length.clamp(min=0), 0, out=offset[1:])
        rows = self.demonstration_rows(plans, pos=pos, puzzle_id=puzzle_id, mask=own, offset=offset,
                                       rows_cap=int(offset[n].cpu()))
        ids = torch.full((rows.num_rows,), self.puzzle_index, dtype=torch.int32, device=self.device)
        out, plan_len, pushes = push_rows_to_plans(self.search._engine, ids, rows, offset, plan_cap=plan_cap)
        return out, torch.where(plans.length < 0, torch.full_like(plan_len, -1), plan_len), pushes

    def covers(self, puzzle_id: torch.Tensor) -> torch.Tensor:
        """bool [n] on the device: the items of ``puzzle_id`` this table answers for."""
        return puzzle_id == self.puzzle_index

    def close(self) -> None:
        search = getattr(self, "search", None)
        if search is not None:
            search.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    __del__ = close


# ---- cost-to-go tables over pushes of many small puzzles in one launch (pw_push_solve_batch_*) -------------------
def pack_push_key(canon, state) -> int:
    """The key of a canonical state as ``PushSolutionTableBatch.keys`` holds it: movable j at bits 8 j (x in the low nibble, y in
    the high one), the agent at ``canon``; ``state`` lists the puzzle's movables only, so nothing lies beyond them."""
    key = 0
    for j, (x, y) in enumerate([tuple(canon)] + [tuple(xy) for xy in list(state)[1:]]):
        if j >= 8 or not (0 <= int(x) < 16 and 0 <= int(y) < 16):
            raise ValueError("a key holds at most 8 movables with coordinates in 0 .. 15")
        key |= (int(x) | (int(y) << 4)) << (8 * j)
    return key


class PushSolutionTableBatch:
    """``PushSolutionTable``'s states and rows for MANY small puzzles of one set, built by ONE launch (``pw_push_solve_batch_run``:
    persistent workgroups, the search over canonical states, the rows and the sweeps of an item inside the kernel) and queried
    for a mixed batch by one launch.  The kernel's limits are ``SolutionTableBatch``'s: 16 x 16 cells with the border, 8
    movables; bigger puzzles (status 3) and bigger spaces (status 2) are ``PushSolutionTable``'s.

    Args:
        source: a ``VecPushWorld`` or an ``_capi.Engine``: the tables are of its puzzle set, in its object order.
        puzzles: set indices (item i is puzzle ``puzzles[i]``); None: every puzzle of the set.
        starts: one entry per item, a state (a sequence of (x, y), the agent first) or None for the puzzle's initial state; None:
            every item starts from its initial state.  A start outside its grid gives status 3.
        max_states_each: cap on the canonical states per item (an item also holds at most 32 rows per state of the cap).
        states, rows: entries of the two pools that hold the tables of all items together.  Both None: one summary-only pass
            sizes them, a second pass stores (nothing is left out); 0 / 0: summaries only.

    Device tensors, one entry per item: ``status`` uint8 (0 stored, 2 beyond the cap, 3 not searched, 4 built but a pool was
    full -- summary only, 5 a cost beyond 65 534, 6 internal error), ``summary`` int32 [n, 6] and its columns ``num_states``,
    ``num_rows``, ``num_goals``, ``dead_ends``, ``max_cost`` (-1: no finite cost), ``start_cost`` (-1: the start is a dead end)
    -- valid for status 0 and 4 --, ``state_offset`` / ``row_offset`` int64 (-1: not stored).  ``states_needed`` /
    ``rows_needed``: the pools that store every built table.

    State 0 is the start; the order of a state's rows ((y, x, action) of the push), ``best``, the costs and the row bits are
    fixed.  State numbers inside a layer (hence ``succ``) and the pool offsets depend on the schedule of the launch: everything
    is found by state (``keys(i)`` / ``states(i)`` / ``query``), never by a number across runs.
    Device memory: 24 bytes per entry of the state pool, 8 per row, see ``pw_push_solve_batch_create``."""

    indexed = False  # (a batch without a cost index: ``build_index`` / ``index=True``)

    def __init__(self, source, puzzles: Optional[Sequence[int]] = None, starts=None, max_states_each: int = 1 << 16,
                 states: Optional[int] = None, rows: Optional[int] = None, index: bool = False):
        engine = source if isinstance(source, _capi.Engine) else getattr(source, "engine", None)
        if not isinstance(engine, _capi.Engine):
            raise ValueError("source must be a VecPushWorld or an _capi.Engine")
        self.engine, self.device, self.npad = engine, engine.device, int(engine.np)
        count = len(engine.pset)
        self.puzzles = list(range(count)) if puzzles is None else [int(p) for p in puzzles]
        if not self.puzzles:
            raise ValueError("puzzles must not be empty")
        if min(self.puzzles) < 0 or max(self.puzzles) >= count:
            raise ValueError(f"puzzles must be indices into the set (0 .. {count - 1})")
        if (states is None) != (rows is None):
            raise ValueError("states and rows must both be given or both be None")
        if states is not None and (int(states) < 0 or int(rows) < 0):
            raise ValueError("states and rows must be >= 0 (or None)")
        if int(max_states_each) < 1:
            raise ValueError("max_states_each must be >= 1")
        self.max_states_each = int(max_states_each)
        self.handle = None
        self._ids = None if puzzles is None else torch.as_tensor(np.asarray(self.puzzles, dtype=np.int32)).to(self.device)
        self._starts = None
        if starts is not None:
            starts = list(starts)
            if len(starts) != len(self.puzzles):
                raise ValueError("starts must hold one entry (a state or None) per item")
            headers = np.frombuffer(engine.pset.headers(), dtype=np.uint8).reshape(count, 320)
            host = np.zeros((len(starts), self.npad, 2), dtype=np.int8)
            for i, (pid, start) in enumerate(zip(self.puzzles, starts)):
                n_mov = int(headers[pid, 6])
                if start is None:
                    init = headers[pid, 256:320].view(np.int8).reshape(32, 2)
                    host[i, :min(n_mov, self.npad)] = init[:min(n_mov, self.npad)]
                    continue
                xy = np.asarray(start, dtype=np.int64)
                if xy.shape != (n_mov, 2):
                    raise ValueError(f"starts[{i}] must list the {n_mov} movables of puzzle {pid} as (x, y)")
                if xy.min() < -128 or xy.max() > 127:
                    raise ValueError(f"starts[{i}] holds a coordinate outside -128 .. 127")
                host[i, :n_mov] = xy
            self._starts = torch.as_tensor(host).to(self.device)
        if states is None:
            self._run(0, 0)
            states, rows = self.states_needed, self.rows_needed
            self.close()
        self._run(int(states), int(rows))
        if index:
            self.build_index()

    def _stream(self):
        return self.engine._stream()

    def _run(self, states: int, rows: int) -> None:
        self.indexed, self.max_cost_stored = False, -1
        h = ctypes.c_void_p()
        _capi.check(_capi.lib.pw_push_solve_batch_create(self.engine.handle, int(states), int(rows), ctypes.byref(h)))
        self.handle = h
        n = len(self.puzzles)
        try:
            _capi.check(_capi.lib.pw_push_solve_batch_run(h, _capi._ptr(self._ids), _capi._ptr(self._starts), self.npad, n,
                                                          self.max_states_each, self._stream()))
            self.status = torch.empty((n,), dtype=torch.uint8, device=self.device)
            self.summary = torch.empty((n, 6), dtype=torch.int32, device=self.device)
            self.state_offset = torch.empty((n,), dtype=torch.int64, device=self.device)
            self.row_offset = torch.empty((n,), dtype=torch.int64, device=self.device)
            _capi.check(_capi.lib.pw_push_solve_batch_copy_results(h, _capi._ptr(self.status), _capi._ptr(self.summary),
                                                                   _capi._ptr(self.state_offset), _capi._ptr(self.row_offset),
                                                                   self._stream()))
            totals = (ctypes.c_int64 * 4)()
            _capi.check(_capi.lib.pw_push_solve_batch_totals(h, totals, self._stream()))
        except Exception:
            self.close()
            raise
        self.pool_states, self.pool_rows = int(states), int(rows)
        self.states_needed, self.rows_needed, self.slots_used, self.missing = (int(t) for t in totals)
        self.num_states, self.num_rows, self.num_goals, self.dead_ends, self.max_cost, self.start_cost = self.summary.unbind(1)
        self._counts, self._covered = None, None

    def __len__(self) -> int:
        return len(self.puzzles)

    def _item(self, item: int) -> Tuple[int, int, int]:
        """(item, its states, its rows); ``ValueError`` for an item without a stored table."""
        if self.handle is None:
            raise ValueError("the batch is closed")
        if not 0 <= int(item) < len(self.puzzles):
            raise ValueError("item out of bounds")
        if self._counts is None:
            self._counts = (self.status.cpu().numpy(), self.summary[:, :2].cpu().numpy())
        if self._counts[0][int(item)] != TABLE_BUILT:
            raise ValueError(f"item {int(item)} has no stored table (status {int(self._counts[0][int(item)])})")
        return int(item), int(self._counts[1][int(item), 0]), int(self._counts[1][int(item), 1])

    def _read_states(self, which: int, item: int) -> torch.Tensor:
        item, count, _ = self._item(item)
        shape, dtype = (((count,), torch.int64), ((count + 1,), torch.int64), ((count,), torch.int32),
                        ((count,), torch.int32))[which]
        out = torch.empty(shape, dtype=dtype, device=self.device)
        ptrs = [None, None, None, None]
        ptrs[which] = _capi._ptr(out)
        _capi.check(_capi.lib.pw_push_solve_batch_read_states(self.handle, item, 0, count, *ptrs, self._stream()))
        return out

    def keys(self, item: int) -> torch.Tensor:
        """int64 [count] on the device: the key of every canonical state (movable j at bits 8 j: x | y << 4, the agent at the
        canon of its walk region; ``pack_push_key``)."""
        return self._read_states(0, item)

    def states(self, item: int) -> np.ndarray:
        """int array [count, N, 2] of (x, y) positions, state by state, the agent at ``canon``."""
        keys = self.keys(item).cpu().numpy().astype(np.uint64)
        n_mov = self.engine.pset.headers()[320 * self.puzzles[int(item)] + 6]
        shifts = (np.arange(n_mov, dtype=np.uint64) * np.uint64(8))[None, :]
        byte = (keys[:, None] >> shifts) & np.uint64(0xFF)
        return np.stack([byte & np.uint64(15), byte >> np.uint64(4)], axis=-1).astype(np.int64)

    def offsets(self, item: int) -> torch.Tensor:
        """int64 [count + 1] on the device: the first row of every state, relative to the item's first row."""
        return self._read_states(1, item)

    def costs(self, item: int) -> torch.Tensor:
        """int32 [count] on the device: pushes to go, -1 = dead end."""
        return self._read_states(2, item)

    def best(self, item: int) -> torch.Tensor:
        """int32 [count] on the device: the lowest optimal row of each state (relative to its first), -1 where there is none."""
        return self._read_states(3, item)

    def rows(self, item: int):
        """(succ int32 [R], from int8 [R, 2], action uint8 [R], flags uint8 [R]) of the item's rows, on the device: the state
        (within the item) a row leads to (-1: outside the grid), the push, and bit 0 goal row, bit 1 optimal, bit 2 safe."""
        item, _, n = self._item(item)
        succ = torch.empty((n,), dtype=torch.int32, device=self.device)
        frm = torch.empty((n, 2), dtype=torch.int8, device=self.device)
        action = torch.empty((n,), dtype=torch.uint8, device=self.device)
        flags = torch.empty((n,), dtype=torch.uint8, device=self.device)
        _capi.check(_capi.lib.pw_push_solve_batch_read_rows(self.handle, item, 0, n, _capi._ptr(succ), _capi._ptr(frm),
                                                            _capi._ptr(action), _capi._ptr(flags), self._stream()))
        return succ, frm, action, flags

    def query(self, puzzle_id: torch.Tensor, pos: torch.Tensor, mask: Optional[torch.Tensor] = None, out=None,
              actions: bool = True) -> PushQuery:
        """``PushSolutionTable.query`` for a mixed batch: ONE launch on the current stream, no allocation besides fresh outputs,
        no wait (it can be captured in a graph with ``out`` given).  ``puzzle_id`` int32 [n], ``pos`` int8 [n, NP, 2], ``mask``
        uint8 / bool [n].  Returns a ``PushQuery``; ``index`` is the state within the puzzle's item.  Items whose puzzle has no
        stored table here and masked items keep what ``out`` held.  ``actions=False`` leaves ``action`` and ``walk`` as they are."""
        n = _state_inputs(puzzle_id, pos, mask, self.npad, self.device)
        out = _push_query_outputs(out, n, self.device)
        if self.handle is None:
            raise ValueError("the batch is closed")
        _capi.check(_capi.lib.pw_push_solve_batch_query(self.handle, _capi._ptr(puzzle_id), _capi._ptr(pos), self.npad,
                                                        _capi._ptr(mask), n, _capi._ptr(out.index), _capi._ptr(out.cost),
                                                        _capi._ptr(out.push_from), _capi._ptr(out.push_action),
                                                        _capi._ptr(out.walk) if actions else None,
                                                        _capi._ptr(out.action) if actions else None, self._stream()))
        return out

    # ---- drawing from the batch (pw_push_solve_batch_index / _sample / _plans / _emit) ---------------------------
    def _live(self):
        if getattr(self, "handle", None) is None:
            raise ValueError("the batch is closed")
        return self.handle

    def build_index(self):
        """Builds the cost index of every stored item (``pw_push_solve_batch_index``: it allocates and waits once; a second call
        does nothing) and returns ``self``.  ``indexed`` says it is there; ``max_cost_stored`` is the largest ``max_cost`` over
        the stored items as a host int (-1: none has a finite cost).  ``sample`` needs the index, and ``VecPushWorld``'s
        ``reset_from_push_tables`` / ``optimal_push_demonstrations`` / ``fewest_push_plans`` take indexed batches only."""
        h = self._live()
        _capi.check(_capi.lib.pw_push_solve_batch_index(h, self._stream()))
        if self._counts is None:
            self._counts = (self.status.cpu().numpy(), self.summary[:, :2].cpu().numpy())
        stored = self._counts[0] == TABLE_BUILT
        costs = self.summary[:, 4].cpu().numpy()[stored]
        self.max_cost_stored = int(costs.max()) if costs.size else -1
        self.indexed = True
        return self

    def cost_index(self, item: int):
        """``(states_by_cost int32 [count], cost_start uint32 [max_cost + 3])`` of a stored item, on the device: its STATES
        grouped by cost-to-go, the dead ends last (bucket ``max_cost + 1``), in ascending KEY inside a bucket -- state numbers
        inside a layer are the schedule's, the key is not, so ``keys(item)[states_by_cost]`` is the same in every run.  Builds
        the index when it is missing (``build_index``)."""
        item, count, _ = self._item(item)
        self.build_index()
        states = torch.empty((count,), dtype=torch.int32, device=self.device)
        start = torch.empty((int(self.summary[item, 4].cpu()) + 3,), dtype=torch.uint32, device=self.device)
        _capi.check(_capi.lib.pw_push_solve_batch_index_read(self.handle, item, _capi._ptr(states), _capi._ptr(start),
                                                             self._stream()))
        return states, start

    def _entry(self, what: str):
        """(function, handle, stream) of ``_sample_call``'s launch."""
        return _capi.lib.pw_push_solve_batch_sample, self._live(), self._stream()

    def sample(self, puzzle_id: torch.Tensor, pos: torch.Tensor, steps: torch.Tensor,
               terminated: Optional[torch.Tensor] = None, truncated: Optional[torch.Tensor] = None, cost=(1, None),
               mask: Optional[torch.Tensor] = None, seed: int = 0, counter: Optional[torch.Tensor] = None, out=None):
        """``PushSolutionTable.sample`` for a mixed batch in ONE launch (``pw_push_solve_batch_sample``; capturable with
        ``counter`` and ``out`` given): every environment draws from the stored item of its own puzzle, the band clamped to
        that item's ``0 .. max_cost``.  ``pos`` gets the canonical state (the agent at the canon of its walk region).  Returns
        ``(state, cost)`` int32 [n]: the state within the item, as ``query`` numbers it, and its cost; -1 / -1 where the item
        has no solvable state or the band holds none.  The STATE drawn is a function of (puzzle, start, ``seed``, environment,
        ``counter``) whatever the launch that built the tables; only its number depends on that.  Masked environments and
        environments whose puzzle has no stored table here keep everything they held, the counter included.  Needs the cost
        index (``build_index``): ``ValueError`` without it."""
        return _sample_call(self, False, puzzle_id, pos, steps, terminated, truncated, cost, mask, seed, counter, out)

    def plans(self, index: torch.Tensor, puzzle_id: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None,
              tie: str = "lowest", seed: int = 0, plan_cap: int = 256, out=None) -> PushPlans:
        """``PushSolutionTable.plans`` for a mixed batch in ONE launch (``pw_push_solve_batch_plans``, no index needed):
        ``index`` int32 [n] are states within each item's puzzle (``query``'s ``index``), ``puzzle_id`` int32 [n] is required.
        ``length`` is ``PLANS_NONE`` also for a puzzle without a stored table here."""
        return _push_plans_call(self, False, index, puzzle_id, mask, tie, seed, plan_cap, out)

    def _plans_launch(self, index, puzzle_id, mask, n, tie, seed, plan_from, plan_action, plan_state, plan_cap, plan_len) -> None:
        p = _capi._ptr
        _capi.check(_capi.lib.pw_push_solve_batch_plans(self._live(), p(index), p(puzzle_id), p(mask), int(n), int(tie),
                                                        int(seed) & 0xFFFFFFFFFFFFFFFF, p(plan_from), p(plan_action),
                                                        p(plan_state), int(plan_cap), p(plan_len), self._stream()))

    def demonstration_rows(self, plans: PushPlans, pos: Optional[torch.Tensor] = None, puzzle_id: Optional[torch.Tensor] = None,
                           mask: Optional[torch.Tensor] = None, rows_cap: Optional[int] = None,
                           offset: Optional[torch.Tensor] = None, out: Optional[PushRows] = None) -> PushRows:
        """``PushSolutionTable.demonstration_rows`` for a mixed batch in ONE launch (``pw_push_solve_batch_emit``):
        ``puzzle_id`` int32 [n] is required; ``state`` is numbered within the item; with ``pos`` None row 0 holds the node's
        canonical state.  Items whose puzzle has no stored table here write nothing."""
        return _push_rows_call(self, False, plans, pos, puzzle_id, mask, rows_cap, offset, out)

    def _emit_launch(self, puzzle_id, mask, n, npad, plan_from, plan_action, plan_state, plan_cap, plan_len, pos, offset, rows_cap,
                     row_item, row_t, row_state, row_from, row_action, row_cost, row_pos, dropped) -> None:
        p = _capi._ptr
        _capi.check(_capi.lib.pw_push_solve_batch_emit(self._live(), p(puzzle_id), p(mask), int(n), int(npad), p(plan_from),
                                                       p(plan_action), p(plan_state), int(plan_cap), p(plan_len), p(pos), p(offset),
                                                       int(rows_cap), p(row_item), p(row_t), p(row_state), p(row_from),
                                                       p(row_action), p(row_cost), p(row_pos), p(dropped), self._stream()))

    def covers(self, puzzle_id: torch.Tensor) -> torch.Tensor:
        """bool [n] on the device: the items of ``puzzle_id`` whose puzzle has a stored table here."""
        if self._covered is None:
            has = torch.zeros((len(self.engine.pset),), dtype=torch.bool, device=self.device)
            ids = self._ids if self._ids is not None else torch.arange(len(self.puzzles), device=self.device)
            has[ids[self.status == TABLE_BUILT].long()] = True
            self._covered = has
        pid = puzzle_id.long()
        inside = (pid >= 0) & (pid < self._covered.shape[0])
        return inside & self._covered[pid.clamp(0, self._covered.shape[0] - 1)]

    def close(self) -> None:
        h = getattr(self, "handle", None)
        if h is not None and _capi.lib is not None:
            _capi.lib.pw_push_solve_batch_destroy(h)
        self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    __del__ = close


# ---- pushes unrolled into primitive actions (pw_push_unroll_count / _write / _plans) ----------------------------
PushUnroll = namedtuple("PushUnroll", "length offset actions num_actions")
PushUnroll.__doc__ = """What ``unroll_pushes`` returns: device tensors ``length`` int32 [n] (the primitive actions of item i's push,
-1 for a refused item), ``offset`` int64 [n + 1] (the actions of item i: ``actions[offset[i] : offset[i + 1]]``), ``actions``
uint8 [num_actions], and ``num_actions`` as an int."""


def _unroll_inputs(puzzle_id, push_from, push_action, pos, mask, npad: int, device) -> int:
    """The checks of ``unroll_pushes`` on its device arrays; returns n."""
    n = _walk_inputs(puzzle_id, pos, mask, npad, device)
    if not isinstance(push_from, torch.Tensor) or push_from.dtype != torch.int8 or tuple(push_from.shape) != (n, 2):
        raise ValueError("push_from must be an int8 tensor [n, 2]")
    if not isinstance(push_action, torch.Tensor) or push_action.dtype != torch.uint8 or tuple(push_action.shape) != (n,):
        raise ValueError("push_action must be a uint8 tensor [n]")
    for name, t in (("push_from", push_from), ("push_action", push_action)):
        if t.device != device:
            raise ValueError(f"{name} must live on {device}")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
    return n


def unroll_pushes(engine_or_vec, puzzle_id: torch.Tensor, push_from: torch.Tensor, push_action: torch.Tensor,
                  pos: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None) -> PushUnroll:
    """Every push of a batch as the primitive actions that perform it (``pw_push_unroll_count`` / ``pw_push_unroll_write``) on
    the current stream: item i is the state ``puzzle_id[i]`` / ``pos[i]`` (int8 [n, NP, 2]; None: the initial states) and the
    choice ``push_from[i]`` (int8 [n, 2]) / ``push_action[i]`` (uint8 [n]); its actions are the walk from the agent's position
    to ``push_from`` along the parent actions of its walk region, then the push -- what ``step_push`` executes.  A choice that
    ``step_push`` would refuse (``PUSH_NONE`` included), a masked item, an id outside the set and a movable outside its grid
    give length -1 and no actions.  Count, ONE host wait for the total, then write.  Returns a ``PushUnroll``."""
    engine = engine_or_vec if isinstance(engine_or_vec, _capi.Engine) else getattr(engine_or_vec, "engine", None)
    if not isinstance(engine, _capi.Engine):
        raise ValueError("engine_or_vec must be a VecPushWorld or an _capi.Engine")
    dev, npad = engine.device, int(engine.np)
    n = _unroll_inputs(puzzle_id, push_from, push_action, pos, mask, npad, dev)
    length = torch.empty((n,), dtype=torch.int32, device=dev)
    offset = torch.empty((n + 1,), dtype=torch.int64, device=dev)
    engine.push_unroll_count(puzzle_id, pos, push_from, push_action, mask, length, offset)
    total = int(offset[n].item())  # the one wait: the number of actions
    actions = torch.empty((total,), dtype=torch.uint8, device=dev)
    if total > 0:
        engine.push_unroll_write(puzzle_id, pos, push_from, push_action, mask, offset, total, actions)
    return PushUnroll(length, offset, actions, total)


def push_rows_to_plans(engine_or_vec, puzzle_id_rows: torch.Tensor, rows, item_offset: torch.Tensor, plan_cap: int = 1024):
    """Plans over pushes as plans over primitive actions: ``rows`` is a ``PushRows`` (one row per push, with the state it is
    made from: ``PushSolutionTable.demonstration_rows``), ``puzzle_id_rows`` int32 [T] the puzzle of every row, and the rows
    ``item_offset[j] : item_offset[j + 1]`` (int64 [m + 1]) are the consecutive pushes of plan j.  One ``unroll_pushes`` over the
    rows (its one wait) and one gather launch (``pw_push_unroll_plans``).  Returns ``(plans uint8 [m, plan_cap], plan_len int32
    [m], pushes int32 [m])`` on the device, in exactly the format ``replay_plans`` takes: ``plan_len`` is the number of
    primitive actions (0 for a plan without rows, ``REPLAY_NONE`` -1 for a plan with a row that is no push move of its state;
    a plan longer than ``plan_cap`` keeps its length and its first ``plan_cap`` actions: ``REPLAY_CUT`` downstream);
    ``pushes`` is the number of rows of every plan."""
    engine = engine_or_vec if isinstance(engine_or_vec, _capi.Engine) else getattr(engine_or_vec, "engine", None)
    if not isinstance(engine, _capi.Engine):
        raise ValueError("engine_or_vec must be a VecPushWorld or an _capi.Engine")
    dev, npad = engine.device, int(engine.np)
    if not isinstance(rows, (tuple, list)) or len(rows) != 9 or not isinstance(rows[0], torch.Tensor) or rows[0].dim() != 1:
        raise ValueError("rows must be a PushRows (PushSolutionTable.demonstration_rows)")
    rows = PushRows(*rows)
    T = int(rows.item.shape[0])
    plan_cap = int(plan_cap)
    if not 1 <= plan_cap <= _capi.PLAN_MAX_ACTIONS:
        raise ValueError(f"plan_cap must be in 1 .. {_capi.PLAN_MAX_ACTIONS}")
    if not isinstance(item_offset, torch.Tensor) or item_offset.dtype != torch.int64 or item_offset.dim() != 1 \
            or not 2 <= int(item_offset.shape[0]) <= 1 << 31:
        raise ValueError("item_offset must be an int64 tensor [m + 1], m >= 1")
    _dev_tensor("item_offset", item_offset, torch.int64, tuple(item_offset.shape), dev)
    m = int(item_offset.shape[0]) - 1
    plans = torch.zeros((m, plan_cap), dtype=torch.uint8, device=dev)
    plan_len = torch.zeros((m,), dtype=torch.int32, device=dev)
    pushes = (item_offset[1:] - item_offset[:-1]).to(torch.int32)
    if T == 0:
        if not isinstance(puzzle_id_rows, torch.Tensor) or tuple(puzzle_id_rows.shape) != (0,):
            raise ValueError("puzzle_id_rows must be an int32 tensor [T], one id per row")
        return plans, plan_len, pushes
    if not isinstance(puzzle_id_rows, torch.Tensor) or tuple(puzzle_id_rows.shape) != (T,):
        raise ValueError("puzzle_id_rows must be an int32 tensor [T], one id per row")
    u = unroll_pushes(engine, puzzle_id_rows, rows.push_from, rows.push_action, pos=rows.pos)
    engine.push_unroll_plans(item_offset, u.length, u.offset, u.actions, T, u.num_actions, plans, plan_len)
    return plans, plan_len, pushes


# ---- best-first search over pushes of many puzzles or live states in one launch (pw_push_plan_batch_*) ----------
PUSH_PLAN_BATCH_INFO = _capi.PUSH_PLAN_BATCH_INFO  # the ten PushPlannerInfo values, then the search time on the device in ns
PUSH_PLAN_CUT = -2  # plan_len of a plan with more pushes than push_cap: nothing of it is written

PushPlanQuery = namedtuple("PushPlanQuery", "push_from push_action pushes status")
PushPlanQuery.__doc__ = """What ``PushStatePlanner.plan`` returns, device tensors with one entry per item: ``push_from`` int8 [n, 2]
and ``push_action`` uint8 [n], the first push of the item's plan ((0, 0) / ``PUSH_NONE`` where ``pushes`` <= 0), ``pushes`` int32
[n] the number of pushes of the plan (-1: no plan, 0: the state is a goal state) and ``status`` int64 [n] (``PLAN_STATUS``)."""


def _push_plan_run_args(max_rounds, time_limit, push_cap):
    if max_rounds is not None and int(max_rounds) <= 0:
        raise ValueError("max_rounds must be positive (or None)")
    if time_limit is not None and not float(time_limit) > 0:
        raise ValueError("time_limit must be positive seconds (or None)")
    if int(push_cap) < 0:
        raise ValueError("push_cap must be >= 0")
    return 0 if max_rounds is None else int(max_rounds), 0.0 if time_limit is None else float(time_limit), int(push_cap)


def _push_plan_create_args(batch, max_states, rgd_budget, cost_range):
    if not 1 <= int(batch) <= 64:
        raise ValueError("batch must be in 1 .. 64")
    if not 1 <= int(max_states) <= 1 << 28:
        raise ValueError("max_states must be in 1 .. 2^28")
    if rgd_budget is not None and int(rgd_budget) < 1:
        raise ValueError("rgd_budget must be >= 1 (or None)")
    if cost_range is not None and not 1 <= int(cost_range) <= 65536:
        raise ValueError("cost_range must be in 1 .. 65536 (or None)")
    return int(batch), int(max_states), 0 if rgd_budget is None else int(rgd_budget), 0 if cost_range is None else int(cost_range)


def _push_plan_results(info, plan_len, plan_from, plan_action):
    """``(pushes as [((x, y), action)] or None, PushPlannerInfo, device seconds)`` per item from host arrays."""
    out = []
    for i in range(info.shape[0]):
        pi = PushPlannerInfo(int(v) for v in info[i, :10])
        n = int(plan_len[i])
        pushes = None
        if pi.status == "solved" and 0 <= n <= plan_from.shape[1]:
            pushes = [((int(plan_from[i, t, 0]), int(plan_from[i, t, 1])), int(plan_action[i, t])) for t in range(n)]
        out.append((pushes, pi, float(info[i, 10]) * 1e-9))
    return out


def _push_plans_to_primitive(engine, puzzle_id, plan_len, plan_from, plan_action, plan_pos, plan_cap: int):
    """The push plans of a run as primitive plans in ``replay_plans``' format: one ``unroll_pushes`` over the plans' rows (its
    one wait, plus one for the number of rows) and one gather launch."""
    n, cap = int(plan_len.shape[0]), int(plan_from.shape[1])
    plan_cap = int(plan_cap)
    if not 1 <= plan_cap <= _capi.PLAN_MAX_ACTIONS:
        raise ValueError(f"plan_cap must be in 1 .. {_capi.PLAN_MAX_ACTIONS}")
    dev = plan_len.device
    pushes = plan_len.clamp(min=0)
    item_offset = torch.zeros((n + 1,), dtype=torch.int64, device=dev)
    item_offset[1:] = torch.cumsum(pushes.to(torch.int64), 0)
    plans = torch.zeros((n, plan_cap), dtype=torch.uint8, device=dev)
    out_len = torch.zeros((n,), dtype=torch.int32, device=dev)
    keep = torch.arange(cap, device=dev).view(1, cap) < pushes.view(n, 1)
    T = int(item_offset[n].item())
    if T > 0:
        ids = puzzle_id.view(n, 1).expand(n, cap)[keep].contiguous()
        u = unroll_pushes(engine, ids, plan_from[keep].contiguous(), plan_action[keep].contiguous(), pos=plan_pos[keep].contiguous())
        engine.push_unroll_plans(item_offset, u.length, u.offset, u.actions, T, u.num_actions, plans, out_len)
    out_len = torch.where(plan_len < 0, torch.full_like(out_len, REPLAY_NONE), out_len)
    return plans, out_len, pushes.to(torch.int32)


class PushPlanBatch:
    """Best-first search over pushes (``PushBestFirstSearch``'s semantics) of MANY puzzles in ONE launch
    (``pw_push_plan_batch_*``, K24): persistent workgroups of one wavefront run each puzzle's whole search inside the kernel.
    Item i's ``PushPlannerInfo``, plan, store and links equal ``PushBestFirstSearch(puzzles[i], batch, max_states, rgd_budget)``
    + ``begin()`` + ``run(max_rounds)`` as long as no finite RGD cost reaches ``cost_range``; three statuses are new:
    ``timeout``, ``range`` and ``skipped`` (a puzzle beyond 16 x 16 cells with the border or 8 movables).

    Args:
        puzzles: ``PushWorldPuzzle`` objects (each in its own object order), all on one device.
        batch: K, states popped per round (1 .. 64).
        max_states: states per puzzle; every workgroup owns a slab of that many (see ``pw_push_plan_batch_create``).
        cost_range: finite costs with a bucket (None: 65536)."""

    def __init__(self, puzzles: Sequence[PushWorldPuzzle], batch: int = 1, max_states: int = 1 << 16,
                 rgd_budget: Optional[int] = None, cost_range: Optional[int] = None):
        self.handle = None
        args = _push_plan_create_args(batch, max_states, rgd_budget, cost_range)
        self.puzzles = list(puzzles)
        if not self.puzzles:
            raise ValueError("puzzles must not be empty")
        from .puzzle import default_device_index

        self.batch, self.max_states = args[0], args[1]
        self._pset = _capi.PuzzleSet([p._parsed for p in self.puzzles], default_device_index())
        self._engine = _capi.Engine(self._pset, None, 3, 1, _capi.OBS_U8)
        self.device, self.npad, self.n = self._engine.device, int(self._engine.np), len(self.puzzles)
        self.handle = _capi.PushPlanBatchHandle(self._engine, list(range(self.n)), args[1], args[0], args[2], args[3])
        self._out = None

    def run(self, max_rounds: Optional[int] = None, time_limit: Optional[float] = None, push_cap: int = 256) -> None:
        """Starts the searches (one launch on the current stream; returns at once).  ``max_rounds`` per puzzle (None: no
        limit), ``time_limit`` seconds per puzzle on the device's clock (None: none); plans of more than ``push_cap`` pushes
        are not written (``plan_len`` -2).  ``results`` waits for them."""
        rounds, limit, cap = _push_plan_run_args(max_rounds, time_limit, push_cap)
        if self.handle is None:
            raise ValueError("the batch is closed")
        info = torch.empty((self.n, PUSH_PLAN_BATCH_INFO), dtype=torch.int64, device=self.device)
        plan_len = torch.empty((self.n,), dtype=torch.int32, device=self.device)
        plan_from = torch.zeros((self.n, cap, 2), dtype=torch.int8, device=self.device)
        plan_action = torch.zeros((self.n, cap), dtype=torch.uint8, device=self.device)
        plan_pos = torch.zeros((self.n, cap, self.npad, 2), dtype=torch.int8, device=self.device)
        self.handle.run(rounds, limit, info, plan_len, plan_from, plan_action, plan_pos, cap, self.npad)
        self._out = (info, plan_len, plan_from, plan_action, plan_pos)

    def _last(self):
        if self._out is None:
            raise RuntimeError("run() has not been called")
        return self._out

    def cancel(self) -> None:
        """Stops the searches of every ``run`` so far soon (their status stays ``running``).  Replays of a captured ``run``
        that begin afterwards are not cancelled."""
        if self.handle is None:
            raise ValueError("the batch is closed")
        self.handle.cancel()

    def results(self):
        """``(pushes as [((x, y), action)] or None, PushPlannerInfo, device seconds)`` per puzzle of the last ``run`` (waits
        for it).  A plan of more than ``push_cap`` pushes is None."""
        info, plan_len, plan_from, plan_action, _ = self._last()
        return _push_plan_results(*(t.cpu().numpy() for t in (info, plan_len, plan_from, plan_action)))

    def primitive_plans(self, plan_cap: int = 4096):
        """``(plans uint8 [n, plan_cap], plan_len int32 [n], pushes int32 [n])`` on the device, in ``replay_plans``' format:
        every push plan of the last ``run`` unrolled into primitive actions (``unroll_pushes`` over the states each push is
        made from, then ``pw_push_unroll_plans``).  ``plan_len`` is ``REPLAY_NONE`` for an item without a written plan; a
        plan longer than ``plan_cap`` keeps its length and its first ``plan_cap`` actions."""
        _, plan_len, plan_from, plan_action, plan_pos = self._last()
        ids = torch.arange(self.n, dtype=torch.int32, device=self.device)
        return _push_plans_to_primitive(self._engine, ids, plan_len, plan_from, plan_action, plan_pos, plan_cap)

    def validate(self, plan_cap: int = 4096) -> torch.Tensor:
        """int8 [n] on the device: the ``is_valid_plan`` verdict (``REPLAY_VERDICT``) of every plan of the last ``run``,
        unrolled by ``primitive_plans`` and replayed by one launch (``replay_plans``)."""
        plans, plan_len, _ = self.primitive_plans(plan_cap)
        ids = torch.arange(self.n, dtype=torch.int32, device=self.device)
        return replay_plans(self._engine, ids, plans, plan_len, rows=False).verdict

    def states(self, item: int, first: int = 0, count: Optional[int] = None):
        """(pos int8 [count, NP, 2] the states as reached, canon int8 [count, 2]) of the store of ``item`` of the last ``run``,
        on the device.  A workgroup keeps the store of the last item it ran: ``ValueError`` for an item that a later one
        displaced (runs of more items than workgroups) or that was skipped."""
        count = self._stored(item) - first if count is None else int(count)
        pos = torch.empty((count, self.npad, 2), dtype=torch.int8, device=self.device)
        canon = torch.empty((count, 2), dtype=torch.int8, device=self.device)
        self.handle.read_states(item, first, count, pos, self.npad, canon)
        return pos, canon

    def links(self, item: int, first: int = 0, count: Optional[int] = None):
        """(parent int32, from int8 [count, 2], action uint8, goal uint8) of the store of ``item``, as ``states``; the start
        state has parent -1 and action 0xFF."""
        count = self._stored(item) - first if count is None else int(count)
        parent = torch.empty((count,), dtype=torch.int32, device=self.device)
        frm = torch.empty((count, 2), dtype=torch.int8, device=self.device)
        action = torch.empty((count,), dtype=torch.uint8, device=self.device)
        goal = torch.empty((count,), dtype=torch.uint8, device=self.device)
        self.handle.read_links(item, first, count, parent, frm, action, goal)
        return parent, frm, action, goal

    def _stored(self, item: int) -> int:
        if not 0 <= int(item) < self.n:
            raise ValueError("item out of bounds")
        return int(self._last()[0][int(item), 3].item())

    def close(self) -> None:
        h = getattr(self, "handle", None)
        if h is not None:
            try:  # (a launch in flight on any stream still uses the slabs)
                torch.cuda.synchronize(self.device)
            except Exception:
                pass
            h.close()
        self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    __del__ = close


def solve_many_pushes(puzzles: Sequence[PushWorldPuzzle], batch: int = 1, max_states: int = 1 << 16,
                      time_limit: Optional[float] = None, rgd_budget: Optional[int] = None, cost_range: Optional[int] = None,
                      push_cap: int = 256):
    """The best-first search over pushes of many puzzles in one launch (``PushPlanBatch``): ``(pushes or None,
    PushPlannerInfo, device seconds)`` per puzzle.  Nothing is raised for a puzzle that ends at ``max_states``, ``time_limit``
    or ``cost_range`` or that is beyond the kernel's limits: its ``PushPlannerInfo.status`` says so."""
    with PushPlanBatch(puzzles, batch=batch, max_states=max_states, rgd_budget=rgd_budget, cost_range=cost_range) as pb:
        pb.run(time_limit=time_limit, push_cap=push_cap)
        return pb.results()


class PushStatePlanner:
    """Best-first search over pushes from given states of a puzzle set, MANY in ONE launch
    (``pw_push_plan_batch_run_states``): typically the live states of a ``VecPushWorld`` -- an expert in pushes where no
    table can be exhausted.  Item i's ``PushPlannerInfo`` and push plan equal ``PushBestFirstSearch(puzzle puzzle_id[i], batch,
    max_states, rgd_budget)`` + ``begin(start=pos[i])`` + ``run(max_rounds)`` as long as no finite RGD cost reaches
    ``cost_range``.  Items that are masked out, name a puzzle outside ``puzzles`` or beyond the kernel's limits (16 x 16 cells
    with the border, 8 movables) or hold a movable outside its grid are ``skipped``.

    Args:
        source: a ``VecPushWorld`` or an ``_capi.Engine``: the planner uses its puzzle set (object order, ``NP``).
        puzzles: the set indices to prepare (None: every puzzle of the set); construction builds one RGD table set each.
        batch: K, states popped per round (1 .. 64).
        max_states: states per item; every workgroup owns a slab of that many (see ``pw_push_plan_batch_create``).
        cost_range: finite costs with a bucket (None: 65536)."""

    def __init__(self, source, puzzles: Optional[Sequence[int]] = None, batch: int = 1, max_states: int = 1 << 16,
                 rgd_budget: Optional[int] = None, cost_range: Optional[int] = None):
        self.handle = None
        args = _push_plan_create_args(batch, max_states, rgd_budget, cost_range)
        engine = source if isinstance(source, _capi.Engine) else getattr(source, "engine", None)
        if not isinstance(engine, _capi.Engine):
            raise ValueError("source must be a VecPushWorld or an _capi.Engine")
        self.engine, self.device, self.npad = engine, engine.device, int(engine.np)
        count = len(engine.pset)
        self.puzzles = list(range(count)) if puzzles is None else [int(p) for p in puzzles]
        if not self.puzzles:
            raise ValueError("puzzles must not be empty")
        if min(self.puzzles) < 0 or max(self.puzzles) >= count:
            raise ValueError(f"puzzles must be indices into the set (0 .. {count - 1})")
        self.batch, self.max_states = args[0], args[1]
        self.handle = _capi.PushPlanBatchHandle(engine, self.puzzles, args[1], args[0], args[2], args[3])
        self._out = None

    def plan(self, puzzle_id: torch.Tensor, pos: torch.Tensor, mask: Optional[torch.Tensor] = None,
             max_rounds: Optional[int] = None, time_limit: Optional[float] = None, push_cap: int = 0) -> PushPlanQuery:
        """Starts the searches from ``pos`` (int8 [n, NP, 2], the engine's layout) of puzzles ``puzzle_id`` (int32 [n]), both
        on the device, on the current stream; does not wait.  ``mask`` (uint8 / bool [n]): 0 skips an item.  ``max_rounds``
        per item (None: no limit), ``time_limit`` seconds per item on the device's clock (None: none).  ``push_cap`` > 0 also
        keeps the whole plans of at most that many pushes for ``results`` / ``primitive_plans`` (longer ones: ``pushes`` -2).
        Returns a ``PushPlanQuery``."""
        n = _state_inputs(puzzle_id, pos, mask, self.npad, self.device)
        rounds, limit, cap = _push_plan_run_args(max_rounds, time_limit, push_cap)
        if self.handle is None:
            raise ValueError("the planner is closed")
        dev = self.device
        info = torch.empty((n, PUSH_PLAN_BATCH_INFO), dtype=torch.int64, device=dev)
        plan_len = torch.empty((n,), dtype=torch.int32, device=dev)
        first_from = torch.empty((n, 2), dtype=torch.int8, device=dev)
        first_action = torch.empty((n,), dtype=torch.uint8, device=dev)
        plan_from = plan_action = plan_pos = None
        if cap > 0:
            plan_from = torch.zeros((n, cap, 2), dtype=torch.int8, device=dev)
            plan_action = torch.zeros((n, cap), dtype=torch.uint8, device=dev)
            plan_pos = torch.zeros((n, cap, self.npad, 2), dtype=torch.int8, device=dev)
        if mask is not None and mask.dtype == torch.bool:
            mask = mask.view(torch.uint8)
        self.handle.run_states(puzzle_id, pos, self.npad, mask, n, rounds, limit, info, plan_len, plan_from, plan_action, plan_pos,
                               cap, first_from, first_action)
        # (the inputs stay referenced until the results are read: the launch reads them on the device)
        self._out = (info, plan_len, plan_from, plan_action, plan_pos, puzzle_id, pos, mask)
        return PushPlanQuery(first_from, first_action, plan_len, info[:, 0])

    def _last(self, plans: bool):
        if self._out is None:
            raise RuntimeError("plan() has not been called")
        if plans and self._out[2] is None:
            raise ValueError("the last plan() call kept no plans (push_cap 0)")
        return self._out

    def info(self) -> torch.Tensor:
        """int64 [n, 11] on the device: the ``PushPlannerInfo`` values of every item of the last ``plan``, then device ns."""
        return self._last(False)[0]

    def results(self):
        """``(pushes as [((x, y), action)] or None, PushPlannerInfo, device seconds)`` per item of the last ``plan`` (waits
        for it), as ``PushPlanBatch.results``; needs ``push_cap`` > 0."""
        info, plan_len, plan_from, plan_action = self._last(True)[:4]
        return _push_plan_results(*(t.cpu().numpy() for t in (info, plan_len, plan_from, plan_action)))

    def primitive_plans(self, plan_cap: int = 4096):
        """As ``PushPlanBatch.primitive_plans``, for the items of the last ``plan`` (from that call's start states)."""
        _, plan_len, plan_from, plan_action, plan_pos, puzzle_id = self._last(True)[:6]
        return _push_plans_to_primitive(self.engine, puzzle_id, plan_len, plan_from, plan_action, plan_pos, plan_cap)

    def validate(self, plan_cap: int = 4096) -> torch.Tensor:
        """int8 [n] on the device: the ``is_valid_plan`` verdict of every plan of the last ``plan`` call, replayed from that
        call's start states."""
        plans, plan_len, _ = self.primitive_plans(plan_cap)
        puzzle_id, pos, mask = self._out[5:8]
        return replay_plans(self.engine, puzzle_id, plans, plan_len, pos=pos, mask=mask, rows=False).verdict

    def cancel(self) -> None:
        """Stops the searches of every ``plan`` so far soon (their status stays ``running``).  Replays of a captured ``plan``
        that begin afterwards are not cancelled."""
        if self.handle is None:
            raise ValueError("the planner is closed")
        self.handle.cancel()

    def close(self) -> None:
        h = getattr(self, "handle", None)
        if h is not None:
            try:  # (a launch in flight still uses the slabs)
                torch.cuda.synchronize(self.device)
            except Exception:
                pass
            h.close()
        self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    __del__ = close

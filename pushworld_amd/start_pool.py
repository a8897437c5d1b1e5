"""Start-state pools: curriculum starts inside autoreset, on the device.

A ``StartPool`` is a flat list of start states of the puzzles of one set -- ``pos``, ``puzzle``, ``level`` -- grouped once by
(puzzle, level).  ``pw_start_pool_draw`` gives every (masked) environment a state of its puzzle drawn uniformly from a band of
levels, in ONE launch whatever the number of puzzles or sources; ``pw_start_pool_update_bands`` moves the band of every puzzle
with the success rate of an ``EpisodeStats`` record.  Nothing leaves the GPU and nothing waits; integer arithmetic throughout.

    vec0 = VecPushWorld(puzzles, 1, observation=None)                    # the set the tables are made on
    pool = StartPool.from_tables(vec0, [vec0.solution_tables()])         # level = cost-to-go
    vec = VecPushWorld(puzzles, 65536, max_steps=100, autoreset=True, episode_stats=True, start_pool=pool)
    vec.reset()
    for t in range(steps):
        vec.step(policy(vec.obs))                                        # finished episodes restart `band` steps from the goal
        if t % 64 == 63:
            pool.update_bands(vec.stats)                                 # one launch: the bands follow the learner
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _capi
from .curriculum import EpisodeStats, _engine_of


def group_entries(puzzle: torch.Tensor, level: torch.Tensor, num_puzzles: int):
    """The grouping of a pool's entries by (puzzle, level): ``(order int32 [S], max_level int32 [P], lvl_off int64 [P], start
    uint32 [W])``.  Bucket (p, l) is ``order[start[lvl_off[p] + l] : start[lvl_off[p] + l + 1]]``, in ascending entry index (a
    stable sort on the key); puzzle p owns ``max_level[p] + 2`` words of ``start`` at ``lvl_off[p]``; ``max_level`` is -1 for
    a puzzle without entries.  Torch ops on whatever device the tensors are on; ``ValueError`` for a puzzle outside the set,
    a negative level, no entry at all or 2^31 and more."""
    P = int(num_puzzles)
    if not isinstance(puzzle, torch.Tensor) or not isinstance(level, torch.Tensor) or puzzle.dim() != 1 \
            or puzzle.shape != level.shape or puzzle.dtype != torch.int32 or level.dtype != torch.int32:
        raise ValueError("puzzle and level must be int32 tensors [S]")
    S = int(puzzle.shape[0])
    if S < 1:
        raise ValueError("a start pool needs at least one entry (S = 0)")
    if S >= 1 << 31:
        raise ValueError("a start pool holds fewer than 2^31 entries")
    if P < 1 or int(puzzle.min()) < 0 or int(puzzle.max()) >= P:
        raise ValueError(f"puzzle must hold indices into the set (0 .. {P - 1})")
    if int(level.min()) < 0:
        raise ValueError("level must be >= 0")
    dev = puzzle.device
    pz, lv = puzzle.to(torch.int64), level.to(torch.int64)
    # the largest level of every puzzle: the last entry of the puzzle in (puzzle, level) order (sort, bincount, cumsum, gather)
    by_key = torch.sort(pz * (int(level.max()) + 1) + lv)[1]
    per_puzzle = torch.bincount(pz, minlength=P)
    last = (torch.cumsum(per_puzzle, 0) - 1).clamp(min=0)
    max_level = torch.where(per_puzzle > 0, lv[by_key][last], torch.full((P,), -1, dtype=torch.int64, device=dev))
    words = max_level + 2
    lvl_off = torch.cumsum(words, 0) - words  # exclusive
    word = lvl_off[pz] + lv                   # the word of an entry's bucket: ascending in (puzzle, level)
    order = torch.sort(word, stable=True)[1]
    counts = torch.bincount(word, minlength=int(words.sum()))
    start = torch.cumsum(counts, 0) - counts  # exclusive: the word behind a puzzle's last level holds the end of its entries
    return (order.to(torch.int32), max_level.to(torch.int32), lvl_off,
            start.to(torch.int32).view(torch.uint32))  # (S < 2^31: the int32 bits are the uint32's)


def _as_tensor(x, dtype, device, name):
    if isinstance(x, torch.Tensor):
        if x.dtype.is_floating_point or x.dtype == torch.bool:
            raise ValueError(f"{name} must hold integers")
        return x.to(device=device, dtype=dtype).contiguous()
    arr = np.asarray(x)
    if not np.issubdtype(arr.dtype, np.integer):
        raise ValueError(f"{name} must hold integers")
    return torch.from_numpy(np.ascontiguousarray(arr.astype(np.int64))).to(device=device, dtype=dtype)


def _q16(name: str, x) -> int:
    if isinstance(x, bool) or not isinstance(x, (int, float)) or not 0.0 <= float(x) <= 1.0:
        raise ValueError(f"{name} must be a number in 0 .. 1")
    return int(round(float(x) * 65536.0))


def keep_to_q16(keep_initial) -> int:
    """The Q16 form of ``keep_initial``, the share of draws that keep the state the environment has (1.0 = 65536: always)."""
    return _q16("keep_initial", keep_initial)


def _check_band(band):
    """``band`` of a draw -> ("pool" | "scalar" | "env", lo, hi)."""
    if isinstance(band, str):
        if band != "pool":
            raise ValueError('band must be "pool", a (lo, hi) pair of ints or a pair of int32 tensors [n]')
        return "pool", 0, -1
    if not isinstance(band, (tuple, list)) or len(band) != 2:
        raise ValueError('band must be "pool", a (lo, hi) pair of ints or a pair of int32 tensors [n]')
    lo, hi = band
    if isinstance(lo, torch.Tensor) or isinstance(hi, torch.Tensor):
        return "env", lo, hi
    hi = -1 if hi is None else hi
    for v in (lo, hi):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not -(1 << 31) <= int(v) < 1 << 31:
            raise ValueError('band must be "pool", a (lo, hi) pair of ints or a pair of int32 tensors [n]')
    return "scalar", int(lo), int(hi)


class StartPool:
    """S start states of the P puzzles of an engine's set, on the engine's device, grouped by (puzzle, level).

    Args:
        source: a ``VecPushWorld``, a vector facade or a ``_capi.Engine``: the pool belongs to its puzzle set (P puzzles, its
            ``npad``) and lives on its device.  Any ``VecPushWorld`` over a set of the same size and layout on that device
            takes it (``start_pool=``).
        puzzle: S set indices.
        level: S levels >= 0 -- for states from a table the cost-to-go; whatever orders a caller's own states from easy to hard.
        pos: the states, ``[S, npad, 2]`` in the engine's layout (agent first, zeros beyond a puzzle's movables).

    numpy arrays or tensors.  ``ValueError``: a puzzle outside the set, a negative level, a ``pos`` of another ``npad``, S = 0,
    S >= 2^31.  Device tensors: ``pos`` int8, ``puzzle`` / ``level`` int32 and the grouping ``order``, ``max_level``,
    ``lvl_off``, ``start`` (``group_entries``); ``band`` int32 ``[P, 2]``, the (lo, hi) of every puzzle that a draw with
    ``band="pool"`` reads, initially (1, 1) clamped to the puzzle's levels.  Device memory: S (2 npad + 12) bytes and a few
    words per (puzzle, level)."""

    def __init__(self, source, puzzle, level, pos):
        # (what can be refused without an engine comes first)
        shape = tuple(getattr(pos, "shape", np.shape(pos)))
        if len(shape) != 3 or shape[2] != 2:
            raise ValueError("pos must be [S, npad, 2] (the engine's state layout)")
        S = shape[0]
        if S < 1:
            raise ValueError("a start pool needs at least one entry (S = 0)")
        if S >= 1 << 31:
            raise ValueError("a start pool holds fewer than 2^31 entries")
        if tuple(np.shape(puzzle)) != (S,) or tuple(np.shape(level)) != (S,):
            raise ValueError("puzzle and level must hold one integer per entry of pos")
        self.engine = _engine_of(source)
        self.num_puzzles = P = len(self.engine.pset)
        self.npad = int(self.engine.np)
        self.device = dev = self.engine.device
        if shape[1] != self.npad:
            raise ValueError(f"pos must be [S, {self.npad}, 2]: the engine's npad is {self.npad}, not {shape[1]}")
        self.puzzle = _as_tensor(puzzle, torch.int32, dev, "puzzle")
        self.level = _as_tensor(level, torch.int32, dev, "level")
        self.pos = _as_tensor(pos, torch.int8, dev, "pos")
        self.num_entries = S
        self.order, self.max_level, self.lvl_off, self.start = group_entries(self.puzzle, self.level, P)
        one = torch.ones((P,), dtype=torch.int32, device=dev)
        edge = torch.minimum(one, self.max_level.clamp(min=0))
        self.band = torch.stack([edge, edge], dim=1).contiguous()
        # the snapshot update_bands subtracts and what it reports (allocated here: update_bands allocates nothing)
        self.base = torch.zeros((P, _capi.EPISODE_STATS), dtype=torch.int64, device=dev)
        self.delta = torch.zeros((P,), dtype=torch.int8, device=dev)
        self.stats = None  # the default record of update_bands (VecPushWorld(start_pool=...) sets its own when there is none)
        self.updates = 0

    # ---------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_tables(cls, vec, tables, max_per_level: Optional[int] = None, seed: int = 0) -> "StartPool":
        """A pool of the states of cost-to-go tables: ``tables`` is a mixed list of ``SolutionTable``, ``SolutionTableBatch``,
        ``PushSolutionTable`` and ``PushSolutionTableBatch`` made on ``vec``'s puzzle set, read through their ``states()`` /
        ``costs()``.  The level is the cost-to-go (in pushes for the push tables, whose state is the store's: the agent where
        the search's push left it, at the canon for a batch); dead ends and unknown costs are dropped, items of a batch without
        a stored table are skipped.  ``max_per_level`` keeps at most that many entries per (puzzle, level), chosen on the host
        with ``numpy.random.default_rng(seed)``.  Waits (the tables are read to the host)."""
        from .search import (TABLE_BUILT, TABLE_DEAD_END, PushSolutionTable, PushSolutionTableBatch, SolutionTable,
                             SolutionTableBatch)

        if max_per_level is not None and (isinstance(max_per_level, bool) or not isinstance(max_per_level, int)
                                          or max_per_level < 1):
            raise ValueError("max_per_level must be None or an integer >= 1")
        engine = _engine_of(vec)
        npad = int(engine.np)
        rng = np.random.default_rng(seed)
        puzzles, levels, states = [], [], []

        def add(p, st, cost, dead):
            st, cost = np.asarray(st), np.asarray(cost).astype(np.int64)
            ok = (cost >= 0) & (cost != dead)
            st, cost = st[ok], cost[ok]
            if max_per_level is not None:
                keep = []
                for c in np.unique(cost):
                    rows = np.flatnonzero(cost == c)
                    if rows.size > max_per_level:
                        rows = np.sort(rng.choice(rows, size=max_per_level, replace=False))
                    keep.append(rows)
                keep = np.concatenate(keep) if keep else np.zeros((0,), np.int64)
                keep.sort()
                st, cost = st[keep], cost[keep]
            pos = np.zeros((st.shape[0], npad, 2), np.int8)
            n = min(npad, st.shape[1])
            pos[:, :n] = st[:, :n]
            puzzles.append(np.full((st.shape[0],), p, np.int32)), levels.append(cost.astype(np.int32)), states.append(pos)

        for table in list(tables):
            if isinstance(table, (SolutionTableBatch, PushSolutionTableBatch)):
                if table.engine.pset is not engine.pset:
                    raise ValueError("the tables must be made on this environment's puzzle set")
                status = table.status.cpu().numpy()
                dead = TABLE_DEAD_END if isinstance(table, SolutionTableBatch) else -1
                for item, p in enumerate(table.puzzles):
                    if status[item] == TABLE_BUILT:
                        add(p, table.states(item), table.costs(item).cpu().numpy(), dead)
            elif isinstance(table, SolutionTable):
                if table.search._engine.pset is not engine.pset:
                    raise ValueError("the tables must be made on this environment's puzzle set")
                add(table.puzzle_index, table.states(), table.costs().cpu().numpy(), TABLE_DEAD_END)
            elif isinstance(table, PushSolutionTable):
                if table.search._engine.pset is not engine.pset:
                    raise ValueError("the tables must be made on this environment's puzzle set")
                st = table.states()[0]
                add(table.puzzle_index, st.cpu().numpy() if isinstance(st, torch.Tensor) else st, table.costs().cpu().numpy(), -1)
            else:
                raise ValueError("tables must hold SolutionTable, SolutionTableBatch, PushSolutionTable or "
                                 "PushSolutionTableBatch objects")
        if not puzzles:
            raise ValueError("a start pool needs at least one entry (S = 0)")
        return cls(engine, np.concatenate(puzzles), np.concatenate(levels), np.concatenate(states))

    # ---------------------------------------------------------------------------------------------------------------
    def bucket(self, puzzle: int, level: int) -> np.ndarray:
        """The entries of level ``level`` of puzzle ``puzzle`` (host copy; waits)."""
        ml = int(self.max_level[puzzle])
        if not 0 <= level <= ml:
            return np.zeros((0,), np.int32)
        off = int(self.lvl_off[puzzle]) + level
        a, b = (int(v) for v in self.start.view(torch.int32)[off:off + 2].cpu())
        return self.order[a:b].cpu().numpy()

    @property
    def nbytes(self) -> int:
        """Device bytes of the pool's tensors."""
        return sum(t.numel() * t.element_size() for t in (self.pos, self.puzzle, self.level, self.order, self.max_level,
                                                           self.lvl_off, self.start, self.band, self.base, self.delta))

    def set_band(self, lo, hi) -> None:
        """Sets ``band``: ints for every puzzle, or P of each (``hi`` -1 / None: up to each puzzle's largest level).  In place."""
        hi = -1 if hi is None else hi
        new = torch.empty_like(self.band)
        new[:, 0] = _as_tensor(lo, torch.int32, self.device, "lo")
        new[:, 1] = _as_tensor(hi, torch.int32, self.device, "hi")
        self.band.copy_(new)

    def update_bands(self, stats=None, min_episodes: int = 32, up: float = 0.8, down: float = 0.2, step: int = 1, width: int = 0,
                     hi_min: int = 1, lo_min: int = 1) -> None:
        """One ``pw_start_pool_update_bands`` launch on the current stream (asynchronous): for every puzzle with at least
        ``min_episodes`` ended episodes since its band last moved -- the difference of ``stats`` (an ``EpisodeStats`` or an
        int64 ``[P, 4]`` device tensor; default ``self.stats``) from the pool's own ``base`` snapshot -- ``hi`` grows by
        ``step`` when the success rate is at least ``up``, shrinks by ``step`` (not below ``hi_min``) when it is below
        ``down``, and the window restarts; ``width`` > 0 keeps ``lo = max(lo_min, hi - width + 1)``, 0 leaves ``lo`` alone.
        ``self.delta`` (int8 ``[P]``) holds how every ``hi`` moved (+1 / -1 / 0)."""
        up_q16, down_q16 = _q16("up", up), _q16("down", down)
        stats = self.stats if stats is None else stats
        block = stats.tensor if isinstance(stats, EpisodeStats) else stats
        if block is None:
            raise ValueError("StartPool.update_bands needs statistics (an EpisodeStats or an int64 [P, 4] tensor)")
        self.engine.start_pool_update_bands(self.max_level, block, self.base, self.band, self.delta, min_episodes, up_q16,
                                            down_q16, step, width, hi_min, lo_min)
        self.updates += 1

    def draw(self, puzzle_id, pos, steps, terminated=None, truncated=None, band="pool", mask=None, seed: int = 0, counter=None,
             keep_initial: float = 0.0, out=None):
        """One ``pw_start_pool_draw`` launch on the current stream, no wait: every (masked) environment whose puzzle has
        entries starts from an entry drawn uniformly among those of its puzzle with a level in the band -- ``pos`` is
        overwritten, ``steps`` and the flags are cleared.  ``band``: "pool" (this pool's ``band`` tensor, per puzzle), ``(lo,
        hi)`` ints for everybody (``hi`` None or -1: up to each puzzle's largest level) or two int32 tensors [n], a band per
        environment; it is clamped to the puzzle's levels.  ``keep_initial``: the share of draws that leave the environment
        in the state it has.  ``counter`` (uint32 bits [n], advanced by the call; default zeros): a draw is a function of
        (seed, environment, count).  Returns ``(entry, level)`` int32 [n] (``out``: the pair of an earlier call) -- -1 / -1
        where nothing was drawn; environments outside ``mask`` keep what ``out`` held."""
        from .search import _dev_tensor, _pos_inputs

        kind, lo, hi = _check_band(band)
        keep_q16 = keep_to_q16(keep_initial)
        n = _pos_inputs(puzzle_id, pos, mask, self.npad, self.device, False)
        _dev_tensor("steps", steps, torch.int32, (n,), self.device)
        _dev_tensor("terminated", terminated, (torch.uint8, torch.bool), (n,), self.device, optional=True)
        _dev_tensor("truncated", truncated, (torch.uint8, torch.bool), (n,), self.device, optional=True)
        lo_n = hi_n = None
        if kind == "env":
            lo_n = _dev_tensor("band: lo", lo, torch.int32, (n,), self.device)
            hi_n = _dev_tensor("band: hi", hi, torch.int32, (n,), self.device)
            lo, hi = 0, -1
        if counter is None:
            counter = torch.zeros((n,), dtype=torch.int32, device=self.device)
        _dev_tensor("counter", counter, (torch.int32, torch.uint32), (n,), self.device)
        if out is None:
            out = (torch.full((n,), -1, dtype=torch.int32, device=self.device),
                   torch.full((n,), -1, dtype=torch.int32, device=self.device))
        if not isinstance(out, (tuple, list)) or len(out) != 2:
            raise ValueError("out must be the (entry, level) pair of an earlier draw")
        _dev_tensor("out: entry", out[0], torch.int32, (n,), self.device)
        _dev_tensor("out: level", out[1], torch.int32, (n,), self.device)
        u8 = [t if t is None or t.dtype == torch.uint8 else t.view(torch.uint8) for t in (terminated, truncated, mask)]
        self.engine.start_pool_draw(self, puzzle_id, pos, steps, u8[0], u8[1], seed,
                                    counter if counter.dtype == torch.uint32 else counter.view(torch.uint32), out[0], out[1],
                                    mask=u8[2], band=self.band if kind == "pool" else None, lo_n=lo_n, hi_n=hi_n,
                                    keep_q16=keep_q16, lo=lo, hi=hi)
        return tuple(out)


def check_start_options(start_pool, start_band, start_keep_initial, autoreset: bool):
    """``VecPushWorld(start_pool=..., start_band=..., start_keep_initial=...)``: the refusals that need no engine; returns
    ``(kind, lo, hi, keep_q16)`` of the band, or None without a pool."""
    if start_pool is None:
        if not (isinstance(start_band, str) and start_band == "pool") or start_keep_initial != 0.0:
            raise ValueError("start_band and start_keep_initial need a start_pool")
        return None
    if not isinstance(start_pool, StartPool):
        raise ValueError("start_pool must be a start_pool.StartPool")
    if not autoreset:
        raise ValueError("start_pool needs autoreset=True: the pool is drawn from inside the step that resets a finished "
                         "environment (without autoreset, call StartPool.draw or reset_from_tables yourself)")
    kind, lo, hi = _check_band(start_band)
    return kind, lo, hi, keep_to_q16(start_keep_initial)

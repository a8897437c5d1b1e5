"""Statistics per puzzle and adaptive puzzle draws on the device.

``EpisodeStats`` keeps, per puzzle of a set, how many episodes ended, how many of them were solved and how long they were
(``pw_episode_stats``: one small launch behind a step, on the flags that step left).  ``Curriculum`` turns such a record
into sampling weights and their prefix sums (``pw_curriculum_update``), which ``pw_resample_weighted`` draws the next puzzle
of a finished environment from.  Nothing leaves the GPU and nothing waits, except the ``read`` / ``probabilities`` calls
that hand numbers to the host.  Integer arithmetic throughout: every figure is exact.

    vec = VecPushWorld(puzzles, 65536, max_steps=100, autoreset=True, resample=True, curriculum="frontier")
    vec.reset()
    for t in range(steps):
        vec.step(policy(vec.obs))
        if t % 64 == 63:
            vec.curriculum.update()        # one launch: the puzzles at a success rate near 1/2 are drawn most often
    vec.puzzle_stats().success_rate
"""
from __future__ import annotations

from collections import namedtuple
from typing import Optional

import numpy as np
import torch

from . import _capi

# what EpisodeStats.read returns: numpy arrays of one entry per puzzle (NaN where no episode ended)
PuzzleStats = namedtuple("PuzzleStats", "episodes solved steps solved_steps success_rate mean_steps")

MODES = tuple(_capi.CURRICULUM_MODES)


def _engine_of(source):
    """The ``_capi.Engine`` of a ``VecPushWorld`` / vector facade / engine."""
    for _ in range(3):
        if isinstance(source, _capi.Engine):
            return source
        source = getattr(source, "vec", None) or getattr(source, "engine", None)
    raise ValueError("expected a VecPushWorld, a vector environment or a _capi.Engine")


def floor_to_q16(floor: float) -> int:
    """The Q16 form of a weight floor given as a fraction of the uniform weight (1.0 = 65536)."""
    if not isinstance(floor, (int, float)) or isinstance(floor, bool) or not 0.0 <= float(floor) < 65536.0:
        raise ValueError("floor must be a number in 0 .. 65535 (a fraction of the uniform weight)")
    return int(round(float(floor) * 65536.0))


class EpisodeStats:
    """The device block int64 ``[P, 4]`` of ``pw_episode_stats`` -- EPISODES, SOLVED, STEPS, SOLVED_STEPS per puzzle of the
    engine's set -- zeroed at construction.  ``tensor`` is the block itself."""

    def __init__(self, source):
        self.engine = _engine_of(source)
        self.num_puzzles = len(self.engine.pset)
        self.tensor = torch.zeros((self.num_puzzles, _capi.EPISODE_STATS), dtype=torch.int64, device=self.engine.device)

    def add(self, puzzle_id, steps, terminated, truncated) -> None:
        """One ``pw_episode_stats`` launch on the flags a step left (asynchronous)."""
        self.engine.episode_stats(puzzle_id, steps, terminated, truncated, self.tensor)

    def read(self) -> PuzzleStats:
        """Host copies (waits for the stream): int64 arrays ``episodes``, ``solved``, ``steps``, ``solved_steps`` and the
        float64 ``success_rate`` = solved / episodes and ``mean_steps`` = steps / episodes, NaN where no episode ended."""
        return stats_tuple(self.tensor.cpu().numpy())

    def reset(self) -> None:
        self.tensor.zero_()

    def snapshot(self) -> torch.Tensor:
        """A device copy of the block, usable as ``base`` of ``pw_curriculum_update`` (asynchronous)."""
        return self.tensor.clone()


def stats_tuple(block: np.ndarray) -> PuzzleStats:
    ep, so, st, ss = (block[:, k].copy() for k in range(_capi.EPISODE_STATS))
    with np.errstate(divide="ignore", invalid="ignore"):
        rate = np.where(ep > 0, so / np.maximum(ep, 1), np.nan)
        mean = np.where(ep > 0, st / np.maximum(ep, 1), np.nan)
    return PuzzleStats(ep, so, st, ss, rate, mean)


class Curriculum:
    """Sampling weights over the puzzles of a set, made on the device from an ``EpisodeStats`` record.

    Args:
        source: a ``VecPushWorld``, a vector facade or a ``_capi.Engine``; its statistics (``source.stats``) are the default
            record.  The weights belong to the puzzle set, not to the environment: a ``Curriculum`` may be handed to another
            ``VecPushWorld`` over a set of the same size on the same device (``curriculum=``), which then draws from it.
        mode: "uniform"; "failure" -- weight (failures + 1) / (episodes + 2), the puzzles that are failed most; "frontier" --
            weight 4 (solved + 1)(failures + 1) / (episodes + 2)^2, largest where the success rate is 1/2 and for puzzles never
            seen; "given" -- the caller's own uint32 weights (``update(given=...)``).
        floor: lower bound of every weight, as a fraction of the uniform weight: no puzzle is starved.  0 allows weight 0,
            and a puzzle of weight 0 is never drawn.
        window: every ``update`` uses the statistics since the previous ``update`` (the difference from a snapshot taken
            there) instead of the whole record.

    ``weights`` (uint32 ``[P]``, Q16: 65536 = the uniform weight) and ``cdf`` (uint64 ``[P]``, their inclusive prefix sums)
    are device tensors that ``update`` overwrites in place: whatever draws from ``cdf`` sees the new weights from its next
    launch on, with no wait and no copy.  Until the first ``update`` they are zero, which draws uniformly."""

    def __init__(self, source, mode: str = "frontier", floor: float = 0.01, window: bool = False, stats=None):
        if mode not in _capi.CURRICULUM_MODES:
            raise ValueError(f"curriculum mode must be one of {', '.join(MODES)}, not {mode!r}")
        self.floor_q16 = floor_to_q16(floor)
        self.mode = mode
        self.window = bool(window)
        self.engine = _engine_of(source)
        self.stats = stats if stats is not None else getattr(getattr(source, "vec", source), "stats", None)
        self.num_puzzles = P = len(self.engine.pset)
        dev = self.engine.device
        # (made as signed tensors and viewed: the unsigned types have copies and views, little else)
        self.weights = torch.zeros((P,), dtype=torch.int32, device=dev).view(torch.uint32)
        self.cdf = torch.zeros((P,), dtype=torch.int64, device=dev).view(torch.uint64)
        # the snapshot a windowed update subtracts (allocated here: update() allocates nothing and can be captured)
        self._base = torch.zeros((P, _capi.EPISODE_STATS), dtype=torch.int64, device=dev) if self.window else None
        self.updates = 0

    def update(self, stats=None, given=None) -> None:
        """One ``pw_curriculum_update`` launch on the current stream (asynchronous).  ``stats``: an ``EpisodeStats`` or an
        int64 ``[P, 4]`` device tensor; default the record this curriculum was made with.  ``given``: the weights of mode
        "given", a uint32 ``[P]`` device tensor or anything ``numpy.asarray`` turns into P integers in 0 .. 2^32 - 1."""
        stats = self.stats if stats is None else stats
        block = stats.tensor if isinstance(stats, EpisodeStats) else stats
        needs = self.mode in ("failure", "frontier")
        if needs and block is None:
            raise ValueError(f"Curriculum.update: mode {self.mode!r} needs statistics (an EpisodeStats or an int64 [P, 4] tensor)")
        if self.mode == "given":
            if given is None:
                raise ValueError("Curriculum.update: mode 'given' needs the weights (given=...)")
            if not isinstance(given, torch.Tensor):
                arr = np.asarray(given)
                if arr.shape != (self.num_puzzles,) or not np.issubdtype(arr.dtype, np.integer) or (arr < 0).any() \
                        or (arr > 0xFFFFFFFF).any():
                    raise ValueError("Curriculum.update: given must hold one integer weight in 0 .. 2^32 - 1 per puzzle")
                given = torch.from_numpy(arr.astype(np.uint32)).to(self.engine.device)
        elif given is not None:
            raise ValueError("Curriculum.update: given weights belong to mode 'given'")
        windowed = self.window and needs
        self.engine.curriculum_update(self.mode, block if needs else None, self.cdf, weights=self.weights,
                                      base=self._base if windowed else None, given=given, floor_q16=self.floor_q16)
        if windowed:
            self._base.copy_(block)  # (stream ordered behind the launch that read the old snapshot)
        self.updates += 1

    def probabilities(self) -> np.ndarray:
        """float64 ``[P]``: the probability of every puzzle under the current weights (waits for the stream); uniform while
        every weight is zero."""
        w = self.weights.cpu().numpy().astype(np.float64)
        total = w.sum()
        return w / total if total > 0 else np.full(self.num_puzzles, 1.0 / self.num_puzzles)


def make_curriculum(vec, curriculum) -> Optional[Curriculum]:
    """``VecPushWorld(curriculum=...)``: a mode name becomes a ``Curriculum`` on ``vec``; a ``Curriculum`` is checked
    against ``vec``'s set and device, and takes ``vec``'s statistics as its record when it has none."""
    if curriculum is None:
        return None
    if isinstance(curriculum, str):
        return Curriculum(vec, mode=curriculum)
    if curriculum.num_puzzles != vec.num_puzzles or curriculum.cdf.device != vec.device:
        raise ValueError(f"the curriculum covers {curriculum.num_puzzles} puzzles on {curriculum.cdf.device}, "
                         f"this environment {vec.num_puzzles} on {vec.device}")
    if curriculum.stats is None:
        curriculum.stats = vec.stats
    return curriculum

"""Batched PushWorld environments on one MI355X.

``VecPushWorld`` is the batched form of the reference's ``PushWorldEnv.step/reset``
(python3/src/pushworld/gym_env.py:150-226): B independent environments, each bound to one
puzzle of a pool, stepped by one kernel launch (+ one render launch).  All state lives in
HBM as torch tensors; nothing is copied to the host per step.

Semantics per environment are exactly the reference's: no implicit reset after
termination (trap T9) unless ``autoreset=True`` (next-step autoreset, gymnasium's vector
convention: the call after a finished episode resets that environment and returns reward 0).
"""
from __future__ import annotations

from collections import namedtuple
from typing import Optional, Sequence, Union

import numpy as np
import torch

from . import _capi
from .puzzle import DEFAULT_BORDER_WIDTH, DEFAULT_PIXELS_PER_CELL, PushWorldPuzzle, default_device_index

# what VecPushWorld.step_push_mask returns
PushStep = namedtuple("PushStep", "obs reward terminated truncated moves status mask num_pushes")


class VecPushWorld:
    """B environments over a pool of puzzles.

    Args:
        puzzles: sequence of ``PushWorldPuzzle`` objects or ``.pwp`` paths (the pool), or a
            ``_capi.PuzzleSet`` (e.g. ``PuzzleSet.load(path, device)`` of a packed pool file).
        num_envs: B.
        puzzle_ids: int array [B] of pool indices (default: ``i % len(puzzles)``).  Grouping
            equal ids together keeps a workgroup's puzzle tables hot in L1/L2.
        max_steps: truncation limit (gym_env.py:223) or None.
        observation: "uint8", "float32", "cells" or None (state only, no render kernel).  "cells": the compact
            cell-grid observation (``PushWorldPuzzle.cells``), ``obs`` is a contiguous uint8 tensor
            [B, 3, Hc, Wc] kept current by ``pw_step_cells`` / ``pw_render_cells``; ``incremental`` and ``tune`` /
            ``tune_allocations`` do not apply to it and are refused, ``fused`` is ignored (a step is always the step
            launch followed by the cells launch).
        pad_cells: (height, width) of the observation frame in cells; default = pool maximum
            (gym_env.py:80-82).
        autoreset: next-step autoreset inside the step kernel.
        fused: one ``pw_step_render`` call per step (default: the step kernel hands its page records to the
            page-ordered render, no pre-pass) instead of ``pw_step`` + ``pw_render``.
        incremental: keep the observation buffer up to date with ``pw_step_render_delta``: a step
            rewrites only the pixel rows swept by the objects that moved (the buffer persists between
            steps, so everything else is already right).  Same observations, a fraction of the HBM
            writes; uint8 / pixels_per_cell 3 only (other settings fall back to the full render).
        resample: draw a new puzzle for every new episode ON THE DEVICE (``pw_resample``), the batched
            form of ``random.choice(self._puzzles)`` in gym_env.py:172.  ``True`` = uniform over the
            pool; a sequence of pool indices = sampling table (repeat an index to weight it).
            Draws happen in ``reset`` (all / masked environments) and, with ``autoreset``, at the
            start of the ``step`` that resets a finished environment.
        seed: seed of the counter-based draw: puzzle = f(seed, environment index, episode number).
        tune: auto-tune the launch configuration of the page-ordered render kernel on this environment's own
            observation buffer (``pw_engine_tune_render``, a few dozen extra render launches in the constructor).
            Default: on for observation buffers of 256 MB and more, where the choice is worth 5-15 %.
        tune_allocations: with ``tune``: the observation buffer is allocated BY THE LIBRARY (``pw_obs_alloc_tuned``:
            physical chunks mapped with the HIP virtual-memory API) from up to this many candidate allocations
            (default: up to 32, within a third of the device memory: 25 for the C3 batch).  What the HBM-write-bound render reaches
            on a buffer follows the buffer's physical backing -- two classes, 7-10 % apart, per allocation
             -- so the library takes a quick look (~10 ms) at one candidate after the other, all
            alive at once, keeps the first of the fast class, releases the others to the DEVICE and tunes on the kept one (nothing stays behind in
            torch's caching allocator).  ``self.obs`` is bound once, in the constructor.  0: a plain torch buffer,
            tuned in place.
        bind: ``pw_batch_bind`` the puzzle assignment at every ``reset`` (and behind every device-side ``resample``): puzzles played by
            at least 48 environments of the batch are stepped one lane per environment with their push tables in LDS instead of by
            lane groups walking the tables through the caches.  Default (None): on, except for ``incremental`` and ``resample`` (a
            binding is rebuilt behind every ``pw_resample``); a set of 8 x 8 puzzles keeps its whole-grid boards unless the segments
            hold every environment.  Same results either way.
        engine_options: ``pw_engine_set_option`` settings (``_capi.OPTIONS``), e.g. ``{"step_kernel": "lane"}`` --
            kernel selection for tests and A/B runs; results never depend on them.
        episode_stats: keep statistics per puzzle on the device (``curriculum.EpisodeStats``): one
            ``pw_episode_stats`` launch follows the step launch of ``step`` / ``step_push`` / ``step_push_mask`` and counts
            the episodes that step ended -- ``self.stats``, read with ``puzzle_stats()``.  Needs ``autoreset`` (without it a
            finished environment keeps its flags and would be counted by every call); ``rollout`` and ``mailbox`` are refused while it is on: their steps cannot be observed.
        curriculum: draw the puzzle of every new episode by weights made from those statistics
            (``pw_resample_weighted``) instead of uniformly: a mode name ("uniform", "failure", "frontier", "given") or a
            ``curriculum.Curriculum``.  Implies ``episode_stats``, needs ``resample=True``.  ``self.curriculum.update()``
            refreshes the weights (one launch, no wait); until the first update the draw is uniform.
        start_pool: a ``start_pool.StartPool``: every new episode starts from a state of its puzzle drawn on the
            device from the pool -- in ``reset`` (all / masked environments, behind the initial states) and inside autoreset:
            ``step`` / ``step_push`` / ``step_push_mask`` become [resample] -> ``pw_start_pool_arm`` -> the step launch (state
            only) -> ``pw_start_pool_draw`` for the environments that step reset -> [statistics] -> render.  The fused
            ``pw_step_render`` and ``pw_step_render_delta`` are NOT taken on this path (``fused`` and ``incremental`` are
            ignored): the draw has to come between the step and the render, which is ``pw_render_retained`` -- a retained
            buffer still gets only its changed pages, behind a record pre-pass that the fused call does not need.  With ``resample`` a finished environment draws from the pool of its NEW puzzle.  Needs ``autoreset``; the
            pool must be of a set of this size and state layout on this device.  Environments whose puzzle has no entry (or
            none in the band) start from the initial state.  ``start_entry`` / ``start_level`` (int32 [B]) hold the pool
            entry and the level every environment started from (-1 / -1: the initial state), ``start_draws`` counts the draws
            per environment -- a draw is a function of (seed, environment, count), ``reset(seed=...)`` restarts the counts.
            ``rollout`` and ``mailbox`` are refused while a pool is set.
        start_band: "pool" (the pool's own ``band`` tensor, (lo, hi) per puzzle: ``set_band`` / ``update_bands`` move it
            without touching this object), ``(lo, hi)`` ints (``hi`` None: up to each puzzle's largest level) or two int32
            device tensors [B], read by every draw.
        start_keep_initial: the share of new episodes that start from the puzzle's initial state all the same.
        changed_rows: where the library turns ``obs_changed_pages`` on by itself (its own buffer, neither ``obs_padding_once`` nor
            ``obs_changed_pages`` given), a step rewrites only the changed pixel rows of every environment
            (``Engine.obs_changed_rows``) instead of the changed pages.  False: the changed pages.  Same observations.
    """

    # statistics per puzzle and the weighted draw (K25): off unless the constructor was asked for them
    stats = None
    curriculum = None
    _call_stats = None
    _call_resample_weighted = None
    # start-state pools (K27): off unless the constructor was given one
    start_pool = None
    _call_pool_arm = None
    _call_pool_draw = None
    # cost-to-go guidance (K28): off unless set_guide was called
    guide = None
    _call_guide = None

    def __init__(self, puzzles: Sequence[Union[str, PushWorldPuzzle]], num_envs: int,
                 puzzle_ids: Optional[Sequence[int]] = None, max_steps: Optional[int] = None,
                 border_width: int = DEFAULT_BORDER_WIDTH, pixels_per_cell: int = DEFAULT_PIXELS_PER_CELL,
                 observation: Optional[str] = "float32", pad_cells=None, device: Optional[int] = None,
                 autoreset: bool = False, fused: bool = True, resample=False, seed: int = 0,
                 incremental: bool = False, engine_options: Optional[dict] = None, tune: Optional[bool] = None,
                 tune_allocations: Optional[int] = None, bind: Optional[bool] = None, episode_stats: bool = False,
                 curriculum=None, start_pool=None, start_band="pool", start_keep_initial: float = 0.0,
                 changed_rows: bool = True):
        # (the new options' refusals come first: nothing has been parsed or allocated yet)
        from .start_pool import check_start_options

        start = check_start_options(start_pool, start_band, start_keep_initial, autoreset)
        if curriculum is not None:
            if isinstance(curriculum, str) and curriculum not in _capi.CURRICULUM_MODES:
                raise ValueError(f"curriculum must be one of {', '.join(_capi.CURRICULUM_MODES)} or a Curriculum, "
                                 f"not {curriculum!r}")
            if resample is not True:
                raise ValueError("curriculum needs resample=True: it replaces the uniform draw of the next puzzle "
                                 "(a sampling table has no place beside it)")
            episode_stats = True
        if episode_stats and not autoreset:
            raise ValueError("episode_stats needs autoreset=True: without it a finished environment keeps its flags and "
                             "would be counted by every step")
        if observation not in ("uint8", "float32", "cells", None):
            raise ValueError("observation must be 'uint8', 'float32', 'cells' or None")
        if observation == "cells" and (incremental or tune or tune_allocations):
            raise ValueError("incremental, tune and tune_allocations apply to the RGB observations, not to observation='cells'")
        dev = default_device_index() if device is None else int(device)
        if isinstance(puzzles, _capi.PuzzleSet):  # e.g. PuzzleSet.load(packed file): no texts, no parsing
            if puzzles.device != dev:
                raise ValueError(f"the puzzle set lives on device {puzzles.device}, not {dev}")
            self.pset = puzzles
            self.puzzles = None
        else:
            self.puzzles = [p if isinstance(p, PushWorldPuzzle) else PushWorldPuzzle(p) for p in puzzles]
            if not self.puzzles:
                raise ValueError("No PushWorld puzzles given")
            self.pset = _capi.PuzzleSet([p._parsed for p in self.puzzles], dev)
        self.num_puzzles = len(self.pset)
        ph, pw = pad_cells if pad_cells is not None else (0, 0)
        dtype = _capi.OBS_F32 if observation == "float32" else _capi.OBS_U8
        # (max_batch: the engine's per-environment scratch is sized here, once -- no step / render call allocates later)
        self.engine = _capi.Engine(self.pset, max_steps, pixels_per_cell, border_width, dtype, ph, pw,
                                   options=engine_options,
                                   max_batch=int(num_envs) if observation in ("uint8", "float32") else 0)
        self.device = self.engine.device
        self.num_envs = int(num_envs)
        self.observation = observation
        self.flags = _capi.STEP_AUTORESET if autoreset else 0
        self.fused = bool(fused)
        self.incremental = bool(incremental)
        self._obs_current = False  # the observation buffer holds the observation of self.pos
        if bind is None:
            # (not with `resample`: every step would rebuild the binding behind its pw_resample -- three small launches)
            # (sets of 8 x 8 puzzles too: the engine takes the segments where they hold EVERY environment -- C2 -- and its whole-grid
            # boards otherwise)
            bind = not self.incremental and self.engine.get_option("bind_puzzles") > 0 \
                and "step_kernel" not in (engine_options or {}) and (resample is False or resample is None)
        self._bind = bool(bind)
        self.bound_info = None  # what the last pw_batch_bind reported (segments, bound environments / puzzles)

        if puzzle_ids is None:
            ids = np.arange(self.num_envs) % self.num_puzzles
        else:
            ids = np.asarray(puzzle_ids)
            if ids.shape != (self.num_envs,) or ids.min() < 0 or ids.max() >= self.num_puzzles:
                raise ValueError("puzzle_ids must be [num_envs] indices into the puzzle pool")
        self.puzzle_id = torch.as_tensor(ids, dtype=torch.int32).to(self.device)
        if "step_block_order" not in (engine_options or {}) and self.num_envs >= 4096 and not resample:
            # A launch lasts as long as its slowest wavefronts: when the expensive puzzles (many movables) sit at the
            # END of the batch (pools sorted by level), let the step kernel start there and the cheap ones fill the tail.
            # (Only for a fixed assignment: with `resample` the puzzles of the batch change every episode.)
            hdr = np.frombuffer(self.pset.headers(), np.uint8)
            assert hdr.size == _capi.PUZZLE_HEADER_BYTES * self.num_puzzles, "PwPuzzleHeader layout changed (csrc/pw_format.h)"
            n_mov = hdr.reshape(-1, _capi.PUZZLE_HEADER_BYTES)[:, _capi.PUZZLE_HEADER_N_OFFSET].astype(np.float64)
            cost = n_mov[np.asarray(ids, dtype=np.int64)]
            q = max(1, self.num_envs // 4)
            if cost[-q:].mean() > 1.15 * cost[:q].mean():
                self.engine.set_option("step_block_order", "reverse")
        st = self.engine.alloc_state(self.num_envs)
        self.pos, self.steps = st["pos"], st["steps"]
        self.reward, self.dgoals = st["reward"], st["dgoals"]
        self.terminated, self.truncated = st["terminated"], st["truncated"]
        self.tuned_config = None  # index returned by the tuner, once it ran
        self.tuned_ms = None      # milliseconds per render launch it measured for that configuration
        self.tuned_candidates_ms = []  # the same for every candidate allocation it tried (tune_allocations)
        self._has_reset = False
        self._obs_storage, self.obs = None, None
        self.obs_owned_by_library = False
        if observation == "cells":
            # (builds the engine's base images now: no later step / render call allocates, so steps are capturable)
            self.obs = torch.empty((self.num_envs,) + self.engine.cells_shape(), dtype=torch.uint8, device=self.device)
        elif observation is not None:
            nbytes = self.num_envs * self.engine.obs_stride
            if tune is None:
                tune = nbytes >= (256 << 20)
            if tune and tune_allocations is None:
                # At most 32 candidates, all alive at once while the choice is made: within a third of the device memory
                # AND within what is free right now (a co-resident model or torch's own allocator must not be pushed into
                # OOM during the constructor); torch.cuda.mem_get_info() was seen returning 0 free bytes on these boxes:
                # then a small count, and the library stops at the candidates there are when memory runs out.
                # (On a box whose allocations are mostly of the slow class -- one in six to thirteen fast,
                # profiles/r03_bench_final7.json: the 14th candidate was the first fast one -- twelve candidates miss one
                # time in three; a candidate costs ~40 ms and goes back to the device.)
                total = torch.cuda.get_device_properties(self.device).total_memory
                try:
                    free = int(torch.cuda.mem_get_info(self.device)[0])
                except Exception:  # noqa: BLE001
                    free = 0
                budget = min(total // 3, free // 2) if free > 0 else 4 * nbytes
                tune_allocations = min(32, max(1, int(budget // nbytes)))
            owned = False
            # a library-owned buffer of a bound batch with a fixed assignment keeps its frame padding: steps render the live pages only
            padding_once = self._bind and not resample and "obs_padding_once" not in (engine_options or {})
            # ... and of those only the pages whose pixel rows a step changed (with neither key given: the library's choice too)
            changed_pages = padding_once and "obs_changed_pages" not in (engine_options or {})
            # ... written as the changed pixel rows of every environment (``Engine.obs_changed_rows``) unless ``changed_rows`` is off
            rows = changed_pages and bool(changed_rows)
            if tune and tune_allocations:
                if padding_once:
                    self.engine.set_option("obs_padding_once", 1)  # (before the tuner: it measures the live launch too)
                if changed_pages:
                    self.engine.set_option("obs_changed_pages", 1)
                if rows:
                    self.engine.obs_changed_rows = True
                # library-owned buffer: candidates are tuned on the initial states (reset() draws them again)
                self.engine.reset(self.puzzle_id, self.pos, self.steps, self.terminated, self.truncated, None)
                try:
                    self._obs_storage, self.obs, self.tuned_config, self.tuned_candidates_ms = \
                        self.engine.alloc_obs_tuned(self.puzzle_id, self.pos, int(tune_allocations))
                    self.tuned_ms = self.engine.get_option("tuned_ns") * 1e-6
                    owned = True
                except (RuntimeError, MemoryError) as exc:
                    # the HIP virtual-memory API refused (old runtime, exotic device): the same kernels on a torch buffer
                    import warnings

                    warnings.warn(f"pw_obs_alloc_tuned failed ({exc}); using a torch-owned observation buffer", RuntimeWarning)
            self.obs_owned_by_library = owned
            if not owned:
                if padding_once:
                    self.engine.set_option("obs_padding_once", 0)
                if changed_pages:
                    self.engine.set_option("obs_changed_pages", 0)
                self.engine.obs_changed_rows = False
                self._obs_storage, self.obs = self.engine.alloc_obs(self.num_envs)
                if tune:
                    self.engine.reset(self.puzzle_id, self.pos, self.steps, self.terminated, self.truncated, None)
                    self.tuned_config = self.engine.tune_render(self.puzzle_id, self.pos, self._obs_storage)
                    self.tuned_ms = self.engine.get_option("tuned_ns") * 1e-6
                    self.tuned_candidates_ms = [self.tuned_ms]

        self.seed = int(seed)
        self.resample = resample is not False and resample is not None
        self.sample_table = None
        if self.resample and resample is not True:
            tab = np.asarray(resample)
            if tab.ndim != 1 or tab.size == 0 or tab.min() < 0 or tab.max() >= self.num_puzzles:
                raise ValueError("resample must be True or a non-empty 1-D sequence of puzzle pool indices")
            self.sample_table = torch.as_tensor(tab, dtype=torch.int32).to(self.device)
        # episode number of every environment (uint32 counter bits in an int32 tensor)
        self.episode = torch.zeros((self.num_envs,), dtype=torch.int32, device=self.device)
        # pre-marshalled step entry points (the state tensors never move: their pointers are converted once)
        self._act_shape = (self.num_envs,)
        self._call_step = self.engine.bind_step(self.puzzle_id, self.pos, self.steps, self.reward, self.dgoals,
                                                self.terminated, self.truncated, self.flags)
        self._call_step_render = self._call_step_delta = None
        if observation == "cells":
            self._call_step_render = self.engine.bind_step_cells(
                self.puzzle_id, self.pos, self.steps, self.reward, self.dgoals, self.terminated, self.truncated,
                self.obs, self.flags)
        elif self.obs is not None:
            self._call_step_render = self.engine.bind_step_render(
                self.puzzle_id, self.pos, self.steps, self.reward, self.dgoals, self.terminated, self.truncated,
                self._obs_storage, self.flags)
            self._call_step_delta = self.engine.bind_step_render(
                self.puzzle_id, self.pos, self.steps, self.reward, self.dgoals, self.terminated, self.truncated,
                self._obs_storage, self.flags, delta=True)
        # statistics per puzzle and the weighted draw (K25): nothing is allocated or launched unless they were asked for
        if episode_stats:
            from .curriculum import EpisodeStats, make_curriculum

            self.stats = EpisodeStats(self.engine)
            self._call_stats = self.engine.bind_episode_stats(self.puzzle_id, self.steps, self.terminated, self.truncated,
                                                              self.stats.tensor)
            self.curriculum = make_curriculum(self, curriculum)
            if self.curriculum is not None:
                self._call_resample_weighted = self.engine.bind_resample_weighted(
                    self.puzzle_id, self.episode, self.curriculum.cdf, self.terminated, self.truncated)
        # start-state pools (K27): nothing is allocated or launched unless a pool was given
        if start is not None:
            self._bind_start_pool(start_pool, start_band, *start)

    def _bind_start_pool(self, pool, band, kind, lo, hi, keep_q16) -> None:
        """The tensors and the ready launch calls of the pool path."""
        B, dev = self.num_envs, self.device
        if pool.num_puzzles != self.num_puzzles or pool.npad != int(self.engine.np) or pool.device != dev:
            raise ValueError(f"the start pool covers {pool.num_puzzles} puzzles with npad {pool.npad} on {pool.device}, "
                             f"this environment {self.num_puzzles} with npad {int(self.engine.np)} on {dev}")
        lo_n = hi_n = None
        if kind == "env":
            from .search import _dev_tensor

            lo_n = _dev_tensor("start_band: lo", lo, torch.int32, (B,), dev)
            hi_n = _dev_tensor("start_band: hi", hi, torch.int32, (B,), dev)
            lo, hi = 0, -1
        self.start_pool = pool
        self.start_seed = self.seed
        self.start_pending = torch.zeros((B,), dtype=torch.uint8, device=dev)
        self.start_entry = torch.full((B,), -1, dtype=torch.int32, device=dev)
        self.start_level = torch.full((B,), -1, dtype=torch.int32, device=dev)
        # (uint32 counter bits over an int32 allocation, like `episode`)
        self.start_draws = torch.zeros((B,), dtype=torch.int32, device=dev).view(torch.uint32)
        self._start_kw = dict(band=pool.band if kind == "pool" else None, lo_n=lo_n, hi_n=hi_n, keep_q16=keep_q16, lo=lo, hi=hi)
        self._call_pool_arm = self.engine.bind_start_pool_arm(self.terminated, self.truncated, self.start_pending)
        self._call_pool_draw = self.engine.bind_start_pool_draw(
            pool, self.puzzle_id, self.pos, self.steps, self.terminated, self.truncated, self.start_draws, self.start_entry,
            self.start_level, mask=self.start_pending, **self._start_kw)
        if pool.stats is None:
            pool.stats = self.stats  # the default record of pool.update_bands

    # --------------------------------------------------------------------------------
    @property
    def num_objects_padded(self) -> int:
        return self.engine.np

    def set_puzzle_ids(self, puzzle_ids) -> None:
        self._obs_current = False
        self.puzzle_id.copy_(torch.as_tensor(np.asarray(puzzle_ids), dtype=torch.int32))
        if self._bind and self.bound_info is not None:
            self.bound_info = self.engine.bind(self.puzzle_id)
        if self.guide is not None:
            self.guide.refresh()

    def reset(self, mask: Optional[torch.Tensor] = None, seed: Optional[int] = None):
        """gym_env.py:150-186 for every (masked) environment; returns the observation tensor.
        ``seed`` (with ``resample``) restarts the puzzle draw sequence: episode numbers return to 0."""
        if mask is not None:
            mask = mask.to(device=self.device, dtype=torch.uint8)
        if seed is not None:
            self.seed = int(seed)
            self.episode.zero_()
        self._reset_states(mask)
        if self.start_pool is not None:
            # the (masked) environments draw their start state, as reset_from_tables does behind the initial states
            if seed is not None:
                self.start_seed = int(seed)
                self.start_draws.view(torch.int32).zero_()
            if mask is None:
                self.start_entry.fill_(-1), self.start_level.fill_(-1)
            else:
                self.start_entry.masked_fill_(mask.bool(), -1), self.start_level.masked_fill_(mask.bool(), -1)
            self.engine.start_pool_draw(self.start_pool, self.puzzle_id, self.pos, self.steps, self.terminated, self.truncated,
                                        self.start_seed, self.start_draws, self.start_entry, self.start_level, mask=mask,
                                        **self._start_kw)
            self._obs_current = False
        if self.guide is not None:
            self.guide.refresh(mask)
        if self.obs is not None:
            self._render()
        return self.obs

    def _reset_states(self, mask: Optional[torch.Tensor]) -> None:
        """``reset`` up to its render: the (masked) environments draw their puzzle and return to its initial state."""
        if self.curriculum is not None:
            self.engine.resample_weighted(self.puzzle_id, self.episode, self.seed, self.curriculum.cdf, terminated=mask)
        elif self.resample:
            self.engine.resample(self.puzzle_id, self.episode, self.seed, terminated=mask, table=self.sample_table)
        self.engine.reset(self.puzzle_id, self.pos, self.steps, self.terminated, self.truncated, mask)
        self._has_reset = True
        if self._bind and (self.bound_info is None or self.resample or mask is None):
            self.bound_info = self.engine.bind(self.puzzle_id)  # (reads the segment count back: later launches have the exact grid)

    def _render(self, retained: bool = False) -> None:
        """``retained`` (the pool path): ``pw_render_retained`` -- a retained buffer gets only the pages that differ from what
        it shows; the same bytes."""
        if self.observation == "cells":
            self.engine.render_cells(self.puzzle_id, self.pos, self.obs)
        else:
            self.engine.render(self.puzzle_id, self.pos, self._obs_storage, retained=retained)
        self._obs_current = True

    def step(self, actions: torch.Tensor):
        """gym_env.py:188-226 for every environment.

        Args:
            actions: uint8 tensor [B] on the device with values in 0..3.

        Returns ``(obs, reward float64[B], terminated uint8[B], truncated uint8[B])`` --
        views of the engine's persistent HBM buffers (overwritten by the next call).
        """
        if not self._has_reset:
            raise RuntimeError("reset() must be called before step() can be called.")
        if actions.dtype != torch.uint8 or actions.device != self.device or actions.shape != self._act_shape \
                or not actions.is_contiguous():
            raise ValueError("actions must be a contiguous uint8 tensor of shape [num_envs] on the engine's device")
        if self._call_resample_weighted is not None:
            self._call_resample_weighted(self.seed)  # ... by the curriculum's weights
        elif self.resample and self.flags & _capi.STEP_AUTORESET:
            # finished environments draw the puzzle their autoreset (inside this step) starts from
            self.engine.resample(self.puzzle_id, self.episode, self.seed, self.terminated, self.truncated,
                                 self.sample_table)
        if self._call_pool_draw is not None:
            # the pool path: the environments this step resets are noted before it and draw their start state behind it; the
            # render follows the draw (never the fused calls; pw_render_retained: a retained buffer gets the pages that differ
            # from what it shows)
            self._call_pool_arm()
            self._call_step(actions.data_ptr())
            self._call_pool_draw(self.start_seed)
            if self._call_guide is not None:
                self._call_guide()  # (K28: a drawn start state already carries its cost)
            if self._call_stats is not None:
                self._call_stats()
            if self.obs is None:
                return None, self.reward, self.terminated, self.truncated
            self._render(retained=True)
            return self.obs, self.reward, self.terminated, self.truncated
        if self.obs is None:
            self._call_step(actions.data_ptr())  # one ctypes call with ready arguments: the launch is host bound
            if self._call_guide is not None:
                self._call_guide()
            if self._call_stats is not None:
                self._call_stats()
            return None, self.reward, self.terminated, self.truncated
        if self.observation == "cells":
            self._call_step_render(actions.data_ptr())  # pw_step_cells
        elif self.incremental and self._obs_current:
            self._call_step_delta(actions.data_ptr())
        elif self.fused:
            self._call_step_render(actions.data_ptr())
        else:
            self._call_step(actions.data_ptr())
            self.engine.render(self.puzzle_id, self.pos, self._obs_storage)
        if self._call_guide is not None:
            self._call_guide()  # (K28, behind the fused render too: the render reads no flags)
        if self._call_stats is not None:
            self._call_stats()  # the episodes this step ended, per puzzle
        self._obs_current = True
        return self.obs, self.reward, self.terminated, self.truncated

    def counters(self) -> dict:
        """Device-side throughput counters of this environment's engine (``pw_counters``): env_steps, episodes_ended,
        episodes_solved, bad_actions since construction (or ``counters_reset``).  Synchronises the stream."""
        return self.engine.counters()

    def counters_reset(self) -> None:
        self.engine.counters_reset()

    def set_guide(self, tables_or_guide, **kw):
        """Cost-to-go guidance inside the step (``guide.ValueGuide``): one ``pw_guide_step`` launch follows the
        step launch (and the pool draw) of ``step`` / ``step_push`` / ``step_push_mask``, in front of the statistics and the
        render -- [resample] -> [arm] -> step -> [draw] -> guide -> [stats] -> render -- and keeps ``self.cost`` (int32 [B]: the
        exact cost-to-go of every environment's state, -1 at a dead end, -2 unknown), ``self.dead`` (uint8 [B]),
        ``self.shaped_reward`` (float64 [B]) and ``self.guide.acts`` / ``optimal_actions`` / ``safe_actions`` current.
        ``tables_or_guide``: one ``solution_tables`` batch (the fused form), a list of tables of one level (the applied form:
        their own queries, then the launch), a ready ``ValueGuide`` made on this environment, or None, which removes the guide.
        ``kw``: ``gamma``, ``scale``, ``dead_cost``, ``end_dead``, ``shaping``, ``counts`` of ``ValueGuide``.  ``end_dead``
        (needs ``autoreset``) truncates an environment that has just entered a dead end: ``pw_episode_stats`` counts it in the
        same call as ended and unsolved, the next call's autoreset (and pool draw) restarts it.  ``reset``,
        ``reset_from_tables``, ``reset_from_push_tables``, ``set_states`` and ``set_puzzle_ids`` refresh the guide for the
        environments they touch; ``rollout`` and ``mailbox`` are refused while a guide is set.  A method and not a constructor
        argument because tables are made on the environment's own engine.  Returns the ``ValueGuide`` (None when removed)."""
        from .guide import ValueGuide

        if tables_or_guide is None:
            if kw:
                raise ValueError("set_guide(None) removes the guide and takes no options")
            self.guide = self._call_guide = None
            return None
        if isinstance(tables_or_guide, ValueGuide):
            if kw:
                raise ValueError("a ready ValueGuide carries its own options")
            if tables_or_guide.vec is not self:
                raise ValueError("the guide must be made on this environment (ValueGuide(vec, tables))")
            guide = tables_or_guide
        else:
            guide = ValueGuide(self, tables_or_guide, **kw)
        self.guide, self._call_guide = guide, guide.step
        if self._has_reset:
            guide.refresh()
        return guide

    @property
    def cost(self):
        """int32 [B]: the guide's cost-to-go of every environment's current state (None without a guide)."""
        return None if self.guide is None else self.guide.cost

    @property
    def dead(self):
        """uint8 [B]: 1 where the guide knows the state to be a dead end (None without a guide)."""
        return None if self.guide is None else self.guide.dead

    @property
    def shaped_reward(self):
        """float64 [B]: the last step's reward plus the guide's potential term (None without a guide or its shaping)."""
        return None if self.guide is None else self.guide.shaped

    def puzzle_stats(self):
        """The statistics per puzzle kept on the device (``episode_stats=True`` / ``curriculum=...``): a
        ``curriculum.PuzzleStats`` of numpy arrays -- ``episodes``, ``solved``, ``steps``, ``solved_steps``, ``success_rate``,
        ``mean_steps``, one entry per puzzle of the pool.  Waits for the stream."""
        if self.stats is None:
            raise RuntimeError("this VecPushWorld keeps no statistics per puzzle (episode_stats=True or curriculum=...)")
        return self.stats.read()

    def rollout(self, actions: torch.Tensor, history: bool = False):
        """T steps in ONE launch without observations (``pw_rollout``): ``actions`` is a uint8 tensor
        [T, B] on the device.  Same semantics as T calls of ``step`` with ``observation=None``.

        Returns ``(reward, terminated, truncated)`` of the last step, or, with ``history=True``,
        the per-step tensors of shape [T, B].
        """
        if self.start_pool is not None:
            raise ValueError("rollout() is not available with a start_pool: the resets inside the launch draw nothing; use step()")
        if self.guide is not None:
            raise RuntimeError("rollout() is not available while a guide is set (set_guide): the steps inside the launch "
                               "cannot be looked up; use step()")
        if self.stats is not None:
            raise RuntimeError("rollout() is not available while statistics per puzzle are kept (episode_stats / curriculum): "
                               "the steps inside the launch cannot be observed; use step()")
        if not self._has_reset:
            raise RuntimeError("reset() must be called before step() can be called.")
        if actions.dtype != torch.uint8 or actions.device != self.device or actions.dim() != 2 \
                or actions.shape[1] != self.num_envs or not actions.is_contiguous():
            raise ValueError("actions must be a contiguous uint8 tensor of shape [T, num_envs] on the engine's device")
        T = actions.shape[0]
        rh = th = uh = None
        if history:
            rh = torch.empty((T, self.num_envs), dtype=torch.float64, device=self.device)
            th = torch.empty((T, self.num_envs), dtype=torch.uint8, device=self.device)
            uh = torch.empty((T, self.num_envs), dtype=torch.uint8, device=self.device)
        self._obs_current = False
        self.engine.rollout(self.puzzle_id, actions, self.pos, self.steps, self.reward, self.dgoals, self.terminated,
                            self.truncated, rh, th, uh, self.flags)
        if history:
            return rh, th, uh
        return self.reward, self.terminated, self.truncated

    def mailbox(self, ring: int = 8, idle_ms: int = 1000):
        """Resident stepping (``pw_mailbox_open``) for hosts that need every step's verdicts before they choose the next actions:
        ``with vec.mailbox() as mb: reward, terminated, truncated = mb.step(actions)`` -- numpy views of pinned host memory, a
        few microseconds per step instead of a launch and a stream synchronisation.  Same semantics as ``step`` with
        ``observation=None`` (this object's ``pos`` / ``steps`` / ``reward`` / ... tensors are kept up to date); state only, up to
        65 536 environments; ``step`` / ``rollout`` / ``reset`` of this object fail while it is open.  Bad
        actions are flagged 0xFF in ``terminated`` / ``truncated`` and counted (``counters()['bad_actions']``) as in ``step``."""
        if self.start_pool is not None:
            raise ValueError("mailbox() is not available with a start_pool: the resident kernel's resets draw nothing; use step()")
        if self.guide is not None:
            raise RuntimeError("mailbox() is not available while a guide is set (set_guide): the resident kernel's steps "
                               "are not looked up; use step()")
        if self.stats is not None:
            raise RuntimeError("mailbox() is not available while statistics per puzzle are kept (episode_stats / curriculum): "
                               "the resident kernel's steps are not counted; use step()")
        if not self._has_reset:
            raise RuntimeError("reset() must be called before step() can be called.")
        self._obs_current = False
        return self.engine.mailbox(self.puzzle_id, self.pos, self.steps, self.reward, self.dgoals, self.terminated, self.truncated,
                                   self.flags, ring, idle_ms)

    def render(self):
        """Re-renders the current states into the observation buffer and returns it."""
        if self.obs is None:
            raise RuntimeError("this VecPushWorld was created with observation=None")
        self._render()
        return self.obs

    def states(self) -> np.ndarray:
        """Host copy of the positions, int8 [B, NP, 2] (entries past a puzzle's movables are 0)."""
        return self.pos.cpu().numpy()

    def planner(self, **kw):
        """A ``search.StatePlanner`` over this batch's puzzle set (its object order and ``NP``); ``kw`` are its arguments
        (``puzzles``, ``heuristic``, ``batch``, ``max_states``, ``action_order``, ``rgd_budget``, ``cost_range``)."""
        from .search import StatePlanner

        return StatePlanner(self, **kw)

    def expert_actions(self, planner, mask: Optional[torch.Tensor] = None, **run_kw) -> torch.Tensor:
        """int8 [B] on the device: the first action of ``planner``'s plan from every environment's current state, -1 where
        there is none (unsolved within the limits, already at the goal, masked out or skipped).  One launch on the current
        stream after whatever was queued there (e.g. ``step``), no wait.  ``run_kw``: ``max_rounds``, ``time_limit`` of
        ``StatePlanner.plan``; ``planner.results()`` reads the whole outcome afterwards."""
        if planner.engine is not self.engine:
            raise ValueError("the planner must be made on this environment (VecPushWorld.planner)")
        if mask is not None:
            mask = mask.to(device=self.device, dtype=torch.uint8)
        return planner.plan(self.puzzle_id, self.pos, mask=mask, plan_cap=0, **run_kw)[3]

    def push_planner(self, **kw):
        """A ``search.PushStatePlanner`` over this batch's puzzle set: the best-first search over pushes from live states;
        ``kw`` are its arguments (``puzzles``, ``batch``, ``max_states``, ``rgd_budget``, ``cost_range``)."""
        from .search import PushStatePlanner

        return PushStatePlanner(self, **kw)

    def planned_pushes(self, planner, mask: Optional[torch.Tensor] = None, **run_kw):
        """A ``search.PushPlanQuery`` of device tensors: ``push_from`` int8 [B, 2] / ``push_action`` uint8 [B], the first push
        of ``planner``'s plan from every environment's current state -- (0, 0) / ``PUSH_NONE`` where there is none (unsolved
        within the limits, already at the goal, masked out or skipped), which ``step_push`` refuses -- ``pushes`` int32 [B]
        (the plan's length, -1 without a plan) and ``status`` int64 [B].  One launch on the current stream after whatever
        was queued there, no wait: ``vec.step_push(q.push_from, q.push_action)`` follows it directly.  ``run_kw``:
        ``max_rounds``, ``time_limit`` and ``push_cap`` of ``PushStatePlanner.plan``.  ``push_cap`` (default 0) > 0 keeps the whole
        plans of at most that many pushes, which ``planner.results()`` / ``primitive_plans()`` / ``validate()`` need;
        ``planner.info()`` reads the counts either way."""
        if planner.engine is not self.engine:
            raise ValueError("the planner must be made on this environment (VecPushWorld.push_planner)")
        if mask is not None:
            mask = mask.to(device=self.device, dtype=torch.uint8)
        return planner.plan(self.puzzle_id, self.pos, mask=mask, **run_kw)

    def demonstrations(self, planner, observation: Optional[str] = "own", include: str = "valid",
                       mask: Optional[torch.Tensor] = None, plan_cap: int = 1024, **run_kw):
        """A flat demonstration dataset from every environment's current state: ``planner`` plans from the live states, the
        plans are replayed on the device (``search.replay_plans``) and every step of every included plan becomes one row --
        ``item`` (the environment), ``t``, ``puzzle_id``, ``pos`` (the state before the action), ``action`` (the expert's),
        ``reward`` and ``done`` as ``step`` would return them, ``next_pos`` -- plus ``obs``, the observation of ``pos``:
        uint8 [T, 3, Hc, Wc] for "cells", [T, H, W, 3] uint8 / float32 for the RGB kind this environment was made with
        (the engine renders one pixel format), None for ``observation=None``.  The default is the environment's own kind.
        ``include``: "valid" keeps the plans that solve their puzzle, "replayed" also the others that were replayed.
        The rows are rendered by ONE ``pw_render`` / ``pw_render_cells`` launch over all T of them.  Everything is queued on
        the current stream behind whatever is there (e.g. ``step``); the call waits once, for the number of rows.  The
        environment's own ``pos``, ``steps`` and ``obs`` are not touched.  ``run_kw``: ``max_rounds``, ``time_limit`` of
        ``StatePlanner.plan``.  Returns a ``search.PlanReplay``."""
        from .search import replay_plans

        if planner.engine is not self.engine:
            raise ValueError("the planner must be made on this environment (VecPushWorld.planner)")
        if observation == "own":
            observation = self.observation
        if observation not in ("uint8", "float32", "cells", None):
            raise ValueError("observation must be 'uint8', 'float32', 'cells' or None")
        own_rgb = "uint8" if self.engine.obs_dtype == torch.uint8 else "float32"
        if observation in ("uint8", "float32") and observation != own_rgb:
            raise ValueError(f"this environment's engine renders {own_rgb} pixels: observation must be '{own_rgb}', 'cells' or None")
        if int(plan_cap) < 1:
            raise ValueError("plan_cap must be >= 1")
        if mask is not None:
            mask = mask.to(device=self.device, dtype=torch.uint8)
        _, plans, plan_len, _ = planner.plan(self.puzzle_id, self.pos, mask=mask, plan_cap=int(plan_cap), **run_kw)
        out = replay_plans(self.engine, self.puzzle_id, plans, plan_len, pos=self.pos, mask=mask, include=include,
                           next_pos=True)
        T = out.num_rows
        if observation == "cells":
            out.obs = torch.empty((T,) + self.engine.cells_shape(), dtype=torch.uint8, device=self.device)
            if T > 0:
                self.engine.render_cells(out.puzzle_id, out.pos, out.obs)
        elif observation is not None:
            storage, out.obs = self.engine.alloc_obs(T)
            if T > 0:
                self.engine.render(out.puzzle_id, out.pos, storage)
        return out

    def walk_regions(self, maps: bool = False):
        """A ``search.WalkRegions`` of every environment's current state: where the agent can walk without displacing anything
        (``region_size``, the canonical position ``canon``, the walk maps on request) and how many push moves are available
        (``offset``).  One launch on the current stream over the live ``puzzle_id`` / ``pos``, no wait, no host round trip."""
        from .search import walk_regions

        return walk_regions(self.engine, self.puzzle_id, self.pos, maps=maps)

    def push_moves(self):
        """A ``search.PushMoves``: every push move available to every environment from its current state (``item`` is the
        environment) -- the push-level action space.  Waits once, for the number of rows."""
        return self.walk_regions().pushes()

    def push_mask(self, expanded: bool = False):
        """The push-level action mask of every environment's current state (``pw_push_mask``), on the device, no wait: uint8
        [B, map_h, map_w] whose entry ``[y, x]`` has bit ``a`` set exactly when ``((x, y), a)`` is a push move (``map_h`` /
        ``map_w``: the set's largest dimensions); with ``expanded`` bool [B, 4, map_h, map_w], the shape of a policy head's
        logits over (direction, cell) that ``step_push(choice=...)`` indexes.  ``self.num_pushes`` (int32 [B]) holds the
        number of push moves of every environment: 0 marks one that ``step_push`` cannot step."""
        if getattr(self, "_push_mask", None) is None:
            self._push_mask = torch.empty((self.num_envs, self.pset.max_height, self.pset.max_width), dtype=torch.uint8,
                                          device=self.device)
            self.num_pushes = torch.empty((self.num_envs,), dtype=torch.int32, device=self.device)
            self._push_bits = torch.tensor([1, 2, 4, 8], dtype=torch.uint8, device=self.device).view(1, 4, 1, 1)
        self.engine.push_mask(self.puzzle_id, self.pos, None, self._push_mask, self.num_pushes)
        if expanded:
            return (self._push_mask.unsqueeze(1) & self._push_bits) != 0
        return self._push_mask

    def step_push(self, push_from: Optional[torch.Tensor] = None, push_action: Optional[torch.Tensor] = None,
                  choice: Optional[torch.Tensor] = None):
        """One macro step per environment in the push-level action space (``pw_step_push``): the agent walks to
        ``push_from`` along the parent actions of its walk region and pushes by ``push_action`` -- bit for bit the loop of
        ``step`` calls it replaces, ended by the first primitive step that terminates or truncates.

        Args: either ``push_from`` (int8 [B, 2], the agent position (x, y) the push starts from) with ``push_action``
            (uint8 [B]) -- e.g. ``q.push_from`` / ``q.push_action`` of ``push_cost_to_go``, or a row of ``push_moves`` -- or
            ``choice``, int64 [B] flat indices into ``[4, map_h, map_w]``, the shape of ``push_mask(expanded=True)``
            (decoded on the device).

        Returns ``(obs, reward float64[B], terminated uint8[B], truncated uint8[B], moves int32[B], status int8[B])``,
        views of persistent device buffers (overwritten by the next call).  ``reward`` is the sequential sum of the
        primitive rewards, ``moves`` the number of primitive steps executed, ``status`` ``PUSH_DONE`` (the push was
        executed), ``PUSH_CUT`` (the macro step ended during the walk: ``max_steps``, or the state was a goal state
        already), ``PUSH_REFUSED`` (the choice is no push move of the state -- anything that is not a row of
        ``push_moves``, ``PUSH_NONE`` included: the environment is left as it was, reward 0, no flag, nothing counted) or
        ``PUSH_RESET`` (``autoreset``: a finished environment was reset as ``step`` resets it; its choice was not read).

        An environment whose state has no push move at all can never be stepped by this call -- every choice is refused.
        There is no policy for that here: watch ``status`` or ``push_mask()`` / ``num_pushes`` and ``reset(mask=...)``."""
        if not self._has_reset:
            raise RuntimeError("reset() must be called before step_push() can be called.")
        push_from, push_action = self._push_choice(push_from, push_action, choice)
        if getattr(self, "push_status", None) is None:
            self.push_moves_taken = torch.zeros((self.num_envs,), dtype=torch.int32, device=self.device)
            self.push_status = torch.zeros((self.num_envs,), dtype=torch.int8, device=self.device)
        if self._call_resample_weighted is not None:
            self._call_resample_weighted(self.seed)  # ... by the curriculum's weights
        elif self.resample and self.flags & _capi.STEP_AUTORESET:
            # finished environments draw the puzzle their autoreset (inside this step) starts from
            self.engine.resample(self.puzzle_id, self.episode, self.seed, self.terminated, self.truncated,
                                 self.sample_table)
        if self._call_pool_draw is not None:
            self._call_pool_arm()  # (K27: the environments this call resets draw their start state behind it)
        self.engine.step_push(self.puzzle_id, push_from, push_action, self.pos, self.steps, self.reward, self.dgoals,
                              self.terminated, self.truncated, self.push_moves_taken, self.push_status, self.flags)
        if self._call_pool_draw is not None:
            self._call_pool_draw(self.start_seed)
        if self._call_guide is not None:
            self._call_guide()
        if self._call_stats is not None:
            self._call_stats()
        self._obs_current = False
        if self.obs is not None:
            self._render(retained=self._call_pool_draw is not None)
        return self.obs, self.reward, self.terminated, self.truncated, self.push_moves_taken, self.push_status

    def _push_choice(self, push_from, push_action, choice):
        """The checked ``(push_from, push_action)`` of ``step_push`` / ``step_push_mask``: given, or decoded from ``choice``."""
        if choice is not None:
            if push_from is not None or push_action is not None:
                raise ValueError("pass either push_from with push_action, or choice")
            if not isinstance(choice, torch.Tensor) or choice.dtype != torch.int64 or choice.device != self.device \
                    or choice.shape != self._act_shape:
                raise ValueError("choice must be an int64 tensor of shape [num_envs] on the engine's device")
            from .search import decode_push_choice

            push_from, push_action = decode_push_choice(choice, self.pset.max_height, self.pset.max_width)
        elif push_from is None or push_action is None:
            raise ValueError("pass either push_from with push_action, or choice")
        if not isinstance(push_from, torch.Tensor) or push_from.dtype != torch.int8 or push_from.device != self.device \
                or tuple(push_from.shape) != (self.num_envs, 2) or not push_from.is_contiguous():
            raise ValueError("push_from must be a contiguous int8 tensor of shape [num_envs, 2] on the engine's device")
        if not isinstance(push_action, torch.Tensor) or push_action.dtype != torch.uint8 or push_action.device != self.device \
                or push_action.shape != self._act_shape or not push_action.is_contiguous():
            raise ValueError("push_action must be a contiguous uint8 tensor of shape [num_envs] on the engine's device")
        return push_from, push_action

    def step_push_mask(self, push_from: Optional[torch.Tensor] = None, push_action: Optional[torch.Tensor] = None,
                       choice: Optional[torch.Tensor] = None, end_stuck: bool = False):
        """``step_push`` and the push mask of the states it leaves, in one launch (``pw_step_push_mask``): what a learner in
        pushes calls once per step.  The arguments, checks and per-environment results are those of ``step_push``; the mask
        is that of ``push_mask()`` for the new states.  The environment keeps a *view* per environment -- mask, number of push
        moves, walk map, region size, and the state they describe -- and the launch uses it: while the view is current, the
        choice is looked up in it and only the state that is left is flooded, one flood per step instead of the two of
        ``step_push`` + ``push_mask``.  A view made stale by anything else that moved the environment (``step``, ``reset``,
        ``set_states``, a new puzzle id) is noticed on the device and rebuilt first.

        ``end_stuck``: an environment that is left without any push move and without a flag gets ``truncated`` set (and
        counts as an ended episode), so that ``autoreset`` restarts it on the next call.

        Returns the named tuple ``PushStep(obs, reward, terminated, truncated, moves, status, mask, num_pushes)``: the six of
        ``step_push``, ``mask`` uint8 [B, map_h, map_w] (bit ``a`` of ``[y, x]``: ``((x, y), a)`` is a push move) and
        ``num_pushes`` int32 [B] -- views of persistent device buffers, no wait.  ``self.push_walk_map`` and
        ``self.push_region_size`` hold the walk maps and region sizes of the same states (``walk_regions(maps=True)``)."""
        if not self._has_reset:
            raise RuntimeError("reset() must be called before step_push_mask() can be called.")
        push_from, push_action = self._push_choice(push_from, push_action, choice)
        self._push_view()
        if getattr(self, "push_status", None) is None:
            self.push_moves_taken = torch.zeros((self.num_envs,), dtype=torch.int32, device=self.device)
            self.push_status = torch.zeros((self.num_envs,), dtype=torch.int8, device=self.device)
        if self._call_resample_weighted is not None:
            self._call_resample_weighted(self.seed)  # ... by the curriculum's weights
        elif self.resample and self.flags & _capi.STEP_AUTORESET:
            # finished environments draw the puzzle their autoreset (inside this step) starts from
            self.engine.resample(self.puzzle_id, self.episode, self.seed, self.terminated, self.truncated,
                                 self.sample_table)
        if self._call_pool_draw is not None:
            self._call_pool_arm()  # (K27: the environments this call resets draw their start state behind it)
        self.engine.step_push_mask(self.puzzle_id, push_from, push_action, self.pos, self.steps, self.reward, self.dgoals,
                                   self.terminated, self.truncated, self.push_moves_taken, self.push_status,
                                   self.push_view_mask, self.push_view_count, self.push_walk_map, self.push_region_size,
                                   self._push_view_pos, self._push_view_id,
                                   self.flags | (_capi.PUSH_END_STUCK if end_stuck else 0))
        if self._call_pool_draw is not None:
            self._call_pool_draw(self.start_seed)
        if self._call_guide is not None:
            self._call_guide()
        if self._call_stats is not None:
            self._call_stats()
        if self._call_pool_draw is not None:
            # the draw made the views of the drawn environments stale: the observe call rebuilds exactly those, so the mask
            # returned describes the drawn states (the stuck rule sees a drawn state at the next call)
            self.observe_pushes()
        self._obs_current = False
        if self.obs is not None:
            self._render(retained=self._call_pool_draw is not None)
        return PushStep(self.obs, self.reward, self.terminated, self.truncated, self.push_moves_taken, self.push_status,
                        self.push_view_mask, self.push_view_count)

    def observe_pushes(self):
        """``(mask, num_pushes)`` of every environment's current state, as ``push_mask()`` gives them, from the views that
        ``step_push_mask`` keeps: the all-``PUSH_NONE`` call without autoreset, which rebuilds the views that are stale and
        steps nothing (no flood at all where every view is current).  ``reward`` and the flags are not touched."""
        if not self._has_reset:
            raise RuntimeError("reset() must be called before observe_pushes() can be called.")
        self._push_view()
        # (reward, dgoals, moves and status are not written: a refusal would overwrite the last step's)
        self.engine.step_push_mask(self.puzzle_id, self._push_none_from, self._push_none_action, self.pos, self.steps, None,
                                   None, self.terminated, self.truncated, None, None, self.push_view_mask,
                                   self.push_view_count, self.push_walk_map, self.push_region_size, self._push_view_pos,
                                   self._push_view_id, 0)
        return self.push_view_mask, self.push_view_count

    def _push_view(self) -> None:
        """The view tensors of ``step_push_mask`` / ``observe_pushes``, allocated on first use with every view invalid."""
        if getattr(self, "_push_view_id", None) is not None:
            return
        B, mh, mw, dev = self.num_envs, self.pset.max_height, self.pset.max_width, self.device
        self.push_view_mask = torch.empty((B, mh, mw), dtype=torch.uint8, device=dev)
        self.push_view_count = torch.empty((B,), dtype=torch.int32, device=dev)
        self.push_walk_map = torch.empty((B, mh, mw), dtype=torch.uint16, device=dev)
        self.push_region_size = torch.empty((B,), dtype=torch.int32, device=dev)
        self._push_view_pos = torch.zeros_like(self.pos)
        self._push_none_from = torch.zeros((B, 2), dtype=torch.int8, device=dev)
        self._push_none_action = torch.full((B,), 0xFF, dtype=torch.uint8, device=dev)
        self._push_view_id = torch.full((B,), -1, dtype=torch.int32, device=dev)

    def solution_table(self, puzzle_index: int, max_states: int = 1 << 22):
        """A ``search.SolutionTable`` -- the exact cost-to-go, optimal actions and dead ends of every reachable state -- of
        puzzle ``puzzle_index`` of this batch's set, in the set's object order: query it with ``puzzle_id`` / ``pos`` as they
        are (``cost_to_go``).  Explores the puzzle's whole reachable space: ``ValueError`` beyond ``max_states``."""
        from .search import SetPuzzle, SolutionTable

        if not 0 <= int(puzzle_index) < self.num_puzzles:
            raise ValueError(f"puzzle_index must be an index into the set (0 .. {self.num_puzzles - 1})")
        return SolutionTable(SetPuzzle(self.pset, int(puzzle_index), engine=self.engine), max_states=max_states)

    def solution_tables(self, puzzles=None, **kw):
        """A ``search.SolutionTableBatch``: the cost-to-go tables of the small puzzles of this batch's set (``puzzles``: set
        indices, None = all), built in one launch and queried in one (``cost_to_go``).  ``kw``: ``max_states_each``, ``rows``."""
        from .search import SolutionTableBatch

        return SolutionTableBatch(self, puzzles, **kw)

    def cost_to_go(self, tables):
        """``(index int32 [B], cost int32 [B], acts uint8 [B])`` on the device for every environment's current state, from
        a list of ``solution_table``s (one ``SolutionTable.query`` launch each on the current stream, no wait) and / or
        ``solution_tables`` batches (one launch for all their puzzles): the cost is -1 at a dead end; environments whose
        puzzle has no table in the list keep -1 / -2 / 0."""
        from .search import COST_UNKNOWN, SolutionTableBatch

        out = (torch.full((self.num_envs,), -1, dtype=torch.int32, device=self.device),
               torch.full((self.num_envs,), COST_UNKNOWN, dtype=torch.int32, device=self.device),
               torch.zeros((self.num_envs,), dtype=torch.uint8, device=self.device))
        for table in tables:
            if isinstance(table, SolutionTableBatch):
                if table.engine is not self.engine:
                    raise ValueError("the tables must be made on this environment (VecPushWorld.solution_tables)")
                table.query(self.puzzle_id, self.pos, out=out)
                continue
            if table.search._engine is not self.engine:
                raise ValueError("the tables must be made on this environment (VecPushWorld.solution_table)")
            table.query(self.puzzle_id, self.pos, out=out)
        return out

    def push_table(self, puzzle_index: int, max_states: int = 1 << 20):
        """A ``search.PushSolutionTable`` -- the exact cost-to-go in pushes, the dead ends and the best push of every canonical
        state -- of puzzle ``puzzle_index`` of this batch's set, in the set's object order: query it with ``puzzle_id`` /
        ``pos`` as they are (``push_cost_to_go``).  Explores the puzzle's whole space of canonical states: ``ValueError``
        beyond ``max_states``."""
        from .search import PushSolutionTable, SetPuzzle

        if not 0 <= int(puzzle_index) < self.num_puzzles:
            raise ValueError(f"puzzle_index must be an index into the set (0 .. {self.num_puzzles - 1})")
        return PushSolutionTable(SetPuzzle(self.pset, int(puzzle_index), engine=self.engine), max_states=max_states)

    def push_tables(self, puzzles=None, **kw):
        """A ``search.PushSolutionTableBatch``: the cost-to-go tables in pushes of the small puzzles of this batch's set
        (``puzzles``: set indices, None = all), built in one launch and queried in one (``push_cost_to_go``).  ``kw``: ``starts``,
        ``max_states_each``, ``states``, ``rows`` and ``index`` -- True builds the cost index (``build_index``) that
        ``reset_from_push_tables``, ``optimal_push_demonstrations`` and ``fewest_push_plans`` ask of a batch."""
        from .search import PushSolutionTableBatch

        return PushSolutionTableBatch(self, puzzles, **kw)

    def push_cost_to_go(self, tables, mask: Optional[torch.Tensor] = None):
        """A ``search.PushQuery`` (index, cost, action, push_from, push_action, walk) on the device for every environment's
        current state, from a list of ``push_table``s (one ``PushSolutionTable.query`` each on the current stream) and / or
        ``push_tables`` batches (one launch for all their puzzles): the cost is in pushes, -1 at a dead end; environments whose
        puzzle has no table in the list keep -1 / -2 / -1 / (0, 0) / 0xFF / -1.  ``q = vec.push_cost_to_go([batch]);
        vec.step_push(q.push_from, q.push_action)`` is an expert in pushes over the whole mix."""
        from .search import PushSolutionTableBatch

        tables = list(tables)
        for table in tables:
            if isinstance(table, PushSolutionTableBatch):
                if table.engine is not self.engine:
                    raise ValueError("the tables must be made on this environment (VecPushWorld.push_tables)")
            elif table.search._engine is not self.engine:
                raise ValueError("the tables must be made on this environment (VecPushWorld.push_table)")
        if mask is not None:
            mask = mask.to(device=self.device, dtype=torch.uint8)
        from .search import _push_query_outputs

        out = _push_query_outputs(None, self.num_envs, self.device)
        for table in tables:
            table.query(self.puzzle_id, self.pos, mask=mask, out=out)
        return out

    def push_expert_actions(self, tables, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """int8 [B] on the device: for every environment the first primitive action of a fewest-pushes plan from its
        current state ("walk to the best push, then push"), -1 where there is none (a goal state, a dead end, a state or a
        puzzle without a table, masked out).  One query per table on the current stream after whatever was queued there
        (e.g. ``step``)."""
        return self.push_cost_to_go(tables, mask=mask).action

    def _own_tables(self, tables) -> list:
        from .search import SolutionTableBatch

        tables = list(tables)
        for table in tables:
            engine = table.engine if isinstance(table, SolutionTableBatch) else table.search._engine
            if engine is not self.engine:
                raise ValueError("the tables must be made on this environment (VecPushWorld.solution_table / solution_tables)")
        return tables

    def reset_from_tables(self, tables, cost=(1, None), mask: Optional[torch.Tensor] = None, seed: Optional[int] = None):
        """``reset(mask)`` with start states drawn from cost-to-go tables (a reverse curriculum): every (masked) environment
        whose puzzle has a table in ``tables`` -- a mixed list of ``solution_table``s and ``solution_tables`` batches, as
        ``cost_to_go`` takes -- starts from a state drawn uniformly among the states of its puzzle with a cost-to-go in
        ``cost`` = ``(lo, hi)`` (``hi`` None: up to each table's own largest cost; two int32 tensors [B]: a band per
        environment).  The band is clamped to each table's costs and dead ends are never drawn, so the default ``(1, None)``
        is "any solvable state that is not solved yet"; grow ``hi`` from 1 for a curriculum.  Environments without a table
        (or whose puzzle has no solvable state) start from the initial state.  One ``pw_reset`` launch, one sample launch
        per table, one render; no wait.  Returns the observation tensor.

        ``self.start_row`` / ``self.start_cost`` (int32 [B]) hold the table row and the cost-to-go every environment started
        from (-1 / -1 without a table); ``self.table_draws`` counts the draws per environment -- a draw is a function of
        (seed, environment, count), ``seed`` restarts the counts.  Autoreset inside ``step`` does not draw from tables: put their
        states into a ``start_pool.StartPool`` (``StartPool.from_tables``) and pass ``start_pool=`` to the constructor, or step
        with ``autoreset=False`` and call ``reset_from_tables(tables, mask=terminated | truncated)``."""
        tables = self._own_tables(tables)
        if mask is not None:
            mask = mask.to(device=self.device, dtype=torch.uint8)
        if getattr(self, "table_draws", None) is None:
            self.table_seed = self.seed
            # (uint32 counter bits over an int32 allocation, like `episode`)
            self.table_draws = torch.zeros((self.num_envs,), dtype=torch.int32, device=self.device).view(torch.uint32)
            self.start_row = torch.full((self.num_envs,), -1, dtype=torch.int32, device=self.device)
            self.start_cost = torch.full((self.num_envs,), -1, dtype=torch.int32, device=self.device)
        if seed is not None:
            self.table_seed = int(seed)
            self.table_draws.view(torch.int32).zero_()
        self._reset_states(mask)
        if mask is None:
            self.start_row.fill_(-1), self.start_cost.fill_(-1)
        else:
            self.start_row.masked_fill_(mask.bool(), -1), self.start_cost.masked_fill_(mask.bool(), -1)
        for table in tables:
            table.sample(self.puzzle_id, self.pos, self.steps, self.terminated, self.truncated, cost=cost, mask=mask,
                         seed=self.table_seed, counter=self.table_draws, out=(self.start_row, self.start_cost))
        if self.guide is not None:
            self.guide.refresh(mask)
        self._obs_current = False
        if self.obs is not None:
            self._render()
        return self.obs

    def optimal_demonstrations(self, tables, tie: str = "lowest", seed: int = 0, observation: Optional[str] = "own",
                               mask: Optional[torch.Tensor] = None, plan_cap: int = 1024):
        """``demonstrations`` with SHORTEST plans read off cost-to-go tables instead of a planner's: from every (unmasked)
        environment's current state, one ``cost_to_go`` over ``tables`` (a mixed list, as there), one plans launch per
        table (``tie`` "lowest": the lowest optimal action at every step, "uniform": drawn among the optimal actions with
        ``seed``), the replay of ``demonstrations`` (every step of every plan becomes one row), one query launch per table
        over the rows and one render launch.  Environments at a dead end, outside every table or with a plan longer than
        ``plan_cap`` contribute no rows.  Returns the same ``search.PlanReplay`` as ``demonstrations`` plus ``cost`` int32
        [T], the cost-to-go of each row's state (it falls by 1 per row to 1), and ``acts`` uint8 [T], its optimal (bits
        0..3) and safe (bits 4..7) actions.  Waits once, for the number of rows."""
        from .search import PLANS_NONE, replay_plans

        tables = self._own_tables(tables)
        if observation == "own":
            observation = self.observation
        if observation not in ("uint8", "float32", "cells", None):
            raise ValueError("observation must be 'uint8', 'float32', 'cells' or None")
        own_rgb = "uint8" if self.engine.obs_dtype == torch.uint8 else "float32"
        if observation in ("uint8", "float32") and observation != own_rgb:
            raise ValueError(f"this environment's engine renders {own_rgb} pixels: observation must be '{own_rgb}', 'cells' or None")
        if tie not in ("lowest", "uniform"):
            raise ValueError("tie must be 'lowest' or 'uniform'")
        if int(plan_cap) < 1:
            raise ValueError("plan_cap must be >= 1")
        if mask is not None:
            mask = mask.to(device=self.device, dtype=torch.uint8)
        index, _, _ = self.cost_to_go(tables)
        plans = torch.zeros((self.num_envs, int(plan_cap)), dtype=torch.uint8, device=self.device)
        plan_len = torch.full((self.num_envs,), PLANS_NONE, dtype=torch.int32, device=self.device)
        for table in tables:  # (a table answers for its own puzzles only: the others keep what another table wrote)
            own = table.covers(self.puzzle_id)
            if mask is not None:
                own &= mask.bool()
            table.plans(index, self.puzzle_id, mask=own, tie=tie, seed=seed, plan_cap=int(plan_cap), out=(plans, plan_len))
        out = replay_plans(self.engine, self.puzzle_id, plans, plan_len, pos=self.pos, mask=mask, include="valid", next_pos=True)
        T = out.num_rows
        out.cost = torch.full((T,), -2, dtype=torch.int32, device=self.device)
        out.acts = torch.zeros((T,), dtype=torch.uint8, device=self.device)
        if T > 0:
            rows = (torch.full((T,), -1, dtype=torch.int32, device=self.device), out.cost, out.acts)
            for table in tables:
                table.query(out.puzzle_id, out.pos, out=rows)
        if observation == "cells":
            out.obs = torch.empty((T,) + self.engine.cells_shape(), dtype=torch.uint8, device=self.device)
            if T > 0:
                self.engine.render_cells(out.puzzle_id, out.pos, out.obs)
        elif observation is not None:
            storage, out.obs = self.engine.alloc_obs(T)
            if T > 0:
                self.engine.render(out.puzzle_id, out.pos, storage)
        return out

    def _own_push_tables(self, tables) -> list:
        from .search import PushSolutionTableBatch

        tables = list(tables)
        for table in tables:
            if isinstance(table, PushSolutionTableBatch):
                if not table.indexed:  # (the index allocates and waits: it is asked for, never built behind a call)
                    raise ValueError("PushSolutionTableBatch is not supported here yet (sampling, plans and demonstrations need a "
                                     "cost index on the batch): pass push_table()s; push_cost_to_go / push_expert_actions take batches")
                if table.engine is not self.engine:
                    raise ValueError("the tables must be made on this environment (VecPushWorld.push_tables)")
                continue
            if table.search._engine is not self.engine:
                raise ValueError("the tables must be made on this environment (VecPushWorld.push_table)")
        return tables

    def reset_from_push_tables(self, tables, cost=(1, None), mask: Optional[torch.Tensor] = None, seed: Optional[int] = None):
        """``reset_from_tables`` with a list of ``push_table``s and / or INDEXED ``push_tables`` batches (``index=True`` or
        ``build_index()``; a batch costs ONE sample launch however many puzzles it holds and draws canonical states, the agent
        at the canon of its walk region; a batch without an index is refused): every (masked) environment whose puzzle has a table in
        ``tables`` starts from a canonical state drawn uniformly among the states of its puzzle with a cost-to-go IN PUSHES
        in ``cost`` = ``(lo, hi)`` (``hi`` None: up to each table's own largest cost; two int32 tensors [B]: a band per
        environment), the agent where the search's push left it.  The band is clamped to each table's costs and dead ends
        are never drawn; environments without a table (or whose table has no solvable state in the band) start from the
        initial state.  One ``pw_reset`` launch, one sample launch per table, one render; no wait once every table has its
        cost index.  Returns the observation tensor.

        ``self.start_row`` (here the store index of the node drawn) / ``self.start_cost`` (int32 [B]) and
        ``self.table_draws`` are ``reset_from_tables``' own: a draw is a function of (seed, environment, count)."""
        tables = self._own_push_tables(tables)
        if mask is not None:
            mask = mask.to(device=self.device, dtype=torch.uint8)
        if getattr(self, "table_draws", None) is None:
            self.table_seed = self.seed
            # (uint32 counter bits over an int32 allocation, like `episode`)
            self.table_draws = torch.zeros((self.num_envs,), dtype=torch.int32, device=self.device).view(torch.uint32)
            self.start_row = torch.full((self.num_envs,), -1, dtype=torch.int32, device=self.device)
            self.start_cost = torch.full((self.num_envs,), -1, dtype=torch.int32, device=self.device)
        if seed is not None:
            self.table_seed = int(seed)
            self.table_draws.view(torch.int32).zero_()
        self._reset_states(mask)
        if mask is None:
            self.start_row.fill_(-1), self.start_cost.fill_(-1)
        else:
            self.start_row.masked_fill_(mask.bool(), -1), self.start_cost.masked_fill_(mask.bool(), -1)
        for table in tables:
            table.sample(self.puzzle_id, self.pos, self.steps, self.terminated, self.truncated, cost=cost, mask=mask,
                         seed=self.table_seed, counter=self.table_draws, out=(self.start_row, self.start_cost))
        if self.guide is not None:
            self.guide.refresh(mask)
        self._obs_current = False
        if self.obs is not None:
            self._render()
        return self.obs

    def optimal_push_demonstrations(self, tables, tie: str = "lowest", seed: int = 0, observation: Optional[str] = "own",
                                    mask: Optional[torch.Tensor] = None, plan_cap: int = 256, masks: bool = False):
        """Fewest-pushes demonstrations in the push-level action space, read off ``push_table``s and / or indexed
        ``push_tables`` batches (one plans and one emit launch per batch, whatever it holds): from every (unmasked)
        environment's current state one ``push_cost_to_go`` over ``tables``, one plans launch per table (``tie`` "lowest":
        each node's best row, "uniform": drawn among its optimal rows with ``seed``), a ``cumsum``, ONE host wait for the
        number of rows T, one emit launch per table -- every push of every plan becomes one row, without a flood or a step
        -- and one render launch.  Environments at a goal state or a dead end, outside every table or with a plan longer
        than ``plan_cap`` contribute no rows.

        Returns a ``types.SimpleNamespace`` of device tensors over the T rows: ``puzzle_id`` int32, ``pos`` int8 [T, NP, 2]
        (the state the push is made from: row 0 of an environment is its live state), ``item`` (the environment) and ``t``
        int32, ``push_from`` int8 [T, 2] / ``push_action`` uint8, ``cost`` int32 (pushes to go, falling by 1 per row to 1),
        ``choice`` int64 -- the push as a flat index into ``[4, map_h, map_w]``, the exact inverse of
        ``search.decode_push_choice``, what ``step_push(choice=...)`` takes -- ``obs`` (``observation`` as in
        ``optimal_demonstrations``; None: no render), ``num_rows`` and, with ``masks``, ``push_mask`` uint8 [T, map_h, map_w]
        (``search.push_mask`` over the rows)."""
        from types import SimpleNamespace

        from .search import encode_push_choice, push_mask

        tables = self._own_push_tables(tables)
        if observation == "own":
            observation = self.observation
        if observation not in ("uint8", "float32", "cells", None):
            raise ValueError("observation must be 'uint8', 'float32', 'cells' or None")
        own_rgb = "uint8" if self.engine.obs_dtype == torch.uint8 else "float32"
        if observation in ("uint8", "float32") and observation != own_rgb:
            raise ValueError(f"this environment's engine renders {own_rgb} pixels: observation must be '{own_rgb}', 'cells' or None")
        if tie not in ("lowest", "uniform"):
            raise ValueError("tie must be 'lowest' or 'uniform'")
        if int(plan_cap) < 1:
            raise ValueError("plan_cap must be >= 1")
        if mask is not None:
            mask = mask.to(device=self.device, dtype=torch.uint8)
        dev = self.device
        T, rows, _, _ = self._push_plan_rows(tables, tie, seed, mask, plan_cap)
        out = SimpleNamespace(num_rows=T, item=rows.item, t=rows.t, state=rows.state, push_from=rows.push_from,
                              push_action=rows.push_action, cost=rows.cost, pos=rows.pos, obs=None)
        out.puzzle_id = self.puzzle_id[rows.item.to(torch.int64)].contiguous() if T > 0 else \
            torch.zeros((0,), dtype=torch.int32, device=dev)
        out.choice = encode_push_choice(rows.push_from, rows.push_action, self.pset.max_height, self.pset.max_width)
        if observation == "cells":
            out.obs = torch.empty((T,) + self.engine.cells_shape(), dtype=torch.uint8, device=dev)
            if T > 0:
                self.engine.render_cells(out.puzzle_id, out.pos, out.obs)
        elif observation is not None:
            storage, out.obs = self.engine.alloc_obs(T)
            if T > 0:
                self.engine.render(out.puzzle_id, out.pos, storage)
        if masks:
            out.push_mask = push_mask(self.engine, out.puzzle_id, out.pos)[0] if T > 0 else \
                torch.zeros((0, self.pset.max_height, self.pset.max_width), dtype=torch.uint8, device=dev)
        return out

    def _push_plan_rows(self, tables, tie: str, seed: int, mask: Optional[torch.Tensor], plan_cap: int):
        """The front half of ``optimal_push_demonstrations``: ``(T, rows, plans, offset)`` -- the query, one plans launch per
        table, the ``cumsum``, the one wait for the number of rows T and one emit launch per table.  ``tables`` are this
        environment's own, ``mask`` uint8 on the device or None."""
        from .search import PushRows, PushSolutionTableBatch, _push_plans_outputs

        B, dev = self.num_envs, self.device
        q = self.push_cost_to_go(tables, mask=mask)
        # (no plan is longer than a table's largest cost: the buffers need no more columns; a cost beyond plan_cap is cut as ever;
        # a batch's largest cost is the host value its index build left)
        costs = [int(t.max_cost_stored if isinstance(t, PushSolutionTableBatch) else t.max_cost) for t in tables]
        width = max(1, min(int(plan_cap), max(costs + [1])))
        plans = _push_plans_outputs(None, B, width, dev)
        owns = []
        for table in tables:  # (a table answers for its own puzzles only: the others keep what another table wrote)
            own = table.covers(self.puzzle_id)
            if mask is not None:
                own &= mask.bool()
            owns.append(own)
            table.plans(q.index, self.puzzle_id, mask=own, tie=tie, seed=seed, plan_cap=width, out=plans)
        offset = torch.zeros((B + 1,), dtype=torch.int64, device=dev)
        torch.cumsum(plans.length.clamp(min=0), 0, out=offset[1:])
        T = int(offset[B].cpu())  # the one wait: the number of rows
        rows = None
        for table, own in zip(tables, owns):
            rows = table.demonstration_rows(plans, pos=self.pos, puzzle_id=self.puzzle_id, mask=own, rows_cap=T, offset=offset,
                                            out=rows)
        if rows is None:
            rows = PushRows(*(torch.zeros((0,) + s, dtype=d, device=dev) for s, d in
                              (((), torch.int32), ((), torch.int32), ((), torch.int32), ((2,), torch.int8), ((), torch.uint8),
                               ((), torch.int32), ((self.num_objects_padded, 2), torch.int8))),
                            torch.zeros((1,), dtype=torch.int32, device=dev).view(torch.uint32), 0)
        return T, rows, plans, offset

    def fewest_push_plans(self, tables, tie: str = "lowest", seed: int = 0, mask: Optional[torch.Tensor] = None,
                          plan_cap: int = 1024, push_cap: int = 256):
        """Fewest-pushes plans IN PRIMITIVE ACTIONS from every (unmasked) environment's current state, read off
        ``push_table``s and / or indexed ``push_tables`` batches: ``optimal_push_demonstrations``' pipeline up to its rows (without a render; plans of at most
        ``push_cap`` pushes), then ``search.push_rows_to_plans`` -- one count launch, one write launch and one gather over the
        rows.  Two host waits: the number of rows and the number of actions.

        Returns a ``types.SimpleNamespace`` of device tensors: ``plans`` uint8 [B, plan_cap], ``plan_len`` int32 [B] and
        ``pushes`` int32 [B] (the pushes of every plan).  ``plan_len`` is 0 for a goal state and -1 for a dead end, a state
        outside every table, a masked environment or a push plan beyond ``push_cap``; a plan of more than ``plan_cap`` actions
        keeps its length and its first ``plan_cap`` actions.  The walk to every push follows the parent actions of the walk
        region, as ``step_push`` walks.  ``search.replay_plans(vec, vec.puzzle_id, r.plans, r.plan_len, pos=vec.pos)`` turns
        the plans into primitive demonstration rows (rewards, dones, and observations through ``demonstrations``' renders)."""
        from types import SimpleNamespace

        from .search import push_rows_to_plans

        tables = self._own_push_tables(tables)
        if tie not in ("lowest", "uniform"):
            raise ValueError("tie must be 'lowest' or 'uniform'")
        if not 1 <= int(plan_cap) <= _capi.PLAN_MAX_ACTIONS:
            raise ValueError(f"plan_cap must be in 1 .. {_capi.PLAN_MAX_ACTIONS}")
        if int(push_cap) < 1:
            raise ValueError("push_cap must be >= 1")
        if mask is not None:
            mask = mask.to(device=self.device, dtype=torch.uint8)
        T, rows, push_plans, offset = self._push_plan_rows(tables, tie, seed, mask, push_cap)
        ids = self.puzzle_id[rows.item.to(torch.int64)].contiguous() if T > 0 else \
            torch.zeros((0,), dtype=torch.int32, device=self.device)
        plans, plan_len, pushes = push_rows_to_plans(self.engine, ids, rows, offset, plan_cap=int(plan_cap))
        plan_len = torch.where(push_plans.length < 0, torch.full_like(plan_len, -1), plan_len)
        return SimpleNamespace(plans=plans, plan_len=plan_len, pushes=pushes)

    def set_states(self, pos: np.ndarray) -> None:
        self.pos.copy_(torch.as_tensor(np.asarray(pos), dtype=torch.int8))
        self._has_reset = True
        self._obs_current = False
        if self.guide is not None:
            self.guide.refresh()

"""Vector-environment facades over ``VecPushWorld``.

``PushWorldVectorEnv`` has the call surface of ``gymnasium.vector.VectorEnv`` (``reset`` /
``step`` / ``step_async`` / ``step_wait`` / spaces / ``close``) and ``PushWorldDmVectorEnv`` returns
batched ``dm_env.TimeStep`` tuples.  Per environment the semantics are the reference's
``PushWorldEnv`` (python3/src/pushworld/gym_env.py:57-226, dm_env.py:60-234): same constructor
arguments, rewards, ``terminated`` / ``truncated``; episode turnover follows gymnasium's
next-step autoreset -- the ``step`` after a finished episode ignores the action, draws a new
puzzle on the device (``pw_resample``), resets and returns that puzzle's first observation with
reward 0.  Nothing leaves the GPU unless ``to_numpy=True``.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _capi, _compat
from .config import PUZZLE_EXTENSION
from .puzzle import DEFAULT_BORDER_WIDTH, DEFAULT_PIXELS_PER_CELL, NUM_ACTIONS, PushWorldPuzzle
from ._single_env import pool_frame
from .utils.filesystem import iter_files_with_extension
from .start_pool import check_start_options
from .vec_env import VecPushWorld


class _BatchSpace:
    """Space of ``num_envs`` stacked copies of a single space (``gymnasium.vector.utils.batch_space``)."""

    def __init__(self, single, num_envs: int):
        self.single = single
        self.num_envs = int(num_envs)
        self.shape = (self.num_envs,) + tuple(single.shape)
        self.dtype = single.dtype

    def contains(self, x) -> bool:
        x = np.asarray(x)
        if x.shape != self.shape:
            return False
        if hasattr(self.single, "n"):
            return bool(np.issubdtype(x.dtype, np.integer) and (x >= 0).all() and (x < self.single.n).all())
        return bool((x >= self.single.low).all() and (x <= self.single.high).all())

    __contains__ = contains

    def sample(self):
        if hasattr(self.single, "n"):
            return np.random.default_rng().integers(self.single.n, size=self.shape)
        raise NotImplementedError

    def __repr__(self):
        return f"Batch({self.single!r}, {self.num_envs})"


def _load_pool(puzzle_path, standard_padding: bool):
    """The puzzle pool and padded frame of ``PushWorldEnv.__init__`` (gym_env.py:66-103)."""
    if isinstance(puzzle_path, (list, tuple)):
        puzzles = [p if isinstance(p, PushWorldPuzzle) else PushWorldPuzzle(p) for p in puzzle_path]
    else:
        puzzles = [PushWorldPuzzle(p) for p in iter_files_with_extension(puzzle_path, PUZZLE_EXTENSION)]
    if len(puzzles) == 0:
        raise ValueError(f"No PushWorld puzzles found in: {puzzle_path}")
    return puzzles, pool_frame(puzzles, standard_padding)


class _VectorCore:
    use_shaped_reward = False  # set_guide(..., use_shaped_reward=True): the returned reward is the guide's shaped one

    def __init__(self, puzzle_path, num_envs: int, max_steps: Optional[int], border_width: int, pixels_per_cell: int,
                 standard_padding: bool, observation: str, seed: int, sample_table, device: Optional[int],
                 to_numpy: bool, incremental: bool = True, curriculum=None, curriculum_update_every: Optional[int] = None,
                 start_pool=None, start_band="pool", start_keep_initial: float = 0.0, start_update_every=None):
        if curriculum_update_every is not None:
            if curriculum is None:
                raise ValueError("curriculum_update_every needs a curriculum")
            if isinstance(curriculum_update_every, bool) or not isinstance(curriculum_update_every, int) \
                    or curriculum_update_every < 1:
                raise ValueError("curriculum_update_every must be None or an integer >= 1")
        update_kw = {}
        if start_update_every is not None:
            if start_pool is None:
                raise ValueError("start_update_every needs a start_pool")
            if isinstance(start_update_every, dict):  # {"every": k, ...}: the other entries are update_bands' arguments
                update_kw = dict(start_update_every)
                start_update_every = update_kw.pop("every", None)
            if isinstance(start_update_every, bool) or not isinstance(start_update_every, int) or start_update_every < 1:
                raise ValueError("start_update_every must be None, an integer >= 1 or a dict with such an 'every'")
        check_start_options(start_pool, start_band, start_keep_initial, True)
        if border_width < 1:
            raise ValueError("border_width must be >= 1")
        if pixels_per_cell < 3:
            raise ValueError("pixels_per_cell must be >= 3")
        if observation not in ("float32", "uint8", "cells"):
            raise ValueError("observation must be 'float32', 'uint8' or 'cells'")
        puzzles, pad = _load_pool(puzzle_path, standard_padding)
        cells = observation == "cells"
        self.vec = VecPushWorld(puzzles, num_envs, max_steps=max_steps, border_width=border_width,
                                pixels_per_cell=pixels_per_cell, observation=observation, pad_cells=pad,
                                device=device, autoreset=True, resample=True if sample_table is None else sample_table,
                                seed=seed, incremental=incremental and not cells, curriculum=curriculum,
                                episode_stats=start_update_every is not None, start_pool=start_pool, start_band=start_band,
                                start_keep_initial=start_keep_initial)
        # ... and after every `start_update_every`-th step the bands of the start pool move with the statistics (K27)
        self.start_update_every = start_update_every
        self._start_update_kw = update_kw
        self._steps_to_start_update = start_update_every
        # steps counted on the host (no wait): after every `curriculum_update_every`-th step the weights are made anew from the
        # statistics that step left, so the draws of the following step are the first to use them
        self.curriculum_update_every = curriculum_update_every
        self._steps_to_update = curriculum_update_every
        self.num_envs = int(num_envs)
        self.to_numpy = bool(to_numpy)
        self._obs_dtype = np.float32 if observation == "float32" else np.uint8
        if cells:  # codes 0 .. 3 in plane 0, 0 .. 1 + largest movable index in planes 1 and 2
            self._obs_high = max(3, max(p.num_movables for p in puzzles))
            self._obs_shape = tuple(self.vec.obs.shape[1:])
        else:
            self._obs_high = 1.0 if observation == "float32" else 255
            self._obs_shape = self.vec.engine.obs_shape
        self._rgb = None  # RGB frames of render() in cells mode: (storage, view), allocated by the first call
        self._pending = False
        self._closed = False

    @property
    def puzzles(self):
        return self.vec.puzzles

    @property
    def start_pool(self):
        """The ``start_pool.StartPool`` new episodes draw their start state from (None: the puzzle's initial state).
        ``vec.start_entry`` / ``vec.start_level`` hold what every environment started from."""
        return self.vec.start_pool

    @property
    def curriculum(self):
        """The ``curriculum.Curriculum`` the puzzles are drawn by (None: uniformly or from the sample table)."""
        return self.vec.curriculum

    def puzzle_stats(self):
        """``VecPushWorld.puzzle_stats``: the statistics per puzzle kept on the device (needs ``curriculum``).  Waits."""
        return self.vec.puzzle_stats()

    def _start_info(self, info: dict) -> dict:
        """With a start pool: ``start_entry`` / ``start_level`` int32 [B], the pool entry and the level every environment's
        episode started from (-1 / -1: the puzzle's initial state).  Without one ``info`` is as it was."""
        if self.vec.start_pool is not None:
            info["start_entry"], info["start_level"] = self._out(self.vec.start_entry), self._out(self.vec.start_level)
        return info

    def set_guide(self, tables_or_guide, use_shaped_reward: bool = False, **kw):
        """``VecPushWorld.set_guide``: exact cost-to-go guidance kept current inside every step.  Make the
        tables on this environment's own engine (``env.vec.solution_tables()`` and the like).  With a guide ``info`` (the
        dm_env forms: ``TimeStep.observation``, a dict with the observation batch under ``"board"``) gains ``cost_to_go`` int32
        [B] (-1 dead end, -2 unknown), ``guide_actions`` uint8 [B] (bits 0..3 optimal, 4..7 safe), ``dead_end`` uint8 [B] and
        ``shaped_reward`` float64 [B]; ``use_shaped_reward`` returns the shaped reward as the step's reward.  None removes
        the guide.  Returns the ``guide.ValueGuide``."""
        if use_shaped_reward and (tables_or_guide is None or kw.get("shaping") is False):
            raise ValueError("use_shaped_reward needs a guide with shaping")
        guide = self.vec.set_guide(tables_or_guide, **kw)
        if use_shaped_reward and guide.shaped is None:
            self.vec.set_guide(None)
            raise ValueError("use_shaped_reward needs a guide with shaping")
        self.use_shaped_reward = bool(use_shaped_reward) and guide is not None
        return guide

    def _guide_info(self, info: dict) -> dict:
        """With a guide: ``cost_to_go``, ``guide_actions``, ``dead_end``, ``shaped_reward``.  Without one ``info`` is as it was."""
        g = self.vec.guide
        if g is not None:
            info["cost_to_go"], info["guide_actions"] = self._out(g.cost), self._out(g.acts)
            info["dead_end"] = self._out(g.dead)
            info["shaped_reward"] = None if g.shaped is None else self._out(g.shaped)
        return info

    def _reward(self, reward):
        """The reward a step returns: the guide's shaped one when ``use_shaped_reward`` is on."""
        return self.vec.guide.shaped if self.use_shaped_reward and self.vec.guide is not None else reward

    def _count_step(self) -> None:
        if self._steps_to_update is not None:
            self._steps_to_update -= 1
            if self._steps_to_update == 0:
                self.vec.curriculum.update()
                self._steps_to_update = self.curriculum_update_every
        if self._steps_to_start_update is not None:
            self._steps_to_start_update -= 1
            if self._steps_to_start_update == 0:
                self.vec.start_pool.update_bands(self.vec.stats, **self._start_update_kw)
                self._steps_to_start_update = self.start_update_every

    @property
    def puzzle_ids(self) -> torch.Tensor:
        """int32 [num_envs]: index (into ``puzzles``) of each environment's current puzzle."""
        return self.vec.puzzle_id

    def _actions(self, actions) -> torch.Tensor:
        if isinstance(actions, torch.Tensor):
            a = actions
            if a.shape != (self.num_envs,) or a.dtype in (torch.bool, torch.float16, torch.float32, torch.float64, torch.bfloat16):
                raise ValueError("The provided action is not in the action space.")
            if a.device != self.vec.device or a.dtype != torch.uint8:
                # Wider integer types are range-checked BEFORE the cast (256 would become LEFT, -1 would become
                # 255): one fused reduction where the tensor lives; on the device this synchronises, which the
                # conversion path can afford -- pass uint8 device tensors to stay asynchronous.
                if bool(((a < 0) | (a >= NUM_ACTIONS)).any()):
                    raise ValueError("The provided action is not in the action space.")
                a = a.to(device=self.vec.device, dtype=torch.uint8)
            return a
        arr = np.asarray(actions)
        if arr.shape != (self.num_envs,) or not np.issubdtype(arr.dtype, np.integer) or (arr < 0).any() or (arr >= NUM_ACTIONS).any():
            raise ValueError("The provided action is not in the action space.")
        return torch.as_tensor(arr.astype(np.uint8)).to(self.vec.device)

    def _out(self, t: torch.Tensor):
        return t.cpu().numpy() if self.to_numpy else t

    def _launch(self, actions) -> None:
        if self._pending:
            raise RuntimeError("step_async() was called twice without step_wait()")
        self.vec.step(self._actions(actions))  # asynchronous on the current HIP stream
        self._count_step()
        self._pending = True

    def _collect(self):
        if not self._pending:
            raise RuntimeError("step_wait() called without a pending step_async()")
        self._pending = False
        v = self.vec
        if self.to_numpy:  # the .cpu() copies synchronise; device tensors stay stream-ordered
            bad = v.terminated.cpu().numpy() == 0xFF
            if bad.any():  # device-side action check of pw_step (action outside 0..3)
                v.engine.bad_actions()  # reported here: clear the sticky counter
                raise ValueError("The provided action is not in the action space.")
        return v.obs, v.reward, v.terminated, v.truncated

    def check_actions(self) -> None:
        """Device-tensor mode (``to_numpy=False``) never synchronises, so a uint8 action outside 0..3 cannot raise
        inside ``step``: the kernel leaves that environment untouched, flags it 0xFF (the next step then resets
        it) and counts it in the engine's sticky counter.  This reads and clears the counter (one stream
        synchronisation) and raises the reference's ``ValueError`` (gym_env.py:195-196) if any was seen."""
        n = self.vec.engine.bad_actions()
        if n:
            raise ValueError(f"The provided action is not in the action space. ({n} since the last check)")

    def close(self) -> None:
        self._closed = True


class PushWorldVectorEnv(_VectorCore):
    """``gymnasium.vector.VectorEnv``-style batch of ``PushWorldEnv``s on one MI355X.

    Args (first five as ``PushWorldEnv``, gym_env.py:57-64):
        puzzle_path: ``.pwp`` file, directory searched recursively, or a list of paths / puzzles.
        num_envs: batch size B.
        observation: "float32" (reference observation, values in [0, 1]), "uint8" (4x fewer bytes) or "cells" (the
            cell-grid observation uint8 [B, 3, Hc, Wc]; ``render()`` still returns RGB frames).
        seed: seed of the per-episode puzzle draw.
        sample_table: optional pool indices to draw from (repeats = weights); default uniform.
        curriculum: draw by weights made on the device from the statistics per puzzle: a mode name
            ("uniform", "failure", "frontier", "given") or a ``curriculum.Curriculum``; not together with ``sample_table``.
            ``puzzle_stats()`` reads the statistics, ``curriculum.update()`` refreshes the weights.
        curriculum_update_every: refresh the weights after every that many steps (counted on the host: no wait).
        start_pool, start_band, start_keep_initial: ``VecPushWorld``'s: new episodes start from states drawn
            on the device from a ``start_pool.StartPool`` of a set of these puzzles (``StartPool.from_tables`` on any
            ``VecPushWorld`` over the same puzzles).  ``info["start_entry"]`` / ``info["start_level"]`` (with a pool only; also
            ``vec.start_entry`` / ``vec.start_level``, which the dm_env forms read there) hold what every episode started from.
        start_update_every: move the pool's bands with the statistics per puzzle (``StartPool.update_bands``, one launch) after
            every that many steps, counted on the host; a dict ``{"every": k, "min_episodes": ..., "up": ..., ...}`` passes
            ``update_bands``' arguments.  Turns the statistics on (``puzzle_stats()``).
        to_numpy: return host numpy arrays (and python-side checks) instead of device tensors.
    """

    metadata = {"render_modes": ["rgb_array"], "autoreset_mode": "next_step"}
    render_mode = "rgb_array"

    def __init__(self, puzzle_path, num_envs: int, max_steps: Optional[int] = None,
                 border_width: int = DEFAULT_BORDER_WIDTH, pixels_per_cell: int = DEFAULT_PIXELS_PER_CELL,
                 standard_padding: bool = False, observation: str = "float32", seed: int = 0, sample_table=None,
                 device: Optional[int] = None, to_numpy: bool = False, curriculum=None,
                 curriculum_update_every: Optional[int] = None, start_pool=None, start_band="pool",
                 start_keep_initial: float = 0.0, start_update_every=None):
        super().__init__(puzzle_path, num_envs, max_steps, border_width, pixels_per_cell, standard_padding,
                         observation, seed, sample_table, device, to_numpy, curriculum=curriculum,
                         curriculum_update_every=curriculum_update_every, start_pool=start_pool, start_band=start_band,
                         start_keep_initial=start_keep_initial, start_update_every=start_update_every)
        self.single_action_space = _compat.make_discrete(NUM_ACTIONS)
        self.single_observation_space = _compat.make_box(0, self._obs_high, self._obs_shape, self._obs_dtype)
        self.action_space = _BatchSpace(_compat.Discrete(NUM_ACTIONS), num_envs)
        self.observation_space = _BatchSpace(_compat.Box(0, self._obs_high, self._obs_shape, self._obs_dtype),
                                             num_envs)

    def reset(self, seed: Optional[int] = None, options: Optional[dict] = None):
        """All environments draw a puzzle and start an episode (gym_env.py:150-186).  Returns
        ``(obs [B, H, W, 3], {"puzzle_id": int32 [B]})``."""
        self._pending = False
        obs = self.vec.reset(seed=seed)
        return self._out(obs), self._info()

    def _info(self) -> dict:
        """``puzzle_state``: int8 [B, NP, 2] (x, y) positions, agent first, zero beyond a puzzle's movables
        (the batched form of the reference's ``info["puzzle_state"]``, gym_env.py:186,226)."""
        return self._guide_info(self._start_info({"puzzle_id": self._out(self.vec.puzzle_id),
                                                  "puzzle_state": self._out(self.vec.pos)}))

    def step_async(self, actions) -> None:
        self._launch(actions)

    def step_wait(self):
        obs, reward, terminated, truncated = self._collect()
        reward = self._reward(reward)
        info = self._info()
        if self.to_numpy:
            return (obs.cpu().numpy(), reward.cpu().numpy(), terminated.cpu().numpy().astype(bool),
                    truncated.cpu().numpy().astype(bool), info)
        return obs, reward, terminated, truncated, info

    def step(self, actions):
        """gym_env.py:188-226 for every environment -> ``(obs, reward f64[B], terminated, truncated, info)``."""
        self.step_async(actions)
        return self.step_wait()

    def render(self):
        """uint8 frames [B, H, W, 3] of the current states (padded frame)."""
        if self.vec.observation == "cells":  # RGB on demand, into a buffer of its own
            if self._rgb is None:
                self._rgb = self.vec.engine.alloc_obs(self.num_envs)
            self.vec.engine.render(self.vec.puzzle_id, self.vec.pos, self._rgb[0])
            return self._out(self._rgb[1])
        if self.vec.observation == "uint8":
            return self._out(self.vec.obs)
        return self._out((self.vec.obs * 255.0).round().to(torch.uint8))


class PushWorldDmVectorEnv(_VectorCore):
    """Batched ``dm_env`` flavour: ``reset`` / ``step`` return one ``TimeStep`` whose fields are
    [B]-shaped (``step_type`` int32, ``reward`` float64, ``discount`` float64) plus the observation
    batch.  Per environment: FIRST after a (auto)reset with reward 0 / discount 1 (``dm_env.restart``
    carries None there; arrays cannot), LAST with discount 0 when terminated or truncated
    (dm_env.py:229-232), MID otherwise."""

    def __init__(self, puzzle_path, num_envs: int, max_steps: Optional[int] = None,
                 border_width: int = DEFAULT_BORDER_WIDTH, pixels_per_cell: int = DEFAULT_PIXELS_PER_CELL,
                 standard_padding: bool = False, observation: str = "float32", seed: int = 0, sample_table=None,
                 device: Optional[int] = None, to_numpy: bool = False, curriculum=None,
                 curriculum_update_every: Optional[int] = None, start_pool=None, start_band="pool",
                 start_keep_initial: float = 0.0, start_update_every=None):
        super().__init__(puzzle_path, num_envs, max_steps, border_width, pixels_per_cell, standard_padding,
                         observation, seed, sample_table, device, to_numpy, curriculum=curriculum,
                         curriculum_update_every=curriculum_update_every, start_pool=start_pool, start_band=start_band,
                         start_keep_initial=start_keep_initial, start_update_every=start_update_every)
        self._action_spec = _compat.make_discrete_array(NUM_ACTIONS, int, "action")
        self._observation_spec = _compat.make_bounded_array(self._obs_shape, self._obs_dtype, "board", 0,
                                                            self._obs_high)
        self._was_done = None

    def action_spec(self):
        return self._action_spec

    def observation_spec(self):
        return self._observation_spec

    def _timestep(self, step_type, reward, discount, obs):
        # (with a guide the observation is a dict: the batch under "board" next to the guide's four entries)
        observation = self._out(obs) if self.vec.guide is None else self._guide_info({"board": self._out(obs)})
        return _compat.TimeStep(self._out(step_type), self._out(reward), self._out(discount), observation)

    def reset(self, seed: Optional[int] = None):
        self._pending = False
        obs = self.vec.reset(seed=seed)
        dev = self.vec.device
        self._was_done = torch.zeros((self.num_envs,), dtype=torch.bool, device=dev)
        return self._timestep(torch.full((self.num_envs,), int(_compat.StepType.FIRST), dtype=torch.int32, device=dev),
                              torch.zeros((self.num_envs,), dtype=torch.float64, device=dev),
                              torch.ones((self.num_envs,), dtype=torch.float64, device=dev), obs)

    def step(self, actions):
        if self._was_done is None:
            raise RuntimeError("reset() must be called before step() can be called.")
        self._launch(actions)
        obs, reward, terminated, truncated = self._collect()
        done = (terminated != 0) | (truncated != 0)
        first = self._was_done  # this call reset those environments
        step_type = torch.where(first, int(_compat.StepType.FIRST),
                                torch.where(done, int(_compat.StepType.LAST), int(_compat.StepType.MID))).to(torch.int32)
        discount = torch.where(done & ~first, 0.0, 1.0).to(torch.float64)
        self._was_done = done & ~first
        return self._timestep(step_type, self._reward(reward), discount, obs)


# ---------------------------------------------------------------------------------------------------------- push mode
def push_action_spaces(map_h: int, map_w: int, num_envs: int):
    """``(single_action_space, action_space)`` of the push-mode facades: an action is the flat index into ``[4, map_h,
    map_w]`` -- (direction, y, x) of the agent position the push starts from -- what ``VecPushWorld.step_push(choice=...)``
    takes."""
    n = 4 * int(map_h) * int(map_w)
    return _compat.make_discrete(n), _BatchSpace(_compat.Discrete(n), num_envs)


class _PushCore(_VectorCore):
    """The core of the push-mode facades: every step is ONE ``VecPushWorld.step_push_mask(choice=..., end_stuck=True)``."""

    def __init__(self, *args, **kw):
        super().__init__(*args, **kw)
        v = self.vec
        self.map_h, self.map_w = v.pset.max_height, v.pset.max_width
        self.num_choices = 4 * self.map_h * self.map_w
        self._bits = torch.tensor([1, 2, 4, 8], dtype=torch.uint8, device=v.device).view(1, 4, 1, 1)
        self._refused = torch.zeros((), dtype=torch.int64, device=v.device)  # refused choices since the last check
        self._step = None  # the PushStep of the pending / last step

    def _actions(self, actions) -> torch.Tensor:
        """int64 [B] on the device.  Host arrays are range-checked here; a device tensor is checked by the step itself (an
        index outside the shape decodes to ``PUSH_NONE``: a refused choice)."""
        if isinstance(actions, torch.Tensor):
            if actions.shape != (self.num_envs,) or actions.dtype not in (torch.int64, torch.int32, torch.int16, torch.int8,
                                                                          torch.uint8):
                raise ValueError("The provided action is not in the action space.")
            return actions.to(device=self.vec.device, dtype=torch.int64)
        arr = np.asarray(actions)
        if arr.shape != (self.num_envs,) or not np.issubdtype(arr.dtype, np.integer) or (arr < 0).any() \
                or (arr >= self.num_choices).any():
            raise ValueError("The provided action is not in the action space.")
        return torch.as_tensor(arr.astype(np.int64)).to(self.vec.device)

    def _launch(self, actions) -> None:
        if self._pending:
            raise RuntimeError("step_async() was called twice without step_wait()")
        choice = self._actions(actions)
        v = self.vec
        if not v._has_reset:
            raise RuntimeError("reset() must be called before step() can be called.")
        # an environment without a push move has no choice to make: its refusal is the stuck rule's business, not an error.
        # (the views are current here: reset() and every step leave them so)
        could = v.push_view_count > 0
        self._step = v.step_push_mask(choice=choice, end_stuck=True)  # asynchronous on the current HIP stream
        self._refused += ((self._step.status == _capi.PUSH_REFUSED) & could).sum()
        self._count_step()
        self._pending = True

    def _collect(self):
        if not self._pending:
            raise RuntimeError("step_wait() called without a pending step_async()")
        self._pending = False
        if self.to_numpy:  # the host path synchronises anyway: a refused choice raises at once
            self.check_actions()
        return self._step

    def _observe(self):
        """After ``vec.reset``: the views of the first states (``observe_pushes``)."""
        self.vec.observe_pushes()
        self._refused.zero_()

    def _action_mask(self) -> torch.Tensor:
        """bool [B, 4 * map_h * map_w]: entry ``(a * map_h + y) * map_w + x`` is set when ``((x, y), a)`` is a push move."""
        return ((self.vec.push_view_mask.unsqueeze(1) & self._bits) != 0).view(self.num_envs, self.num_choices)

    def check_actions(self) -> None:
        """Device-tensor mode (``to_numpy=False``) never synchronises, so a choice that is no push move cannot raise inside
        ``step``: the environment is left as it was (reward 0, ``status`` 0) and the refusal is counted on the device.  This
        reads and clears the count (one stream synchronisation) and raises ``ValueError`` if any choice was refused since the
        last check.  Choices of environments without any push move (``stuck``) and of environments that the step reset are
        not counted: there was nothing valid to choose."""
        n = int(self._refused.item())
        self._refused.zero_()
        if n:
            raise ValueError(f"The provided action is not in the action space: no push move. ({n} since the last check)")


class PushWorldPushVectorEnv(_PushCore):
    """``PushWorldVectorEnv`` in the push-level action space: an action is a push move -- the agent walks
    to a cell of its walk region along the shortest path and pushes from there -- given as the flat index into ``[4, map_h,
    map_w]`` (direction, y, x), the shape of a policy head's logits and of ``info["action_mask"]``.  One ``step`` is one
    launch (``pw_step_push_mask``) plus the render; its reward is the sum of the primitive rewards of the walk and the push.

    Constructor arguments as ``PushWorldVectorEnv``.  Next-step autoreset: the ``step`` after a finished episode ignores the
    choice, draws a new puzzle and returns its first observation with reward 0.  An environment that is left without any
    push move and is not solved is ``stuck``: it is truncated at once, and reset by the following ``step``.

    ``info``: ``action_mask`` bool [B, 4 * map_h * map_w]; ``push_mask`` uint8 [B, map_h, map_w] (the same, packed: bit a of
    [y, x]); ``num_pushes`` int32 [B]; ``moves`` int32 [B] primitive steps executed; ``status`` int8 [B] (``PUSH_DONE`` /
    ``PUSH_CUT`` / ``PUSH_REFUSED`` / ``PUSH_RESET``); ``stuck`` bool [B]; ``puzzle_id``; ``puzzle_state``.  A choice that is
    no push move is a refused no-op (reward 0, ``status`` 0); see ``check_actions``.  With ``to_numpy=True`` it raises."""

    metadata = {"render_modes": ["rgb_array"], "autoreset_mode": "next_step"}
    render_mode = "rgb_array"

    def __init__(self, puzzle_path, num_envs: int, max_steps: Optional[int] = None,
                 border_width: int = DEFAULT_BORDER_WIDTH, pixels_per_cell: int = DEFAULT_PIXELS_PER_CELL,
                 standard_padding: bool = False, observation: str = "float32", seed: int = 0, sample_table=None,
                 device: Optional[int] = None, to_numpy: bool = False, curriculum=None,
                 curriculum_update_every: Optional[int] = None, start_pool=None, start_band="pool",
                 start_keep_initial: float = 0.0, start_update_every=None):
        super().__init__(puzzle_path, num_envs, max_steps, border_width, pixels_per_cell, standard_padding,
                         observation, seed, sample_table, device, to_numpy, curriculum=curriculum,
                         curriculum_update_every=curriculum_update_every, start_pool=start_pool, start_band=start_band,
                         start_keep_initial=start_keep_initial, start_update_every=start_update_every)
        self.single_action_space, self.action_space = push_action_spaces(self.map_h, self.map_w, num_envs)
        self.single_observation_space = _compat.make_box(0, self._obs_high, self._obs_shape, self._obs_dtype)
        self.observation_space = _BatchSpace(_compat.Box(0, self._obs_high, self._obs_shape, self._obs_dtype),
                                             num_envs)

    def reset(self, seed: Optional[int] = None, options: Optional[dict] = None):
        """All environments draw a puzzle and start an episode.  Returns ``(obs, info)``; ``moves`` and ``status`` are zeros."""
        self._pending = False
        obs = self.vec.reset(seed=seed)
        self._observe()
        zeros = torch.zeros((self.num_envs,), dtype=torch.int32, device=self.vec.device)
        return self._out(obs), self._info(zeros, zeros.to(torch.int8))

    def _info(self, moves, status) -> dict:
        v = self.vec
        info = self._start_info({"action_mask": self._out(self._action_mask()), "push_mask": self._out(v.push_view_mask),
                                 "num_pushes": self._out(v.push_view_count), "moves": self._out(moves),
                                 "status": self._out(status), "stuck": self._out((v.push_view_count == 0) & (v.terminated == 0)),
                                 "puzzle_id": self._out(v.puzzle_id), "puzzle_state": self._out(v.pos)})
        return self._guide_info(info)

    def step_async(self, actions) -> None:
        self._launch(actions)

    def step_wait(self):
        s = self._collect()
        reward = self._reward(s.reward)
        info = self._info(s.moves, s.status)
        if self.to_numpy:
            return (s.obs.cpu().numpy(), reward.cpu().numpy(), s.terminated.cpu().numpy().astype(bool),
                    s.truncated.cpu().numpy().astype(bool), info)
        return s.obs, reward, s.terminated, s.truncated, info

    def step(self, actions):
        """One macro step per environment -> ``(obs, reward f64[B], terminated, truncated, info)``."""
        self.step_async(actions)
        return self.step_wait()

    render = PushWorldVectorEnv.render


class PushWorldPushDmVectorEnv(_PushCore):
    """Batched ``dm_env`` flavour of ``PushWorldPushVectorEnv``: ``TimeStep.observation`` is ``{"board": obs, "action_mask":
    bool [B, 4 * map_h * map_w]}``; step types and discounts follow ``PushWorldDmVectorEnv``'s rules (FIRST after a
    (auto)reset with reward 0 / discount 1, LAST with discount 0 when terminated or truncated -- the stuck rule included --
    MID otherwise)."""

    def __init__(self, puzzle_path, num_envs: int, max_steps: Optional[int] = None,
                 border_width: int = DEFAULT_BORDER_WIDTH, pixels_per_cell: int = DEFAULT_PIXELS_PER_CELL,
                 standard_padding: bool = False, observation: str = "float32", seed: int = 0, sample_table=None,
                 device: Optional[int] = None, to_numpy: bool = False, curriculum=None,
                 curriculum_update_every: Optional[int] = None, start_pool=None, start_band="pool",
                 start_keep_initial: float = 0.0, start_update_every=None):
        super().__init__(puzzle_path, num_envs, max_steps, border_width, pixels_per_cell, standard_padding,
                         observation, seed, sample_table, device, to_numpy, curriculum=curriculum,
                         curriculum_update_every=curriculum_update_every, start_pool=start_pool, start_band=start_band,
                         start_keep_initial=start_keep_initial, start_update_every=start_update_every)
        self._action_spec = _compat.make_discrete_array(self.num_choices, int, "action")
        self._observation_spec = {
            "board": _compat.make_bounded_array(self._obs_shape, self._obs_dtype, "board", 0, self._obs_high),
            "action_mask": _compat.make_bounded_array((self.num_choices,), np.bool_, "action_mask", False, True),
        }
        self._was_done = None

    def action_spec(self):
        return self._action_spec

    def observation_spec(self):
        return self._observation_spec

    def _timestep(self, step_type, reward, discount, obs):
        observation = self._guide_info({"board": self._out(obs), "action_mask": self._out(self._action_mask())})
        return _compat.TimeStep(self._out(step_type), self._out(reward), self._out(discount), observation)

    def reset(self, seed: Optional[int] = None):
        self._pending = False
        obs = self.vec.reset(seed=seed)
        self._observe()
        dev = self.vec.device
        self._was_done = torch.zeros((self.num_envs,), dtype=torch.bool, device=dev)
        return self._timestep(torch.full((self.num_envs,), int(_compat.StepType.FIRST), dtype=torch.int32, device=dev),
                              torch.zeros((self.num_envs,), dtype=torch.float64, device=dev),
                              torch.ones((self.num_envs,), dtype=torch.float64, device=dev), obs)

    def step(self, actions):
        if self._was_done is None:
            raise RuntimeError("reset() must be called before step() can be called.")
        self._launch(actions)
        s = self._collect()
        done = (s.terminated != 0) | (s.truncated != 0)
        first = self._was_done  # this call reset those environments
        step_type = torch.where(first, int(_compat.StepType.FIRST),
                                torch.where(done, int(_compat.StepType.LAST), int(_compat.StepType.MID))).to(torch.int32)
        discount = torch.where(done & ~first, 0.0, 1.0).to(torch.float64)
        # (a reset clears the flags, but the stuck rule may set truncated again in the same call -- an initial state without a
        # push move: the next call resets that environment once more, so it is FIRST again)
        self._was_done = done
        return self._timestep(step_type, self._reward(s.reward), discount, s.obs)

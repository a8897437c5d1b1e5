"""``python -m pushworld_amd.benchmark_rgd``: the reference's ``benchmark_rgd_planner`` on the GPU.

Every puzzle below ``--puzzles-path`` is planned by best-first search (RGD or N+RGD) -- all of them in one launch
(``search.PlanBatch``), each under its own time limit -- and one YAML result per puzzle is written under ``--results-path``,
mirroring the puzzles' directory structure.  The files hold the reference's keys: ``planner``, ``puzzle``, ``plan`` (a string of
L / R / U / D, or null), ``planning_time`` (seconds) and, without a plan, ``failure_reason``.  All plans are checked by one
replay launch (``PlanBatch.validate``: the reference's ``is_valid_plan``) before they are written.  The YAML is written here, in ``yaml.dump``'s format for these
flat mappings (keys sorted, plain scalars where PyYAML writes them plain): PyYAML is not needed.
"""
from __future__ import annotations

import argparse
import math
import os
import re
import sys
import time
from typing import Optional

PLANNER_NAMES = {"N+RGD": "Novelty+RGD", "RGD": "RGD"}
GIGABYTE = 1 << 30
MAX_STATES_CAP = 1 << 24  # states per puzzle at most, whatever the memory limit

# strings that a YAML 1.1 loader would read as something else (PyYAML's implicit resolvers)
_IMPLICIT = re.compile(r"""^(?:
    ~|null|Null|NULL|yes|Yes|YES|no|No|NO|true|True|TRUE|false|False|FALSE|on|On|ON|off|Off|OFF|y|Y|n|N|=|<<
  | [-+]?(?:0b[0-1_]+|0[0-7_]+|(?:0|[1-9][0-9_]*)|0x[0-9a-fA-F_]+|[1-9][0-9_]*(?::[0-5]?[0-9])+)
  | [-+]?(?:[0-9][0-9_]*)\.[0-9_]*(?:[eE][-+][0-9]+)?|\.[0-9_]+(?:[eE][-+][0-9]+)?|[-+]?[0-9][0-9_]*(?::[0-5]?[0-9])+\.[0-9_]*
  | [-+]?\.(?:inf|Inf|INF)|\.(?:nan|NaN|NAN)
  | [0-9][0-9][0-9][0-9]-[0-9][0-9]?-[0-9][0-9]?.*
)$""", re.X)


def yaml_scalar(value) -> str:
    """One scalar as ``yaml.dump`` writes it in a block mapping."""
    if value is None:
        return "null"
    if isinstance(value, bool):
        return "true" if value else "false"
    if isinstance(value, int):
        return str(value)
    if isinstance(value, float):
        if value != value:
            return ".nan"
        if math.isinf(value):
            return ".inf" if value > 0 else "-.inf"
        r = repr(value).lower()
        if "." not in r and "e" in r:  # PyYAML's representer: 1e-05 -> 1.0e-05
            r = r.replace("e", ".0e", 1)
        return r
    s = str(value)
    if any(not " " <= c < "\x7f" for c in s):  # double quotes with escapes, as PyYAML writes them
        esc = {"\t": "\\t", "\n": "\\n", "\r": "\\r", "\\": "\\\\", '"': '\\"'}
        return '"' + "".join(esc.get(c) or (c if " " <= c < "\x7f" else
                                            (f"\\x{ord(c):02X}" if ord(c) < 0x100 else f"\\u{ord(c):04X}")) for c in s) + '"'
    lead_ok = s != "" and (s[0] not in "-?:,[]{}#&*!|>'\"%@`" or (s[0] in "-?:" and len(s) > 1 and s[1] != " "))
    plain = lead_ok and s == s.strip() and not _IMPLICIT.match(s) and ": " not in s and " #" not in s and not s.endswith(":")
    return s if plain else "'" + s.replace("'", "''") + "'"


def yaml_dump(mapping: dict) -> str:
    """A flat mapping as ``yaml.dump(mapping)`` writes it (keys sorted)."""
    return "".join(f"{k}: {yaml_scalar(mapping[k])}\n" for k in sorted(mapping))


def planning_result(planner: str, puzzle_name: str, status: str, plan: Optional[str], seconds: float,
                    time_limit: Optional[float], valid: bool = True) -> dict:
    """The reference's result mapping of one puzzle (benchmark_rgd.py), from a ``PlannerInfo.status``."""
    out = {"planner": planner, "puzzle": puzzle_name, "planning_time": seconds}
    if status == "solved" and plan is not None:
        if valid:
            out["plan"] = plan
        else:
            out["failure_reason"] = "invalid plan"
            out["plan"] = None
    elif status == "timeout":
        out["failure_reason"] = "time limit reached"
        out["plan"] = None
        out["planning_time"] = time_limit
    elif status == "exhausted":
        out["failure_reason"] = "no solution exists"
        out["plan"] = None
    elif status == "limit":
        out["failure_reason"] = "memory error"
        out["plan"] = None
    else:
        out["failure_reason"] = "unknown"
        out["plan"] = None
    return out


def benchmark_rgd_planner(results_path: str = "nrgd_results", puzzles_path: Optional[str] = None, heuristic: str = "N+RGD",
                          time_limit: Optional[float] = 60 * 30, memory_limit: Optional[float] = 30, batch: int = 1,
                          max_states: Optional[int] = None, action_order: str = "reference") -> dict:
    """Plans every puzzle below ``puzzles_path`` (default: the benchmark's) in one launch and writes one YAML per puzzle.
    ``memory_limit`` (gigabytes per puzzle) sets the store size unless ``max_states`` is given.  Returns the result mappings
    by output path."""
    from .config import BENCHMARK_PUZZLES_PATH, PUZZLE_EXTENSION
    from .puzzle import PushWorldPuzzle
    from .search import REPLAY_VALID, PlanBatch
    from .utils.filesystem import map_files_with_extension

    if heuristic not in PLANNER_NAMES:
        raise ValueError(f'Unknown heuristic: "{heuristic}". Supported values are {list(PLANNER_NAMES)}')
    pairs = list(map_files_with_extension(puzzles_path or BENCHMARK_PUZZLES_PATH, PUZZLE_EXTENSION, results_path, ".yaml"))
    if not pairs:
        return {}
    puzzles = [PushWorldPuzzle(src, order="cpp") for src, _ in pairs]  # (the reference planner's object order)
    if max_states is None:
        n_max = max(p.num_movables for p in puzzles)
        per_state = 4 * ((n_max + 1) // 2) + 25  # store, links, queue links, closed set at half load
        budget = MAX_STATES_CAP if memory_limit is None else int(memory_limit * GIGABYTE) // per_state
        max_states = max(4 * batch + 1, min(MAX_STATES_CAP, budget))
    pb = PlanBatch(puzzles, heuristic=heuristic, batch=batch, max_states=max_states, action_order=action_order)
    try:
        pb.run(time_limit=time_limit)
        verdicts = pb.validate()  # (queued behind the searches; results() waits for both)
        results = pb.results()
        verdicts = verdicts.cpu().numpy()
    finally:
        pb.close()
    out = {}
    for (src, dst), (plan, info, seconds), verdict in zip(pairs, results, verdicts):
        text = None if plan is None else "".join("LRUD"[a] for a in plan)
        valid = text is None or int(verdict) == REPLAY_VALID
        name = os.path.splitext(os.path.split(src)[1])[0]
        result = planning_result(PLANNER_NAMES[heuristic], name, info.status, text, seconds, time_limit, valid)
        with open(dst, "w") as f:
            f.write(yaml_dump(result))
        out[dst] = result
    return out


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m pushworld_amd.benchmark_rgd",
                                 description="Plan every PushWorld puzzle below a directory with RGD / N+RGD best-first search "
                                             "on the GPU (all in one launch) and write one YAML result per puzzle.")
    ap.add_argument("--results-path", default="nrgd_results", help="directory of the YAML results (default: nrgd_results)")
    ap.add_argument("--puzzles-path", default=None, help="a .pwp file or a directory of them (default: the benchmark)")
    ap.add_argument("--heuristic", default="N+RGD", choices=sorted(PLANNER_NAMES), help="default: N+RGD")
    ap.add_argument("--time-limit", type=float, default=60 * 30, help="seconds per puzzle, 0 = none (default: 1800)")
    ap.add_argument("--memory-limit", type=float, default=30, help="gigabytes per puzzle, 0 = none (default: 30)")
    ap.add_argument("--max-states", type=int, default=None, help="states per puzzle (default: from --memory-limit)")
    ap.add_argument("--batch", type=int, default=1, help="states expanded per round, 1 .. 64 (default: 1)")
    ap.add_argument("--actions", choices=("fixed", "reference"), default="reference")
    args = ap.parse_args(argv)
    t0 = time.perf_counter()
    try:
        res = benchmark_rgd_planner(args.results_path, args.puzzles_path, args.heuristic, args.time_limit or None,
                                    args.memory_limit or None, args.batch, args.max_states, args.actions)
    except (ValueError, RuntimeError, OSError) as e:
        sys.stderr.write(f"ERROR: {e}\n")
        return 1
    solved = sum(1 for r in res.values() if r.get("plan"))
    print(f"{solved} / {len(res)} puzzles solved in {time.perf_counter() - t0:.2f} s; results in {args.results_path}")
    return 0


if __name__ == "__main__":
    sys.exit(main())

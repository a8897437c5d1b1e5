"""``python -m pushworld_amd.run_planner <mode> <puzzle.pwp>``: the reference's ``run_planner`` on the GPU.

Parses the puzzle in the C++ object order, runs best-first search (``search.BestFirstSearch``) and prints the plan as a line
of L / R / U / D, or ``NO SOLUTION``.
"""
from __future__ import annotations

import argparse
import sys

USAGE = """\
usage: python -m pushworld_amd.run_planner <mode> <puzzle> [--batch K] [--max-states M] [--actions fixed|reference]
       python -m pushworld_amd.run_planner --pushes <puzzle> [--max-states M]
       python -m pushworld_amd.run_planner --pushes --best-first <puzzle> [--batch K] [--max-states M]

Solves a PushWorld puzzle by best-first search on the GPU and prints the plan as a line of
(L)eft, (R)ight, (U)p, (D)own actions, or "NO SOLUTION" when the puzzle has none.

  <mode>        RGD    order states by the recursive graph distance heuristic
                N+RGD  order states by novelty first, then by RGD
  <puzzle>      a PushWorld puzzle file (.pwp)
  --batch K     states expanded per round (default 1: the reference's order of expansion)
  --max-states  capacity of the state store (default 2^24); the search gives up when it is reached
  --actions     order of the four actions per expanded state: "reference" (default) or "fixed" (L R U D)
  --pushes      breadth-first search over pushes instead (no <mode>): a plan with the fewest pushes
  --best-first  with --pushes: best-first search over pushes in RGD order, K states per round (--batch)
"""


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(add_help=False, usage=USAGE)
    ap.add_argument("mode", nargs="?")
    ap.add_argument("puzzle", nargs="?")
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--max-states", type=int, default=1 << 24)
    ap.add_argument("--actions", choices=("fixed", "reference"), default="reference")
    ap.add_argument("--pushes", action="store_true")
    ap.add_argument("--best-first", action="store_true", dest="best_first")
    ap.add_argument("-h", "--help", action="store_true")
    args = ap.parse_args(argv)
    if args.best_first and not args.pushes:
        sys.stderr.write("ERROR: --best-first needs --pushes\n")
        return 1
    if args.pushes and args.puzzle is None:
        args.mode, args.puzzle = "PUSHES", args.mode
    if args.help or args.mode is None or args.puzzle is None:
        sys.stdout.write(USAGE)
        return 0
    if args.mode not in ("RGD", "N+RGD") and not args.pushes:
        sys.stderr.write(f"ERROR: Unrecognized mode: {args.mode}\n")
        return 1
    from .puzzle import PushWorldPuzzle
    from .search import PushBestFirstSearch, PushBreadthFirstSearch, solve

    try:
        pz = PushWorldPuzzle(args.puzzle, order="cpp")
        if args.pushes and args.best_first:
            with PushBestFirstSearch(pz, batch=args.batch, max_states=min(args.max_states, (1 << 31) - 1)) as search:
                plan = search.solve()
        elif args.pushes:
            with PushBreadthFirstSearch(pz, max_states=min(args.max_states, (1 << 31) - 1)) as search:
                plan = search.solve()
        else:
            plan = solve(pz, args.mode, batch=args.batch, max_states=args.max_states, action_order=args.actions)
    except (ValueError, RuntimeError, OSError) as e:
        sys.stderr.write(f"ERROR: {e}\n")
        return 1
    print("NO SOLUTION" if plan is None else "".join("LRUD"[a] for a in plan))
    return 0


if __name__ == "__main__":
    sys.exit(main())

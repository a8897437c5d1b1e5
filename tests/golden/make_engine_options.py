#!/usr/bin/env python3
"""Recorded answers of pw_engine_set_option / pw_engine_get_option (needs the GPU and the built library): one engine over one
tiny puzzle, and for every option number 0 .. 60 the value a fresh engine reports, then for each probe value the return code of
the set, the text of pw_last_error() where it fails, and the value the get reports afterwards.  The probes are the edges of every
rule of the setter and one step beyond.  A last sweep reads every option once more.  tests/test_gpu_engine_options.py replays
the file.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_engine_options.py [OUT.json]

Run it twice and compare: an entry that differs between two runs depends on the device, not on the code, and does not belong in
the file (none did when this was recorded).
"""
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
from pushworld_amd import _capi  # noqa: E402

PUZZLE = "tests/puzzles/ref_cpp/trivial.pwp"
PPC, BORDER = 3, 1
OPTION_NUMBERS = range(0, 61)  # 1 .. 58 exist; 0, 59 and 60 do not
PROBES = [-2**40, -2, -1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 16, 20, 21, 22, 27, 28, 31, 32, 33, 48, 49, 64, 65, 80, 85, 86, 96,
          1024, 1025, 2047, 2048, 2049, 4096, 4097, 65536, 65537, 100000, 100001, 2**20, 2**20 + 1, 2**31, 2**40]
PROFILE_RENDER = _capi.OPTIONS["profile_render"]  # every accepted launch creates two HIP events: accepted values above 64 are left out


def record(engine):
    lib, h = _capi.lib, engine.handle
    options, messages = {}, []  # (a probe holds the index of its message in `messages`, -1 where the set succeeds)
    for k in OPTION_NUMBERS:
        fresh = int(lib.pw_engine_get_option(h, k))
        probes = []
        for v in PROBES:
            if k == PROFILE_RENDER and 64 < v <= 65536:
                continue
            rc = int(lib.pw_engine_set_option(h, k, v))
            m = -1
            if rc < 0:
                if _capi.last_error() not in messages:
                    messages.append(_capi.last_error())
                m = messages.index(_capi.last_error())
            probes.append([v, rc, m, int(lib.pw_engine_get_option(h, k))])
        options[str(k)] = {"fresh": fresh, "probes": probes}
    final = {str(k): int(lib.pw_engine_get_option(h, k)) for k in OPTION_NUMBERS}
    return {"puzzle": PUZZLE, "pixels_per_cell": PPC, "border_width": BORDER, "messages": messages, "options": options,
            "final": final}


def make_engine():
    with open(os.path.join(REPO, PUZZLE)) as f:
        pset = _capi.PuzzleSet([_capi.ParsedPuzzle(f.read())], 0)
    return _capi.Engine(pset, max_steps=100, pixels_per_cell=PPC, border_width=BORDER, obs_dtype=_capi.OBS_U8)


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "engine_options.json")
    rec = record(make_engine())
    text = json.dumps(rec, sort_keys=True).replace(', "', ',\n"') + "\n"  # (a line per key: the probes of an option stay on one)
    assert json.loads(text) == rec
    with open(out, "w") as f:
        f.write(text)
    print(out, sum(len(o["probes"]) for o in rec["options"].values()), "probes")

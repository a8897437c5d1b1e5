"""pw_engine_set_option / pw_engine_get_option answer as recorded (tests/golden/engine_options.json, written by
tests/golden/make_engine_options.py with the library as it was before the option table, csrc/pw_engine_options.inc): for every
option number 0 .. 60 the value of a fresh engine, then for each probe value the return code of the set, the text of
pw_last_error() where it fails and the value read back, and a last sweep over all options.  Two recordings were identical, entry
for entry: nothing in the file depends on the device.

One difference is meant: the seven read-only options the old setter did not know (it answered "unknown engine option") are
refused like the other read-only ones."""
import json
import os

import pytest

from pushworld_amd import _capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READ_ONLY_NOW = {_capi.OPTIONS[k] for k in ("bind_mismatches", "bind_puzzles", "mailbox_form", "obs_screen_ms", "step_board_set",
                                            "step_one_applies", "step_quad16_puzzles")}


def test_options_answer_as_recorded():
    with open(os.path.join(ROOT, "tests", "golden", "engine_options.json")) as f:
        rec = json.load(f)
    with open(os.path.join(ROOT, rec["puzzle"])) as f:
        pset = _capi.PuzzleSet([_capi.ParsedPuzzle(f.read())], 0)
    engine = _capi.Engine(pset, max_steps=100, pixels_per_cell=rec["pixels_per_cell"], border_width=rec["border_width"],
                          obs_dtype=_capi.OBS_U8)  # (no observation buffer: nothing is rendered)
    lib, h = _capi.lib, engine.handle
    assert sorted(int(k) for k in rec["options"]) == list(range(61)) and sorted(rec["final"]) == sorted(rec["options"])
    probes = 0
    for key, option in sorted(rec["options"].items(), key=lambda kv: int(kv[0])):
        k = int(key)
        assert lib.pw_engine_get_option(h, k) == option["fresh"], (k, "fresh")
        for value, rc, message, got in option["probes"]:
            want = rec["messages"][message] if rc < 0 else ""
            if k in READ_ONLY_NOW:
                assert (rc, want) == (_capi.PW_EINVAL, "unknown engine option"), (k, value)  # (what the file holds for them)
                want = "read-only option"
            assert lib.pw_engine_set_option(h, k, value) == rc, (k, value)
            if rc < 0:
                assert _capi.last_error() == want, (k, value, _capi.last_error())
            assert lib.pw_engine_get_option(h, k) == got, (k, value)
            probes += 1
    for key, got in rec["final"].items():
        assert lib.pw_engine_get_option(h, int(key)) == got, (key, "final")
    assert probes > 2900

"""The shared host plumbing (csrc/pw_hostlib.inc, csrc/pw_hostlib_pure.h): the idioms it replaced occur nowhere else,
``build.HEADERS`` is the directory listing, the argument checks it serves still answer in each entry point's words (through the
loaded library and stand-in pointers: every check returns before anything is read through them, no device memory), and the pure
arithmetic passes a stand-alone host program under the address and undefined-behaviour sanitizers.  And the engine's family files
(csrc/pw_engine*.inc): their include order, and the option table of pw_engine_options.inc against the header and ``_capi.OPTIONS``."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from pushworld_amd import _capi, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pushworld_amd", "csrc")
HOSTLIB = ("pw_hostlib.inc", "pw_hostlib_pure.h")
P = ctypes.c_void_p(4096)  # a stand-in for a pointer
lib = _capi.lib


def _code(name):
    """A source file without its comments (they may name what the code must not hold)."""
    with open(os.path.join(CSRC, name)) as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    return "\n".join(line.split("//")[0] for line in src.splitlines())


def _sources():
    return sorted(f for f in os.listdir(CSRC) if f.endswith((".inc", ".h", ".hip", ".cpp")))


@pytest.mark.parametrize("idiom", ["hipErrorOutOfMemory ? PW_ENOMEM", "npad != 4 && npad != 8", "search_batch_groups_per_cu > 0 ?",
                                   "hipDeviceAttributeWallClockRate", "1.8e19"])
def test_each_idiom_is_written_once(idiom):
    where = [name for name in _sources() if idiom in _code(name)]
    assert len(where) == 1 and where[0] in HOSTLIB, (idiom, where)


# The device half of the batched searches (csrc/pw_batch_set.inc) and their ladder (pw_hostlib_pure.h): each idiom is written in
# its one file.  Two idioms are read as the searches wrote them: pw_seg_kernels.inc, one of the files whose hashes the PMC records
# under profiles/ carry (tools/config_suite.py: not edited), has a `srow` of its own, and `N > 8 ||` is the bare test of a
# kernel's header field (pw_engine.inc asks `h.N > 8 ||` about its 8 x 8 boards on the host).
# LEFT OUT: pw_push_solve_batch_kernel (K22's search kernel, pw_push_solution_batch.inc) keeps the parent's text, so its file still
# holds four of the idioms: with the shared helpers its builds measured about 1 % slower and the cause was not found
# (profiles/batch_closed_set.txt).  Its query kernel and its host half use the shared code.
K22 = ("pw_push_solution_batch.inc",)
@pytest.mark.parametrize("idiom, home, elsewhere", [
    (r"1u << 20,\s*1u << 22", "pw_hostlib_pure.h", ()),
    (r"(?<![.\w])N > 8 \|\|", "pw_batch_set.inc", K22),
    (r"gmask \|= 0xffull", "pw_batch_set.inc", K22),
    (r"atomicCAS\(tab \+ slot, PW_BS_EMPTY", "pw_batch_set.inc", ()),
    (r"== PW_SB_NOROW", "pw_batch_set.inc", K22),
    (r"reinterpret_cast<const uint2\*>\(s?row\)", "pw_batch_set.inc", ("pw_seg_kernels.inc",) + K22),
    (r"guide_lookup", None, ()),
])
def test_each_batched_search_idiom_is_written_once(idiom, home, elsewhere):
    where = [name for name in _sources() if name not in elsewhere and re.search(idiom, _code(name))]
    assert where == ([home] if home else []), (idiom, where)


def test_the_batched_searches_include_their_closed_set():
    unit = _code("pw_kernels.hip")
    assert unit.index('#include "pw_step_kernels.inc"') < unit.index('#include "pw_batch_set.inc"') < unit.index('#include "pw_search.inc"')
    assert "ladder[6]" not in "".join(_code(n) for n in _sources() if n != "pw_hostlib_pure.h")


def test_no_local_copies_of_the_helpers():
    for name in _sources():
        code = _code(name)
        assert "auto alloc = [&]" not in code, name
        if name not in HOSTLIB:
            assert not re.search(r"\+ 255u?\) & ~(static_cast<size_t>|uint64_t)", code), name  # (the rounding lambdas)
            assert not re.search(r"\bcheck_launch\(const char", code), name
    unit = _code("pw_kernels.hip")
    mine = unit.index('#include "pw_hostlib.inc"')
    assert unit.index("struct PwEngine {") < mine < unit.index('#include "pw_step_kernels.inc"') < unit.index('#include "pw_engine.inc"')
    # the engine's family files follow pw_engine.inc in the order their headers name; the option table comes behind pw_mailbox.inc
    engine = [unit.index('#include "%s"' % f) for f in ("pw_engine.inc", "pw_engine_render.inc", "pw_engine_step.inc",
                                                         "pw_engine_step_render.inc", "pw_engine_expand.inc", "pw_engine_obs.inc",
                                                         "pw_engine_plan.inc", "pw_mailbox.inc", "pw_engine_options.inc")]
    assert engine == sorted(engine)
    for name in HOSTLIB:
        code = _code(name)
        assert "__global__" not in code and "__device__" not in code, name
    pure = _code("pw_hostlib_pure.h")
    assert "hip" not in pure and "PwEngine" not in pure
    assert set(re.findall(r"#include [<\"]([^>\"]+)[>\"]", pure)) == {"algorithm", "cstdint"}
    # the second table's checks are the first's, and the two planners' handles share their parts
    assert "push_table_sample_checks" not in _code("pw_push_table_sample.inc")
    for name in ("pw_plan_batch.inc", "pw_push_plan_batch.inc"):
        code = _code(name)
        for used in ("PwSlabPool pool;", "PwCancelWord cancel;", "slab_pool_create(", "slab_pool_grow(", "cancel_word_create(",
                     "cancel_word_cancel(", "cancel_word_destroy(", "pw_wall_clock_khz(", "pw_slot_of(", "pw_puzzles_ok(",
                     "pw_deadline_ticks(", "pw_table_slots(", "PwDeviceGuard guard(b->eng->set->device);\n  if (b->d_items)"):
            assert used in code, (name, used)
    for name in ("pw_search.inc", "pw_solution_batch.inc", "pw_push_solution_batch.inc"):
        assert "engine_search_slab(" in _code(name), name
    assert "pw_wall_clock_khz(" in _code("pw_mailbox.inc")


def test_build_headers_is_the_directory():
    public = os.path.join("..", "..", "include", "pushworld_amd.h")
    want = {f for f in os.listdir(CSRC) if f.endswith((".h", ".inc"))} | {public}
    assert isinstance(build.HEADERS, list) and all(isinstance(h, str) for h in build.HEADERS)
    assert set(build.HEADERS) == want and len(build.HEADERS) == len(want)
    assert {"pw_hostlib.inc", "pw_hostlib_pure.h"} <= want
    for h in build.HEADERS:
        assert os.path.isfile(os.path.join(CSRC, h)), h


# ---- the engine option table (csrc/pw_engine_options.inc): one row per PW_OPT_*, written nowhere else -------------------------------
OPTIONS_FILE = "pw_engine_options.inc"


def _header_options():
    with open(os.path.join(ROOT, "include", "pushworld_amd.h")) as f:
        return {name: int(num) for name, num in re.findall(r"^#define (PW_OPT_\w+) (\d+)\b", f.read(), flags=re.M)}


def test_header_options_are_the_python_options():
    header = _header_options()
    assert len(header) == 58 and len(set(header.values())) == 58
    assert {name[len("PW_OPT_"):].lower(): num for name, num in header.items()} == _capi.OPTIONS


def test_every_option_has_one_table_row():
    code = _code(OPTIONS_FILE)
    table = code[code.index("kOptionRows[] = {"):]
    table = table[:table.index("\n};")]
    rows = re.findall(r"^\s*\{(PW_OPT_\w+),", table, flags=re.M)
    assert sorted(rows) == sorted(_header_options()) and len(rows) == len(set(rows)) == 58
    assert len(re.findall(r"^\s*\{", table, flags=re.M)) == 58  # (and nothing else is a row)


@pytest.mark.parametrize("idiom", ["case PW_OPT_", 'return pw_fail(PW_EINVAL, "read-only option")', '"unknown engine option"'])
def test_option_idioms_live_in_the_option_file(idiom):
    where = [name for name in _sources() if idiom in _code(name)]
    assert where == [OPTIONS_FILE], (idiom, where)


def test_engine_files_need_no_forward_declaration():
    for name in _sources():
        assert not re.search(r"^static [\w ]+\b(rebind_async|live_build|mailbox_form_of)\([^)]*\);", _code(name), flags=re.M), name


# ---- the argument checks, through the library ---------------------------------------------------------------------------------------
def _params(name):
    with open(os.path.join(ROOT, "include", "pushworld_amd.h")) as f:
        src = f.read()
    decl = re.search(r"\bint\s+%s\((.*?)\);" % name, src, re.S)
    assert decl, name
    params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", decl.group(1), flags=re.S).split(",") if p.strip()]
    return [(p, re.search(r"(\w+)$", p).group(1)) for p in params]


class _Handle(ctypes.Structure):
    """The head of a PwPushPlanBatch that never ran and whose puzzles are larger than any npad: what follows the npad check
    answers from the head alone."""
    _fields_ = [("eng", ctypes.c_void_p), ("n", ctypes.c_int32), ("K", ctypes.c_int32), ("max_n", ctypes.c_int32),
                ("rest", ctypes.c_uint8 * 4076)]


def _call(name, **kw):
    """``name`` with stand-ins: pointers P, counts 1, no limits, no stream -- and ``kw`` by parameter name."""
    args = []
    for decl, pname in _params(name):
        if pname in kw:
            args.append(kw[pname])
        elif pname in ("stream", "mask", "lo_n", "hi_n"):
            args.append(None)
        elif "*" in decl:
            args.append(P)
        elif "double" in decl:
            args.append(0.0)
        elif pname == "max_states_each":
            args.append(1 << 12)
        elif pname == "lo":
            args.append(0)
        else:
            args.append(1)
    assert len(args) == len(_capi.SIGNATURES[name][1]), name
    return getattr(lib, name)(*args)


# every entry point with an npad check, and the words its message starts with ("": pw_plan_batch's carry no name)
NPAD_ENTRY_POINTS = [
    ("pw_search_table_query", "pw_search_table_query: "),
    ("pw_solve_batch_query", "pw_solve_batch_query: "),
    ("pw_solve_batch_sample", "pw_solve_batch_sample: "),
    ("pw_search_table_sample", "pw_search_table_sample: "),
    ("pw_plan_batch_run_states", ""),
    ("pw_plan_replay_check", "pw_plan_replay_check: "),
    ("pw_plan_replay_emit", "pw_plan_replay_emit: "),
    ("pw_walk_regions", "pw_walk_regions: "),
    ("pw_walk_pushes", "pw_walk_pushes: "),
    ("pw_push_unroll_count", "pw_push_unroll_count: "),
    ("pw_push_unroll_write", "pw_push_unroll_write: "),
    ("pw_push_search_table_query", "pw_push_search_table_query: "),
    ("pw_push_search_table_sample", "pw_push_search_table_sample: "),
    ("pw_push_search_table_emit", "pw_push_search_table_emit: "),
    ("pw_push_solve_batch_run", "pw_push_solve_batch_run: "),
    ("pw_push_solve_batch_query", "pw_push_solve_batch_query: "),
    ("pw_push_solve_batch_emit", "pw_push_solve_batch_emit: "),
    ("pw_push_plan_batch_run", "pw_push_plan_batch_run: "),
    ("pw_push_plan_batch_run_states", "pw_push_plan_batch_run_states: "),
    ("pw_push_plan_batch_read_states", "pw_push_plan_batch_read_states: "),
]


@pytest.mark.parametrize("name, prefix", NPAD_ENTRY_POINTS)
def test_npad_checks_keep_their_words(name, prefix):
    handle = _Handle()
    handle.max_n = 40
    kw = {}
    if name.startswith("pw_push_plan_batch"):
        kw["b"] = ctypes.cast(ctypes.pointer(handle), ctypes.c_void_p)
    for npad in (0, 12, 64):
        assert _call(name, npad=npad, **kw) == _capi.PW_EINVAL, (name, npad)
        assert _capi.last_error() == prefix + "npad must be 4, 8, 16 or 32", (name, npad, _capi.last_error())
    if name.startswith("pw_push_plan_batch"):  # a good npad passes this check: the next one answers, from the handle's head
        for npad in (4, 8, 16, 32):
            assert _call(name, npad=npad, **kw) == _capi.PW_EINVAL, (name, npad)
            word = "no run yet" if name.endswith("read_states") else "smaller than the largest prepared"
            assert word in _capi.last_error(), (name, npad, _capi.last_error())


def test_every_npad_check_is_listed():
    """An entry point whose file calls pw_check_npad (directly or through the shared checks) is in the table above."""
    listed = {name for name, _ in NPAD_ENTRY_POINTS}
    calls = sum(_code(name).count("pw_check_npad(") for name in _sources() if name not in HOSTLIB)
    assert calls == 13  # the sites; table_sample_checks and the argument checks of walk / replay / unroll each serve two or three
    with open(os.path.join(ROOT, "include", "pushworld_amd.h")) as f:
        header = f.read()
    for name in listed:
        assert re.search(r"\bint\s+%s\(" % name, header) and name in _capi.SIGNATURES, name


@pytest.mark.parametrize("name, out, word", [
    ("pw_solve_batch_sample", "out_row", "null out_row / out_cost"),
    ("pw_search_table_sample", "out_row", "null out_row / out_cost"),
    ("pw_solve_batch_sample", "out_cost", "null out_row / out_cost"),
    ("pw_push_search_table_sample", "out_state", "null out_state / out_cost"),
    ("pw_push_search_table_sample", "out_cost", "null out_state / out_cost"),
])
def test_null_outputs_are_named(name, out, word):
    assert _call(name, npad=8, **{out: None}) == _capi.PW_EINVAL
    assert _capi.last_error() == "%s: %s" % (name, word)


def test_shared_sample_checks_in_both_tables_words():
    for name in ("pw_solve_batch_sample", "pw_search_table_sample", "pw_push_search_table_sample"):
        for kw, word in [(dict(n=0), "n must be >= 1"), (dict(pos=None), "null pos"), (dict(steps=None), "null steps"),
                         (dict(counter=None), "null counter"), (dict(lo_n=P), "the band arrays lo and hi come together"),
                         (dict(lo=3, hi=2), "the cost band needs 0 <= lo <= hi"), (dict(lo=-1, hi=2), "the cost band needs")]:
            assert _call(name, npad=8, **kw) == _capi.PW_EINVAL, (name, kw)
            assert _capi.last_error().startswith(name + ": ") and word in _capi.last_error(), (name, kw, _capi.last_error())


# ---- the pure arithmetic, as a stand-alone host program under the sanitizers -----------------------------------------------------------
def _host_compiler():
    for cand in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        path = shutil.which(cand) if cand else None
        if path:
            return path
    return None


def test_pure_helpers_standalone_sanitized(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "hostlib_pure_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", CSRC, os.path.join(ROOT, "tests", "hostlib_pure_main.cpp"), "-o", exe]
    # the sanitizers' runtimes linked into the program where the compiler has them as archives (gcc; clang's default): the
    # program then runs whatever else the environment loads into every process
    for static in (["-static-libasan", "-static-libubsan"], []):
        built = subprocess.run(cmd + static, capture_output=True, text=True)
        if built.returncode == 0:
            break
    assert built.returncode == 0, built.stdout + built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert ran.returncode == 0 and ran.stdout.strip() == "ok" and not ran.stderr, ran.stdout + ran.stderr

"""pw_rows_chunk_range (csrc/pw_hostlib_pure.h) -- the run -> chunk-range arithmetic of the changed-row render -- as a
stand-alone host program under the sanitizers: tests/rows_range_main.cpp compares it with a byte-by-byte definition on the
frames 51 x 42, 54 x 47, 16 x 16 and 12 x 12, element sizes 1 and 4, every puzzle height and every run of rows."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pushworld_amd", "csrc")


def _host_compiler():
    for cand in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        path = shutil.which(cand) if cand else None
        if path:
            return path
    return None


def test_rows_chunk_range_standalone_sanitized(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "rows_range_main")
    cmd = [cxx, "-std=c++17", "-O2", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-I", CSRC, os.path.join(ROOT, "tests", "rows_range_main.cpp"), "-o", exe]
    # the sanitizers' runtimes linked into the program where the compiler has them as archives (gcc; clang's default)
    for static in (["-static-libasan", "-static-libubsan"], []):
        built = subprocess.run(cmd + static, capture_output=True, text=True)
        if built.returncode == 0:
            break
    assert built.returncode == 0, built.stdout + built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert ran.returncode == 0 and ran.stdout.strip() == "ok" and not ran.stderr, ran.stdout + ran.stderr

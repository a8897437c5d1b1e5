#!/usr/bin/env python3
"""HBM bytes per launch of the dominant (render) kernel from two rocprofv3 PMC passes (FETCH_SIZE and WRITE_SIZE
in separate runs with --kernel-trace only), corrected as MI355X_MICROARCH.md section HBM prescribes: FETCH_SIZE
counts the 128-byte requests of a wide coalesced read as 64 bytes on gfx950, so it is doubled.

    python tools/make_pmc_record.py fetch_results.db write_results.db KERNEL_SUBSTRING envs obs_bytes source > record.json
"""
import hashlib
import json
import os
import re
import sqlite3
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS_KERNEL = "pw_render_rows_kernel"
KERNEL_SOURCE = os.path.join(ROOT, "pushworld_amd", "csrc", "pw_render_kernels.inc")


def kernel_source_sha():
    """sha256 of the render kernels' source: bench.py copies a record into its line only for the source it was
    measured on."""
    with open(KERNEL_SOURCE, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()[:16]


def git_head():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True,
                              timeout=10).stdout.strip() or None
    except Exception:  # noqa: BLE001
        return None


def mean_counter(db, kernel, counter, load_all):
    """Mean of `counter` over the dispatches of the page kernel's instances with / without kLoadAll (the production
    symbol <T, 0, L> and the tuner's <T, 1, L> are the same code): (name of the most frequent symbol, mean, dispatches)."""
    con = sqlite3.connect(db)
    rows = con.execute(
        "select k.name, avg(p.counter_value), count(*) from pmc_events p join kernels k on p.dispatch_id = k.dispatch_id "
        "where p.counter_name = ? group by k.name", (counter,)).fetchall()
    # instances <T, kTag, kLoadAll, kLive>: where the changed-page form (kLive = 3, PW_OPT_OBS_CHANGED_PAGES) ran, the record is
    # that of its launches -- what the step path of a retained buffer runs; what they write depends on the steps --, else of
    # the live-page form (kLive = 1, PW_OPT_OBS_PADDING_ONCE), else of the full render
    def form(name):  # (kLoadAll, kLive) of an instance's symbol
        m = re.search(r"<[^<>]*,\s*(true|false),\s*(\d)>", name)
        return (m.group(1) == "true", int(m.group(2))) if m and kernel in name else None

    # the changed-row launch (pw_render_rows_kernel<T, kNT>, pw_engine_set_obs_changed_rows) stands in the changed-page form's place
    # where it ran: one symbol per dtype, no kLoadAll instances -- the same record under both keys
    rows_form = [r for r in rows if ROWS_KERNEL in r[0]]
    if rows_form:
        total = sum(n for _, _, n in rows_form)
        return max(rows_form, key=lambda r: r[2])[0], sum(val * n for _, val, n in rows_form) / total, total

    # (the form is chosen over both kLoadAll instances: a variant that only the tuner's trials of another form ran gets no record)
    ran = {form(r[0])[1] for r in rows if form(r[0]) is not None}
    best = next((v for v in (3, 1, 0) if v in ran), None)
    sel = [r for r in rows if form(r[0]) == (bool(load_all), best)]
    if not sel:
        return None
    total = sum(n for _, _, n in sel)
    return max(sel, key=lambda r: r[2])[0], sum(val * n for _, val, n in sel) / total, total


def main():
    fetch_db, write_db, kernel, envs, obs_bytes, source = sys.argv[1:7]
    variants = {}
    for load_all in (0, 1):
        f = mean_counter(fetch_db, kernel, "FETCH_SIZE", load_all)
        w = mean_counter(write_db, kernel, "WRITE_SIZE", load_all)
        if f is None or w is None:
            continue
        variants[str(load_all)] = {
            "kernel_symbol": f[0], "hbm_bytes_per_launch": (2.0 * f[1] + w[1]) * 1024.0, "write_size_kb": w[1],
            "fetch_size_kb_raw": f[1], "dispatches": [f[2], w[2]],
        }
    if not variants:
        raise SystemExit(f"no kernel matching {kernel!r} in {fetch_db} / {write_db}")
    rec = {
        "kernel": kernel,
        "envs": int(envs),
        "obs_bytes": int(obs_bytes),
        "by_page_load_all": variants,  # the tuner picks the instance per buffer: bench.py reads the one it runs
        "source": source,
        "kernel_source_sha16": kernel_source_sha(),
        "git_head": git_head(),
        "note": "rocprofv3 --pmc WRITE_SIZE / --pmc FETCH_SIZE (separate passes, --kernel-trace only), mean over all "
                "dispatches of the kernel's instances (production <T, 0, L, V> and the tuner's <T, 1, L, V>: same code; V = 3, the "
                "launches of the changed pages of a retained buffer, where there are any, else V = 1, those of its live pages, "
                "else V = 0, the full render; where the changed-row launch pw_render_rows_kernel ran, its dispatches instead) on the "
                "C3 workload; FETCH_SIZE doubled per MI355X_MICROARCH.md (gfx950 tallies 128-B requests as 64 B)",
    }
    print(json.dumps(rec, indent=1))


if __name__ == "__main__":
    main()

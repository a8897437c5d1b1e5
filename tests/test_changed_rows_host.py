"""The restatement of the changed pixel rows (tests/changed_rows_restatement.py) against the C oracle, the coverage its walks
promise, and the premise of pw_engine_set_obs_changed_rows: the chunks of the changed rows are about 0.4 of the bytes of the
changed pages.

Soundness: over the random walks of tests/test_changed_pages_host.py (autoresets included) every byte outside the TIGHT chunks
is the same oracle byte before and after the step -- so a retained buffer in which only those chunks are written stays right."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import changed_pages_restatement as cp  # noqa: E402
import changed_rows_restatement as cr  # noqa: E402
import live_pages_restatement as lp  # noqa: E402
import test_changed_pages_host as tp  # noqa: E402  (its four walks, its pools and its walker)

WALKS = tp.WALKS
pools = tp.pools  # (the module-scoped fixture, for this module)


def _env_bytes(pool, ids, pos, pad_h, pad_w, es, stride):
    """uint8 [B, stride]: the oracle's observations laid out like a library-owned buffer (zeros behind every image)."""
    from oracle import c_oracle

    obs = c_oracle.observe_batch(pool["oracles"], ids, pos, np.arange(len(ids)), pad_h, pad_w, lp.PPC, lp.BW, "f32" if es == 4 else "u8")
    flat = np.zeros((len(ids), stride), np.uint8)
    raw = obs.reshape(len(ids), -1).view(np.uint8)
    flat[:, :raw.shape[1]] = raw
    return flat


def _check_step(pool, ids, es, frame, shown, new):
    """Bytes outside the tight chunks of the step shown -> new are equal; returns (rows, tight, differs): the changed cell rows, the tight chunk
    set, and the chunks in which the two observations differ."""
    pad_h, pad_w = frame
    stride = lp.frame(pad_h, pad_w, es)[1]
    rows = cp.changed_rows(pool["obj_heights"], ids, pool["heights"], shown, new)
    tight, wide = cr.chunk_sets(pad_h, pad_w, es, pool["heights"], ids, rows)
    before = _env_bytes(pool, ids, shown, pad_h, pad_w, es, stride)
    after = _env_bytes(pool, ids, new, pad_h, pad_w, es, stride)
    differs = (before != after).reshape(len(ids), -1, lp.CHUNK).any(axis=2)
    assert not (differs & ~tight).any(), np.argwhere(differs & ~tight)[0]
    assert not (tight & ~wide).any()
    return rows, tight, differs


@pytest.fixture(scope="module")
def walked(pools):
    out = []
    for k, (name, pad_h, pad_w, dtype, B, steps, max_steps) in enumerate(WALKS):
        pool = pools[name]
        ids = tp._ids(pool, B)
        pos, done = tp._walk(pool, ids, steps, max_steps, 11 + k)
        out.append({"pool": pool, "ids": ids, "es": 1 if dtype == "uint8" else 4, "frame": (pad_h, pad_w), "pos": pos, "done": done})
    return out


@pytest.mark.parametrize("k", range(len(WALKS)), ids=["-".join(map(str, w[:5])) for w in WALKS])
def test_bytes_outside_the_tight_chunks_keep_their_value(walked, k):
    w = walked[k]
    changed = resets = 0
    for t in range(len(w["pos"]) - 1):
        _, _, differs = _check_step(w["pool"], w["ids"], w["es"], w["frame"], w["pos"][t], w["pos"][t + 1])
        changed += int(differs.sum())
        resets += int(w["done"][t - 1].sum()) if t > 0 else 0
    assert changed > 0 and resets > 0  # (the check looked at something, autoreset steps among it)


def test_the_walks_hold_the_promised_cases(walked):
    seen = set()
    for w in walked:
        pool, ids, pos, done = w["pool"], w["ids"], w["pos"], w["done"]
        for t in range(len(pos) - 1):
            reset = done[t - 1] if t > 0 else np.zeros(len(ids), bool)
            moved = (pos[t] != pos[t + 1]).any(axis=2)
            rows = cp.changed_rows(pool["obj_heights"], ids, pool["heights"], pos[t], pos[t + 1])
            if (~moved.any(axis=1) & ~reset).any():
                seen.add("a step with no move")
            # (the agent moves with what it pushes: three or more moved entries outside an autoreset = it pushed at least two)
            if ((moved.sum(axis=1) >= 3) & ~reset).any():
                seen.add("a push of two or more objects")
            if reset.any():
                seen.add("an autoreset")
            for e in np.flatnonzero(moved.any(axis=1)):
                hs = np.array(pool["obj_heights"][ids[e]])
                if w["frame"] == (51, 42) and (hs[moved[e, :len(hs)]] > 3).any():
                    seen.add("an object taller than one pass")
                if len(cr.runs_of(rows[e])) >= 2:
                    seen.add("two separate runs of rows in one environment")
    assert seen == {"a step with no move", "a push of two or more objects", "an autoreset", "an object taller than one pass",
                    "two separate runs of rows in one environment"}


def test_two_separate_runs_by_hand(pools):
    """Two movables of one environment change in rows far apart (positions set by a caller): two runs, and the bytes between
    them keep their value."""
    pool = pools["level1"]
    p = next(i for i, hs in enumerate(pool["obj_heights"]) if len(hs) >= 2 and pool["heights"][i] >= 8)
    ids = np.array([p], dtype=np.int64)
    o = pool["oracles"][p]
    shown = cp.positions_of(pool["oracles"], ids, [o.initial_state], pool["np"])
    new = shown.copy()
    hs = pool["obj_heights"][p]
    H = int(pool["heights"][p])
    new[0, 0, 1] = 0          # the agent into the top row ...
    new[0, 1, 1] = H - hs[1]  # ... and movable 1 down to the last rows
    for es in (1, 4):
        rows, tight, _ = _check_step(pool, ids, es, (51, 42), shown, new)
        assert len(cr.runs_of(rows[0])) >= 2
        assert tight.any() and not tight.all()


def test_the_changed_rows_are_about_two_fifths_of_the_changed_pages(pools):
    """The premise, on the C3 frame (51 x 42, uint8) over all 68 Level-1 puzzles: 0.39 by rows, before chunk rounding."""
    pool = pools["level1"]
    ids = tp._ids(pool, 68 * 3)
    pos, _ = tp._walk(pool, ids, 60, 200, 5)
    chunk_bytes = page_bytes = 0
    for t in range(60):
        rows = cp.changed_rows(pool["obj_heights"], ids, pool["heights"], pos[t], pos[t + 1])
        tight, _ = cr.chunk_sets(51, 42, 1, pool["heights"], ids, rows)
        pages, _, _ = cp.page_sets(51, 42, 1, pool["heights"], ids, rows)
        chunk_bytes += int(tight.sum()) * lp.CHUNK
        page_bytes += int(pages.sum()) * cp.PAGE
    share = chunk_bytes / page_bytes
    assert 0.33 <= share <= 0.45, share

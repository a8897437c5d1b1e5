"""The restatement of the changed pages (tests/changed_pages_restatement.py) against the C oracle, the coverage its walks
promise, and the premise of PW_OPT_OBS_CHANGED_PAGES: a step changes under a third of the live pages.

Soundness: over random walks (autoresets included) every page outside the TIGHT set holds the same oracle bytes before and
after the step -- so a retained buffer in which only those pages are written stays right."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import changed_pages_restatement as cp  # noqa: E402
import live_pages_restatement as lp  # noqa: E402

# (pool, pad_h, pad_w, dtype, B, steps, max_steps)
WALKS = [("level1", 51, 42, "uint8", 136, 24, 10), ("level1", 51, 42, "float32", 12, 12, 5),
         ("small", 16, 16, "uint8", 300, 12, 5), ("small", 12, 12, "float32", 37, 12, 5)]


@pytest.fixture(scope="module")
def pools():
    from oracle import c_oracle

    out = {}
    for name, texts in lp.POOLS.items():
        texts = texts()
        oracles = [c_oracle.COraclePuzzle(t) for t in texts]
        out[name] = {"oracles": oracles, "heights": lp.text_heights(texts), "np": max(o.num_movables for o in oracles),
                     "obj_heights": cp.obj_heights_of(oracles)}
    return out


def _ids(pool, B):
    n = len(pool["oracles"])
    return (np.arange(B, dtype=np.int64) * n) // B if B >= n else np.arange(B, dtype=np.int64) * (n // B)


def _walk(pool, ids, steps, max_steps, seed):
    """pos int8 [steps + 1, B, NP, 2] (the initial states first), terminated | truncated [steps, B]."""
    from oracle import c_oracle

    rng = np.random.default_rng(seed)
    actions = rng.integers(0, 4, (steps, len(ids))).astype(np.uint8)
    pos, _, term, trunc, _ = c_oracle.rollout_trace(pool["oracles"], ids, actions, max_steps, True, pool["np"])
    init = cp.positions_of(pool["oracles"], ids, [pool["oracles"][p].initial_state for p in ids], pool["np"])
    return np.concatenate([init[None], pos]), (term | trunc).astype(bool)


def _flat_obs(pool, ids, pos, pad_h, pad_w, es, stride):
    from oracle import c_oracle

    obs = c_oracle.observe_batch(pool["oracles"], ids, pos, np.arange(len(ids)), pad_h, pad_w, lp.PPC, lp.BW, "f32" if es == 4 else "u8")
    flat = np.zeros((len(ids), stride), np.uint8)
    raw = obs.reshape(len(ids), -1).view(np.uint8)
    flat[:, :raw.shape[1]] = raw
    n_pages = -(-flat.size // cp.PAGE)
    out = np.zeros(n_pages * cp.PAGE, np.uint8)
    out[:flat.size] = flat.reshape(-1)
    return out.reshape(n_pages, cp.PAGE)


@pytest.fixture(scope="module")
def walks(pools):
    """Per walk and step: (tight, wide, live, rows, moved movables per environment, done before the step)."""
    out = []
    for k, (name, pad_h, pad_w, dtype, B, steps, max_steps) in enumerate(WALKS):
        pool = pools[name]
        ids = _ids(pool, B)
        es = 1 if dtype == "uint8" else 4
        pos, done = _walk(pool, ids, steps, max_steps, 11 + k)
        per_step = []
        for t in range(steps):
            rows = cp.changed_rows(pool["obj_heights"], ids, pool["heights"], pos[t], pos[t + 1])
            tight, wide, live = cp.page_sets(pad_h, pad_w, es, pool["heights"], ids, rows)
            moved = (pos[t] != pos[t + 1]).any(axis=2)  # [B, NP]
            per_step.append({"tight": tight, "wide": wide, "live": live, "rows": rows, "moved": moved,
                             "reset": done[t - 1] if t > 0 else np.zeros(B, bool)})
        out.append({"pool": pool, "ids": ids, "es": es, "pos": pos, "steps": per_step, "frame": (pad_h, pad_w)})
    return out


@pytest.mark.parametrize("k", range(len(WALKS)), ids=["-".join(map(str, w[:5])) for w in WALKS])
def test_pages_outside_the_tight_set_keep_their_bytes(walks, k):
    w = walks[k]
    pad_h, pad_w = w["frame"]
    stride = lp.frame(pad_h, pad_w, w["es"])[1]
    before = _flat_obs(w["pool"], w["ids"], w["pos"][0], pad_h, pad_w, w["es"], stride)
    changed_pages = resets = 0
    for t, s in enumerate(w["steps"]):
        after = _flat_obs(w["pool"], w["ids"], w["pos"][t + 1], pad_h, pad_w, w["es"], stride)
        differs = (before != after).any(axis=1)
        assert not (differs & ~s["tight"]).any(), (t, int(np.flatnonzero(differs & ~s["tight"])[0]))
        assert not (s["tight"] & ~s["wide"]).any() and not (s["wide"] & ~s["live"]).any()
        changed_pages += int(differs.sum())
        resets += int(s["reset"].sum())
        before = after
    assert changed_pages > 0 and resets > 0  # (the check looked at something, autoreset steps among it)


def test_the_walks_hold_the_promised_cases(walks):
    seen = set()
    for w in walks:
        pad_h, pad_w = w["frame"]
        parts = lp.page_parts(pad_h, pad_w, w["es"], w["pool"]["heights"], w["ids"])
        row_bytes = pad_w * lp.PPC * 3 * w["es"]
        page_cell_rows = cp.PAGE / (lp.PPC * row_bytes)
        strad = np.flatnonzero(~parts["whole"] & parts["has_head"])
        for s in w["steps"]:
            any_row = s["rows"].any(axis=1)
            if (~s["moved"].any(axis=1) & ~s["reset"]).any():
                seen.add("a step with no move")
            if ((s["moved"].sum(axis=1) >= 3) & ~s["reset"]).any():
                seen.add("a push of two or more objects")
            if s["reset"].any():
                seen.add("an autoreset")
            for e in np.flatnonzero(s["moved"].any(axis=1)):
                hs = np.array(w["pool"]["obj_heights"][w["ids"][e]])
                if (hs[s["moved"][e, :len(hs)]] > page_cell_rows).any():
                    seen.add("an object taller than one page's rows")
            e0 = parts["env"][strad]
            if (s["tight"][strad] & any_row[e0] & ~any_row[e0 + 1]).any():
                seen.add("a change only in env0 of a straddling page")
            if (s["tight"][strad] & ~any_row[e0] & any_row[e0 + 1]).any():
                seen.add("a change only in env1 of a straddling page")
    assert seen == {"a step with no move", "a push of two or more objects", "an autoreset", "an object taller than one page's rows",
                    "a change only in env0 of a straddling page", "a change only in env1 of a straddling page"}


def test_a_step_changes_under_a_third_of_the_live_pages(pools):
    """The premise, on the C3 frame (51 x 42, uint8) over all 68 Level-1 puzzles: measured 0.29 with uniform random actions."""
    pool = pools["level1"]
    ids = _ids(pool, 68 * 3)
    pos, _ = _walk(pool, ids, 60, 200, 5)
    tight_n = live_n = 0
    for t in range(60):
        rows = cp.changed_rows(pool["obj_heights"], ids, pool["heights"], pos[t], pos[t + 1])
        tight, _, live = cp.page_sets(51, 42, 1, pool["heights"], ids, rows)
        tight_n += int(tight.sum())
        live_n += int(live.sum())
    share = tight_n / live_n
    print("tight / live =", share)
    assert 0.25 <= share <= 0.35, share

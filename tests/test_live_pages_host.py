"""The restatement of the live pages (tests/live_pages_restatement.py) against the C oracle, and the coverage its cases promise.

Soundness: whatever the state, every byte of an observation that the live launch does NOT store is zero in the oracle's image --
so a retained buffer whose padding was written once stays right.  Coverage: the cases hold every kind of page and every count of
live pages the GPU tests are meant to run; asserted here so that a later change of seeds cannot silently lose one."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import live_pages_restatement as lp  # noqa: E402

STATES = 8  # seeded random states per environment, on top of the initial one


@pytest.fixture(scope="module")
def pools():
    from oracle import c_oracle

    out = {}
    for name, texts in lp.POOLS.items():
        texts = texts()
        oracles = [c_oracle.COraclePuzzle(t) for t in texts]
        heights = lp.text_heights(texts)
        assert heights.tolist() == [o.height for o in oracles]
        out[name] = {"oracles": oracles, "heights": heights, "np": max(o.num_movables for o in oracles)}
    l1 = out["level1"]["oracles"]
    assert len(l1) == 68 and (l1[lp.BIG].height, l1[lp.BIG].width) == (51, 42) and (l1[lp.SMALL].height, l1[lp.SMALL].width) == (5, 6)
    assert [(o.height, o.width) for o in out["small"]["oracles"]] == [(5, 4), (8, 7), (12, 12)]
    return out


def _parts(pools, c):
    pool = pools[c.pool]
    ids = lp.case_ids(c, len(pool["oracles"]))
    return lp.page_parts(c.pad_h, c.pad_w, lp.case_es(c), pool["heights"], ids), ids


def test_the_cases_are_the_ones_promised(pools):
    assert len(lp.CASES) == 3 * 7 + 4 * 8 and len(set(lp.CASES)) == len(lp.CASES)
    for c in lp.CASES:
        ids = lp.case_ids(c, len(pools[c.pool]["oracles"]))
        assert ids.shape == (c.B,) and np.array_equal(ids, lp.case_ids(c, len(pools[c.pool]["oracles"])))  # seeded
        if c.pool == "level1" and c.B > 1:
            assert lp.SMALL in ids and lp.BIG in ids
        if c.pool == "small" and c.B > 2:
            assert set(ids.tolist()) == {0, 1, 2}
    strides = sorted({lp.frame(c.pad_h, c.pad_w, 1)[1] for c in lp.CASES if c.pool == "small"})
    assert strides == [4096, 4608, 5632, 7168]
    cpes = sorted({lp.frame(c.pad_h, c.pad_w, 4)[2] for c in lp.CASES if c.pool == "small"})
    assert cpes[0] == 992 and cpes[-1] == 1728


def _old_pages(heights, ids, es):
    from test_gpu_obs_padding import _pages

    return _pages(heights, ids, es)


@pytest.mark.parametrize("es", [1, 4])
@pytest.mark.parametrize("B", [1, 3, 50, 4096])
def test_it_equals_the_restatement_of_the_level1_frame(pools, B, es):
    from test_gpu_obs_padding import PAD_H, PAD_W, _ids

    heights = pools["level1"]["heights"]
    ids = _ids(B, len(heights))
    live, whole, n_pages, stride, obs_bytes = lp.pages(PAD_H, PAD_W, es, heights, ids)
    want_live, want_whole, want_pages = _old_pages(heights, ids, es)
    assert n_pages == want_pages and np.array_equal(live, want_live) and np.array_equal(whole, want_whole)
    assert obs_bytes == 153 * 126 * 3 * es and stride == {1: 57856, 4: 231424}[es]
    # ... and for seeded ids, where the neighbours of a straddling page are any two puzzles
    ids = np.random.default_rng(B + es).integers(0, len(heights), B)
    got, want = lp.pages(PAD_H, PAD_W, es, heights, ids), _old_pages(heights, ids, es)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def _random_pos(rng, pool, ids, count):
    """int8 [count, B, NP, 2]: every movable anywhere inside its puzzle's grid (borders included), overlaps allowed."""
    pos = np.zeros((count, len(ids), pool["np"], 2), np.int8)
    for p in np.unique(ids):
        o = pool["oracles"][p]
        envs = np.flatnonzero(ids == p)
        for j, (w, h) in enumerate(o.py.sizes):
            pos[:, envs, j, 0] = rng.integers(0, o.width - w + 1, (count, len(envs)))
            pos[:, envs, j, 1] = rng.integers(0, o.height - h + 1, (count, len(envs)))
    return pos


@pytest.mark.parametrize("c", lp.CASES, ids=lp.case_id)
def test_what_the_live_launch_leaves_alone_is_zero_in_every_state(pools, c):
    from oracle import c_oracle

    pool = pools[c.pool]
    ids = lp.case_ids(c, len(pool["oracles"]))
    es = lp.case_es(c)
    live, _, n_pages, stride, obs_bytes = lp.pages(c.pad_h, c.pad_w, es, pool["heights"], ids)
    cpe = stride // 16
    rng = np.random.default_rng(c.B + 7 * es)
    init = np.zeros((1, c.B, pool["np"], 2), np.int8)
    for e, p in enumerate(ids):
        xy = np.array(pool["oracles"][p].initial_state, np.int8)
        init[0, e, :len(xy)] = xy
    pos = np.concatenate([init, _random_pos(rng, pool, ids, STATES)])
    drawn = 0
    for e0 in range(0, c.B, 512):  # (blocks of environments: the big batches need not be in memory at once)
        e1 = min(c.B, e0 + 512)
        sel = np.arange(e0, e1)
        seen = np.zeros((e1 - e0, stride), np.uint8)  # the oracle's observations laid out at the stride, OR-ed over the states
        for s in range(len(pos)):
            obs = c_oracle.observe_batch(pool["oracles"], ids, pos[s], sel, c.pad_h, c.pad_w, lp.PPC, lp.BW, "f32" if es == 4 else "u8")
            flat = obs.reshape(e1 - e0, -1).view(np.uint8)
            assert flat.shape[1] == obs_bytes
            np.maximum(seen[:, :obs_bytes], flat, out=seen[:, :obs_bytes])
        drawn += int(np.count_nonzero(seen.any(axis=1)))
        p0, p1 = e0 * cpe // 256, -(-(e1 * cpe) // 256)
        m = lp.written_mask(c.pad_h, c.pad_w, es, pool["heights"], ids, live=live, first_page=p0, count=p1 - p0, chunks=True)
        m = m[e0 * cpe - p0 * 256:e1 * cpe - p0 * 256]
        nonzero = seen.reshape(-1, 16).any(axis=1)
        bad = np.flatnonzero(nonzero & ~m)
        assert bad.size == 0, (lp.case_id(c), e0 + int(bad[0]) // cpe, int(bad[0]) % cpe)
    assert drawn == c.B  # (every image has pixels: the check looked at something)


def test_the_byte_mask_is_the_chunk_mask(pools):
    c = next(k for k in lp.CASES if k.pool == "small" and k.dtype == "float32" and k.B == 37)
    pool = pools[c.pool]
    ids = lp.case_ids(c, 3)
    live, _, n_pages, stride, obs_bytes = lp.pages(c.pad_h, c.pad_w, 4, pool["heights"], ids)
    by = lp.written_mask(c.pad_h, c.pad_w, 4, pool["heights"], ids)
    ch = lp.written_mask(c.pad_h, c.pad_w, 4, pool["heights"], ids, chunks=True)
    assert by.shape == (n_pages * 4096,) and by.dtype == bool and np.array_equal(by.reshape(-1, 16).all(axis=1), ch)
    assert not by.reshape(-1, 4096)[~live].any() and by.reshape(-1, 4096)[live].any(axis=1).all()
    per_env = by[:c.B * stride].reshape(c.B, stride)
    assert not per_env[:, -(-obs_bytes // 16) * 16:].any()  # the gap behind an image is never stored
    assert not by[c.B * stride:].any()                      # nor anything behind the last environment


def test_the_cases_cover_every_kind_of_page_and_count(pools):
    seen = set()
    for c in lp.CASES:
        p, ids = _parts(pools, c)
        live, whole, n_live = p["live"], p["whole"], int(p["live"].sum())
        if c.pool == "level1" or c.dtype == "float32":
            if (whole & ~live).any():
                seen.add("whole dead page")
            if (~whole & p["has_head"] & ~live).any():
                seen.add("straddling dead page")
            if (~whole & p["has_head"] & p["tail_live"] & ~p["head_live"]).any():
                seen.add("straddling page live through its tail only")
            if (~whole & p["has_head"] & ~p["tail_live"] & p["head_live"]).any():
                seen.add("straddling page live through its head only")
            if len(set(((c.pad_h - pools[c.pool]["heights"][ids]) % 2).tolist())) == 2:
                seen.add("odd and even pad_h - H in one batch")
        if 0 < n_live < 8:
            seen.add("n_live < 8")
        if n_live % 8 != 0 and n_live % 512 != 0:
            seen.add("n_live no multiple of 8 or 512")
        if n_live > 512 and n_live % 512 != 0:
            seen.add("more than one span of 512, the last one short")
        if n_live == p["n_pages"] and c.pool == "small" and c.dtype == "uint8" and c.B > 1:
            seen.add("every page live")
        if p["cpe"] % 256 == 0:
            seen.add("cpe % 256 == 0")
        if p["cpe"] == 256 and p["n_chunks"] < 256:
            seen.add("cpe == 256 with n_chunks < 256")
        if p["cpe"] == 288:
            seen.add("cpe == 288")
        if c.B > 1:
            assert 0 < n_live
    assert seen == {"whole dead page", "straddling dead page", "straddling page live through its tail only",
                    "straddling page live through its head only", "odd and even pad_h - H in one batch", "n_live < 8",
                    "n_live no multiple of 8 or 512", "more than one span of 512, the last one short", "every page live",
                    "cpe % 256 == 0", "cpe == 256 with n_chunks < 256", "cpe == 288"}
    # the C4 frame at float32: no page straddles two environments
    for c in lp.CASES:
        p, _ = _parts(pools, c)
        if (c.pad_h, c.pad_w, c.dtype) == (54, 47, "float32"):
            assert p["cpe"] % 256 == 0 and not p["has_head"].any()

"""The live pages of a retained observation buffer (PW_OPT_OBS_PADDING_ONCE), restated in plain numpy -- a helper module for
tests/test_live_pages_host.py and tests/test_gpu_obs_padding_frames.py, which share the cases defined at the end.

From the header's wording of the rule (include/pushworld_amd.h, option 53), for ppc 3: the buffer is a flat run of 16-byte
chunks, `cpe` of them per environment (the stride of the library's own buffers: the observation rounded up to 512 bytes), cut
into 4 KiB pages of 256 chunks.  The full render stores the chunks c < n_chunks of every environment (those that hold bytes
of its image) and nothing in the gap [n_chunks, cpe).  A puzzle of H cell rows is centred in the frame: its own pixel rows
are [top, top + 3 H) with top = (pad_h - H) * 3 // 2, everything above and below is zero in every state.  A page is LIVE iff
at least one of the chunks stored in it holds a byte of a puzzle's own pixel rows; the live launch stores, in the live pages
only, exactly what the full render stores there.  Nothing here follows the kernels' case split (whole page / tail + head):
a page is looked at as the one or two runs of chunks of one environment each that it is made of."""
from collections import namedtuple

import numpy as np

PPC, BW = 3, 1             # every case: 3 pixels per cell, border width 1
PAGE_CHUNKS, CHUNK = 256, 16


def frame(pad_h, pad_w, es):
    """(obs_bytes, stride, cpe, n_chunks) of a pad_h x pad_w cell frame with elements of `es` bytes."""
    obs_bytes = (pad_h * PPC) * (pad_w * PPC) * 3 * es
    stride = -(-obs_bytes // 512) * 512
    return obs_bytes, stride, stride // CHUNK, -(-obs_bytes // CHUNK)


def own_chunks(pad_h, pad_w, es, H):
    """[lo, hi): the chunks of an environment's image that hold a byte of the puzzle's own pixel rows (H: array of heights)."""
    row_bytes = pad_w * PPC * 3 * es
    top = (pad_h - H) * PPC // 2
    return (top * row_bytes) // CHUNK, -(-((top + PPC * H) * row_bytes) // CHUNK)


def page_parts(pad_h, pad_w, es, heights, ids):
    """Per page: the run of chunks of its first environment (`tail`) and, where the page reaches into the next one, of that
    (`head`); which of the two hold stored chunks of a puzzle's own rows; and whether all 256 chunks are stored chunks of one
    environment (`whole`)."""
    obs_bytes, stride, cpe, n_chunks = frame(pad_h, pad_w, es)
    ids = np.asarray(ids, dtype=np.int64)
    B = len(ids)
    n_pages = -(-(B * cpe) // PAGE_CHUNKS)
    lo, hi = own_chunks(pad_h, pad_w, es, np.asarray(heights, dtype=np.int64)[ids])
    first = np.arange(n_pages, dtype=np.int64) * PAGE_CHUNKS   # global chunk a page starts with
    env = first // cpe
    a = first - env * cpe                                      # ... as a chunk of that environment
    # the first environment's run [a, min(a + 256, cpe)), of which [.., n_chunks) is stored
    tail_live = np.maximum(a, lo[env]) < np.minimum(np.minimum(a + PAGE_CHUNKS, n_chunks), hi[env])
    # the next environment's run [0, a + 256 - cpe), where there is a next environment
    reach = a + PAGE_CHUNKS - cpe
    has_head = (reach > 0) & (env + 1 < B)
    nxt = np.minimum(env + 1, B - 1)
    head_live = has_head & (lo[nxt] < np.minimum(np.minimum(reach, n_chunks), hi[nxt]))
    return {"n_pages": n_pages, "stride": stride, "obs_bytes": obs_bytes, "cpe": cpe, "n_chunks": n_chunks, "env": env,
            "whole": a + PAGE_CHUNKS <= n_chunks, "has_head": has_head, "tail_live": tail_live, "head_live": head_live,
            "live": tail_live | head_live}


def pages(pad_h, pad_w, es, heights, ids):
    """(live mask, whole-page mask, pages, stride, obs_bytes) of a library-owned buffer of the batch `ids`."""
    p = page_parts(pad_h, pad_w, es, heights, ids)
    return p["live"], p["whole"], p["n_pages"], p["stride"], p["obs_bytes"]


def written_mask(pad_h, pad_w, es, heights, ids, live=None, first_page=0, count=None, chunks=False, arange=np.arange):
    """True for the bytes the live launch stores: every chunk c < n_chunks of an environment of the batch that lies in a live
    page.  One flag per byte of the pages [first_page, first_page + count) (default: all n_pages * 4096 bytes), or per chunk
    with `chunks`.  `live` / `arange`: the live mask and an arange of another array library (a torch device), for big buffers."""
    _, _, cpe, n_chunks = frame(pad_h, pad_w, es)
    if live is None:
        live = pages(pad_h, pad_w, es, heights, ids)[0]
    count = len(live) - first_page if count is None else count
    g = arange(first_page * PAGE_CHUNKS, (first_page + count) * PAGE_CHUNKS)
    env = g // cpe
    m = live[g // PAGE_CHUNKS] & (g - env * cpe < n_chunks) & (env < len(ids))
    return m if chunks else np.repeat(m, CHUNK)


# ---- the pools --------------------------------------------------------------------------------------------------------
BIG, SMALL = 40, 36  # Level-1 pool indices of the 51 x 42 puzzle and of the 5 x 6 one


def level1_texts():
    import bench

    return [open(p).read() for p in bench.level1_paths()]


def small_texts():
    """Three hand-made puzzles of 5 x 4, 8 x 7 and 12 x 12 cells, borders included: the agent left of a box, its goal two cells
    on, and a wall in the far corner where there is room."""
    out = []
    for H, W in ((5, 4), (8, 7), (12, 12)):
        rows, cols = H - 2, W - 2
        grid = [["."] * cols for _ in range(rows)]
        if cols >= 4:
            grid[rows // 2][0:4] = ["A", "M1", ".", "G1"]
            grid[rows - 1][cols - 1] = "W"
        else:
            grid[0][0], grid[1][0], grid[2][0] = "A", "M1", "G1"
        out.append("\n".join("  ".join(r) for r in grid) + "\n")
    return out


def text_heights(texts):
    """Cell rows of every puzzle, the two border rows included."""
    return np.array([sum(1 for line in t.splitlines() if line.strip()) + 2 for t in texts], dtype=np.int64)


POOLS = {"level1": level1_texts, "small": small_texts}

# ---- the cases --------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "pool pad_h pad_w dtype B")


def _cases():
    out = []
    for pad in ((54, 47), (52, 43), (57, 42)):
        for dtype in ("uint8", "float32"):
            out += [Case("level1", pad[0], pad[1], dtype, B) for B in (1, 3, 50)]
        out.append(Case("level1", pad[0], pad[1], "uint8", 4096))
    for pad in ((12, 12), (13, 12), (16, 12), (16, 16)):
        for dtype in ("uint8", "float32"):
            out += [Case("small", pad[0], pad[1], dtype, B) for B in (1, 2, 37, 300)]
    return out


CASES = _cases()


def case_id(c):
    return f"{c.pool}-{c.pad_h}x{c.pad_w}-{c.dtype}-B{c.B}"


def case_es(c):
    return 1 if c.dtype == "uint8" else 4


def case_ids(c, n_pool):
    """The seeded puzzle assignment of a case.  Level-1: the 5 x 6 and the 51 x 42 puzzle are in every batch (a batch of one
    holds the small one at uint8, the big one at float32); small pool: every puzzle is in every batch that has room."""
    rng = np.random.default_rng([c.pad_h, c.pad_w, case_es(c), c.B])
    if c.pool == "level1":
        if c.B == 1:
            return np.array([SMALL if c.dtype == "uint8" else BIG], dtype=np.int64)
        must = [SMALL, BIG]
    else:
        if c.B == 1:
            return np.array([(c.pad_h + c.pad_w + case_es(c)) % n_pool], dtype=np.int64)
        must = list(range(n_pool))[:c.B]
    ids = rng.integers(0, n_pool, c.B)
    ids[rng.choice(c.B, len(must), replace=False)] = rng.permutation(must)
    return ids.astype(np.int64)

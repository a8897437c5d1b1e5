"""The changed pages of a retained observation buffer (PW_OPT_OBS_CHANGED_PAGES), restated in plain numpy -- a helper module
for tests/test_changed_pages_host.py and tests/test_gpu_obs_changed.py, on top of tests/live_pages_restatement.py.

From the header's wording (include/pushworld_amd.h, option 58), for ppc 3: the engine knows the positions the buffer SHOWS.
A movable whose new position differs from the shown one changes the cell rows it leaves and enters, [y_old, y_old + h) and
[y_new, y_new + h); every row when a y lies outside 0 .. 63.  Cell row r of a puzzle of H rows is the pixel rows
[top + 3 r, top + 3 r + 3) of the frame, top = (pad_h - H) * 3 // 2.  Of the live pages
  * the TIGHT set holds a byte of a changed cell row's three pixel rows: the launch must write these;
  * the WIDE set is the same with one cell row added on either side: the launch may write no page outside it
(the kernel looks at zone entries of 9 channels, which reach a few bytes across a row boundary).  Nothing here follows the
kernel's case split or its arithmetic: every environment's changed pixel rows become a byte range of the flat buffer."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import live_pages_restatement as lp  # noqa: E402

PAGE = lp.PAGE_CHUNKS * lp.CHUNK


def changed_rows(obj_heights, ids, puzzle_heights, shown, new):
    """bool [B, 64]: the cell rows of every environment in which the picture of `new` may differ from that of `shown` (int8
    [B, NP, 2] each).  obj_heights[p] = heights of puzzle p's movables in cells."""
    shown, new = np.asarray(shown, dtype=np.int64), np.asarray(new, dtype=np.int64)
    B = len(ids)
    rows = np.zeros((B, 64), dtype=bool)
    for e in range(B):
        for j, h in enumerate(obj_heights[ids[e]]):
            if tuple(shown[e, j]) == tuple(new[e, j]):
                continue
            for y in (shown[e, j, 1], new[e, j, 1]):
                if not 0 <= y < 64:
                    rows[e, :] = True
                else:
                    rows[e, y:min(y + h, 64)] = True
        rows[e, puzzle_heights[ids[e]]:] = False  # (rows below the puzzle do not exist)
    return rows


def page_sets(pad_h, pad_w, es, puzzle_heights, ids, rows):
    """(tight, wide, live): page masks of a library-owned buffer of the batch `ids` whose environments changed in `rows`."""
    live, _, n_pages, stride, obs_bytes = lp.pages(pad_h, pad_w, es, puzzle_heights, ids)
    row_bytes = pad_w * lp.PPC * 3 * es
    out = []
    for margin in (0, 1):
        hit = np.zeros(n_pages, dtype=bool)
        for e in range(len(ids)):
            H = int(puzzle_heights[ids[e]])
            top = (pad_h - H) * lp.PPC // 2
            for r in np.flatnonzero(rows[e]):
                r0, r1 = int(r) - margin, int(r) + 1 + margin  # (the margin may be a cell row of the frame padding)
                b0 = e * stride + max((top + lp.PPC * r0) * row_bytes, 0)
                b1 = e * stride + min((top + lp.PPC * r1) * row_bytes, obs_bytes)
                hit[b0 // PAGE:(b1 - 1) // PAGE + 1] = True
        out.append(hit & live)
    return out[0], out[1], live


def obj_heights_of(oracles):
    return [[h for (_w, h) in o.py.sizes] for o in oracles]


def positions_of(oracles, ids, states, np_pad):
    """int8 [B, np_pad, 2] from a list of oracle states (tuples of (x, y))."""
    pos = np.zeros((len(ids), np_pad, 2), np.int8)
    for e, s in enumerate(states):
        xy = np.array(s, np.int8).reshape(-1, 2)
        pos[e, :len(xy)] = xy
    return pos

"""The changed pixel rows of a retained observation buffer (pw_engine_set_obs_changed_rows), restated in plain numpy -- a helper
module for tests/test_changed_rows_host.py and tests/test_gpu_obs_rows.py, on top of tests/changed_pages_restatement.py.

From the header's wording (include/pushworld_amd.h), for ppc 3: with the switch on a step rewrites, per environment, the 16-byte
chunks that hold the pixel rows of the cell rows in which the new state differs from what the buffer shows
(changed_pages_restatement.changed_rows).  Cell row r of a puzzle of H rows is the pixel rows [top + 3 r, top + 3 r + 3) of the
frame, top = (pad_h - H) * 3 // 2.  Of the 16-byte chunks of an environment's image
  * the TIGHT set holds a byte of a changed cell row's three pixel rows: the launch must write these;
  * the WIDE set is the same with one cell row added on either side: the launch may write no chunk outside it
(the kernel looks at zone entries of 9 channels, which reach a few bytes across a row boundary).  Nothing here follows the
kernel's arithmetic: every changed cell row becomes a byte range of its environment's image, every byte of it marks its chunk."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import changed_pages_restatement as cp  # noqa: E402,F401  (changed_rows is the input of chunk_sets)
import live_pages_restatement as lp  # noqa: E402


def chunk_sets(pad_h, pad_w, es, puzzle_heights, ids, rows):
    """(tight, wide): bool [B, stride // 16] chunk masks of a library-owned buffer of the batch `ids` whose environments changed
    in the cell rows `rows` (bool [B, 64])."""
    obs_bytes, _stride, cpe, _n_chunks = lp.frame(pad_h, pad_w, es)
    row_bytes = pad_w * lp.PPC * 3 * es
    out = []
    for margin in (0, 1):
        hit = np.zeros((len(ids), cpe * lp.CHUNK), dtype=bool)  # per byte
        for e in range(len(ids)):
            H = int(puzzle_heights[ids[e]])
            top = (pad_h - H) * lp.PPC // 2
            for r in np.flatnonzero(rows[e]):
                r0, r1 = int(r) - margin, int(r) + 1 + margin  # (the margin may be a cell row of the frame padding)
                b0 = max((top + lp.PPC * r0) * row_bytes, 0)
                b1 = min((top + lp.PPC * r1) * row_bytes, obs_bytes)
                hit[e, b0:b1] = True
        out.append(hit.reshape(len(ids), cpe, lp.CHUNK).any(axis=2))
    return out[0], out[1]


def runs_of(row_mask):
    """[(r0, r1)]: the maximal runs of set entries of one environment's bool [64] row mask."""
    m = np.concatenate([[False], np.asarray(row_mask, dtype=bool), [False]])
    d = np.flatnonzero(m[1:] != m[:-1])
    return [(int(a), int(b)) for a, b in zip(d[0::2], d[1::2])]

// rows_range_main.cpp -- pw_rows_chunk_range (csrc/pw_hostlib_pure.h), the run -> chunk-range arithmetic of
// pw_render_rows_kernel, against a byte-by-byte definition.  A stand-alone host program: tests/test_rows_range_host.py
// compiles it with -fsanitize=address,undefined and runs it.
//
// For every frame, element size, puzzle height H (two widths each) and run 0 <= r0 < r1 <= H:
//   * the range is exactly the set of 16-byte chunks that hold a byte whose channel lies in a cell row's channels
//     [27 pad_w r + shift, 27 pad_w (r + 1) + shift + 9) for some r of the run (page_rows_hit's statement, row by row);
//   * it holds every byte of the pixel rows [top + 3 r0, top + 3 r1) of the frame;
//   * it holds no byte outside the pixel rows [top + 3 (r0 - 1), top + 3 (r1 + 1)).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "pw_hostlib_pure.h"

static int failures = 0;

static void fail(const char* what, int pad_h, int pad_w, int es, int H, int W, int r0, int r1) {
  if (failures++ < 10) std::printf("%s: frame %d x %d, es %d, H %d, W %d, rows [%d, %d)\n", what, pad_h, pad_w, es, H, W, r0, r1);
}

static void check_frame(int pad_h, int pad_w, int es) {
  const int row_channels = 9 * pad_w;  // one pixel row: 3 pad_w pixels of 3 channels
  const int obs_bytes = 3 * pad_h * row_channels * es;
  const int n_chunks = (obs_bytes + 15) / 16;
  // per chunk: the lowest and the highest cell row some byte of the chunk belongs to (none: 1, 0)
  std::vector<int16_t> row_min(static_cast<size_t>(n_chunks)), row_max(static_cast<size_t>(n_chunks));
  for (int H = 1; H <= pad_h; H++) {
    const int widths[2] = {pad_w, pad_w > 3 ? pad_w - 3 : 1};
    for (int W : widths) {
      const int top = (pad_h - H) * 3 / 2, left = (pad_w - W) * 3 / 2;  // pixels
      const int c0 = (left + 2) / 3;                                     // cell columns left of the puzzle, rounded up
      const int shift = 3 * (top * 3 * pad_w + left) - 9 * c0;           // channel of entry 0
      for (int c = 0; c < n_chunks; c++) row_min[static_cast<size_t>(c)] = 1, row_max[static_cast<size_t>(c)] = 0;
      for (int b = 0; b < obs_bytes; b++) {  // byte by byte: the cell rows whose channels hold this byte's channel
        const int ch = b / es;
        const size_t c = static_cast<size_t>(b / 16);
        for (int r = 0; r < H && 27 * pad_w * r + shift <= ch; r++) {
          if (ch >= 27 * pad_w * (r + 1) + shift + 9) continue;
          if (row_min[c] > row_max[c]) row_min[c] = row_max[c] = static_cast<int16_t>(r);
          if (r < row_min[c]) row_min[c] = static_cast<int16_t>(r);
          if (r > row_max[c]) row_max[c] = static_cast<int16_t>(r);
        }
      }
      for (int r0 = 0; r0 < H; r0++) {
        for (int r1 = r0 + 1; r1 <= H; r1++) {
          const PwChunkRange got = pw_rows_chunk_range(pad_h, pad_w, H, W, es, r0, r1, n_chunks);
          if (got.lo < 0 || got.hi > n_chunks || got.lo >= got.hi) {
            fail("range out of bounds or empty", pad_h, pad_w, es, H, W, r0, r1);
            continue;
          }
          // (consecutive bytes belong to consecutive cell rows: a chunk holds a byte of the run when its rows meet [r0, r1))
          int differ = 0;
          for (int c = 0; c < n_chunks; c++) {
            const size_t k = static_cast<size_t>(c);
            const bool want = row_min[k] <= row_max[k] && row_min[k] < r1 && row_max[k] >= r0;
            differ += want != (c >= got.lo && c < got.hi);
          }
          if (differ) fail("not the byte-by-byte chunk set", pad_h, pad_w, es, H, W, r0, r1);
          // the first and the last byte of the run's pixel rows lie in the range (which is one interval) ...
          const int b_first = (top + 3 * r0) * row_channels * es, b_last = (top + 3 * r1) * row_channels * es - 1;
          if (b_first / 16 < got.lo || b_last / 16 >= got.hi) fail("a byte of the run's pixel rows is outside the range", pad_h, pad_w, es, H, W, r0, r1);
          // ... and its first and last chunk hold a byte of the pixel rows of the run widened by one cell row
          const int py_lo = ((got.lo * 16 + 15) / es) / row_channels, py_hi = ((got.hi - 1) * 16 / es) / row_channels;
          if (py_lo < top + 3 * (r0 - 1) || py_hi >= top + 3 * (r1 + 1)) fail("a chunk beyond one cell row of margin", pad_h, pad_w, es, H, W, r0, r1);
        }
      }
    }
  }
}

int main() {
  const int frames[4][2] = {{51, 42}, {54, 47}, {16, 16}, {12, 12}};
  for (const auto& f : frames)
    for (int es : {1, 4}) check_frame(f[0], f[1], es);
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}

// pw_hostlib_pure.h -- the arithmetic of the host plumbing (pw_hostlib.inc).  No HIP, no engine: a stand-alone host program
// compiles this header alone (tests/hostlib_pure_main.cpp).
#ifndef PW_HOSTLIB_PURE_H
#define PW_HOSTLIB_PURE_H

#include <algorithm>
#include <cstdint>

// v rounded up to the 256-byte granule of every slab field
inline uint64_t pw_pad256(uint64_t v) { return (v + 255u) & ~uint64_t(255); }

// slots of a closed set that stays at most half full: the smallest power of two >= 2 * max_states
inline uint64_t pw_table_slots(uint64_t max_states) {
  uint64_t slots = 1;
  while (slots < 2ull * max_states) slots <<= 1;
  return slots;
}

// The ladder of a batched search's closed set (csrc/pw_batch_set.inc): the set starts with `lds_slots` slots in LDS and climbs
// tables of 2^16, 2^20, 2^22 ... slots in the workgroup's slab, laid out from byte offset `off`, until one holds 2 * max_states
// (max_states <= 2^28).  Entries beyond the last level are 0.  Returns the offset behind the last table.
inline uint64_t pw_bs_ladder(uint64_t max_states, uint32_t lds_slots, uint32_t bytes_per_slot, uint64_t off,
                             uint32_t (&level_slots)[6], uint64_t (&level_off)[6]) {
  const uint32_t ladder[6] = {1u << 16, 1u << 20, 1u << 22, 1u << 24, 1u << 26, 1u << 29};
  for (int k = 0; k < 6; k++) {
    level_slots[k] = 0u;
    level_off[k] = 0;
  }
  uint64_t have = lds_slots;
  for (int k = 0; k < 6 && have < 2ull * max_states; k++) {
    level_slots[k] = ladder[k];
    level_off[k] = off;
    off += static_cast<uint64_t>(ladder[k]) * bytes_per_slot;
    have = ladder[k];
  }
  return off;
}

// a time limit in seconds as wall-clock ticks of a kernel: 0 = no limit, at least 1 otherwise, ~0 where the product leaves
// 64 bits (+inf included)
inline unsigned long long pw_deadline_ticks(double time_limit, uint32_t clock_khz) {
  if (!(time_limit > 0.0)) return 0ull;
  const double ticks = time_limit * static_cast<double>(clock_khz) * 1000.0;
  if (ticks >= 1.8e19) return ~0ull;
  return std::max<unsigned long long>(1ull, static_cast<unsigned long long>(ticks));
}

// the padded movable counts of the position layouts
inline bool pw_npad_ok(int npad) { return !(npad != 4 && npad != 8 && npad != 16 && npad != 32); }

// Which values an integer setting accepts (a row of the engine option table, pw_engine_options.inc): an inclusive range
// a .. b, one of the listed values a, b, c (a set of two repeats one), any value >= 0, or any value at all.  The remaining
// kinds accept nothing here: a read-only setting, and one whose test is code next to the table.
enum PwValueKind : uint8_t { PW_VALUE_RANGE, PW_VALUE_SET, PW_VALUE_NONNEG, PW_VALUE_ANY, PW_VALUE_CUSTOM, PW_VALUE_READ_ONLY };
struct PwValueRule {
  PwValueKind kind;
  int64_t a, b, c;
};
inline bool pw_value_ok(const PwValueRule& r, int64_t value) {
  switch (r.kind) {
    case PW_VALUE_RANGE: return value >= r.a && value <= r.b;
    case PW_VALUE_SET: return value == r.a || value == r.b || value == r.c;
    case PW_VALUE_NONNEG: return value >= 0;
    case PW_VALUE_ANY: return true;
    default: return false;
  }
}

// function qualifiers of the helpers a kernel calls too: the kernels' translation unit defines them before it includes this
// header, a host program leaves them empty
#ifndef PW_PURE_HD
#define PW_PURE_HD
#endif

// The 16-byte chunks [lo, hi) of one environment's ppc-3 image that hold the pixels of the cell rows [r0, r1) of its puzzle
// (pw_render_rows_kernel; 0 <= r0 < r1 <= H).  The frame is pad_h x pad_w cells, the puzzle H x W cells, es bytes per channel
// value; the geometry is the page kernel's (PageGeom, page_rows_hit in csrc/pw_render_kernels.inc): cell row r covers the
// channels [27 pad_w r + shift, 27 pad_w (r + 1) + shift + 9) of the image, where `shift` is the channel of zone entry 0
// (the top-left frame padding, up to 6 channels early: entries are 9 channels wide and start on multiples of 3 pixels).
// Clamped to the n_chunks chunks of the image.
struct PwChunkRange {
  int32_t lo, hi;
};
PW_PURE_HD inline int32_t pw_rows_entry_shift(int32_t pad_h, int32_t pad_w, int32_t H, int32_t W) {
  const int32_t pady = (pad_h - H) * 3 / 2, padx = (pad_w - W) * 3 / 2;
  const int32_t c0 = (padx + 2) / 3;
  return 3 * (pady * pad_w * 3 + padx - 3 * c0);
}
PW_PURE_HD inline PwChunkRange pw_rows_chunk_range(int32_t pad_h, int32_t pad_w, int32_t H, int32_t W, int32_t es, int32_t r0,
                                                   int32_t r1, int32_t n_chunks) {
  const int32_t shift = pw_rows_entry_shift(pad_h, pad_w, H, W);
  const int32_t ch_lo = 27 * pad_w * r0 + shift, ch_hi = 27 * pad_w * r1 + shift + 9;  // channels
  PwChunkRange c;
  c.lo = ch_lo > 0 ? (ch_lo * es) >> 4 : 0;
  c.hi = (ch_hi * es + 15) >> 4;
  if (c.hi > n_chunks) c.hi = n_chunks;
  if (c.lo > c.hi) c.lo = c.hi;
  return c;
}

#endif  // PW_HOSTLIB_PURE_H

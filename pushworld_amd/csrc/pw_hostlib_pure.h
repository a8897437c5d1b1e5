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

#endif  // PW_HOSTLIB_PURE_H

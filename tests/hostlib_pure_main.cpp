// Stand-alone check of csrc/pw_hostlib_pure.h (tests/test_hostlib_host.py compiles this with the host compiler and
// -fsanitize=address,undefined and runs it).  Exit status 0 and "ok" on success; the first failed check is printed.
#include "pw_hostlib_pure.h"

#include <cstdio>
#include <limits>

static int failures = 0;

#define CHECK(cond)                                         \
  do {                                                      \
    if (!(cond)) {                                          \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond); \
      failures++;                                           \
    }                                                       \
  } while (0)

// pw_bs_ladder: the top level (the LDS table without slab levels) holds 2 * max_states, the levels grow strictly, the offsets
// advance by slots * bytes_per_slot from `off`, unused entries are 0, and the return value is the end of the last table
static void check_ladder(uint64_t max_states, uint32_t lds_slots, uint32_t bytes_per_slot) {
  const uint64_t off0 = 768;
  uint32_t slots[6] = {1, 2, 3, 4, 5, 6};
  uint64_t offs[6] = {1, 2, 3, 4, 5, 6};
  const uint64_t end = pw_bs_ladder(max_states, lds_slots, bytes_per_slot, off0, slots, offs);
  uint64_t top = lds_slots, at = off0;
  int k = 0;
  for (; k < 6 && slots[k] != 0u; k++) {
    CHECK(slots[k] > top);
    CHECK((slots[k] & (slots[k] - 1u)) == 0u);
    CHECK(offs[k] == at);
    CHECK(top < 2 * max_states);  // (a level is only added while the one below is too small)
    at += static_cast<uint64_t>(slots[k]) * bytes_per_slot;
    top = slots[k];
  }
  CHECK(top >= 2 * max_states);
  CHECK(end == at);
  for (; k < 6; k++) CHECK(slots[k] == 0u && offs[k] == 0u);
}

int main() {
  const unsigned long long never = ~0ull;
  // pw_bs_ladder around the LDS tables' half load (4 096 and 2 048 slots), the first slab level (2^16) and the largest cap
  const uint64_t caps4096[] = {1, 2047, 2048, 2049, 1ull << 15, (1ull << 15) + 1, 1ull << 28};
  for (uint64_t m : caps4096) {
    check_ladder(m, 4096u, 8);
    check_ladder(m, 4096u, 12);
  }
  const uint64_t caps2048[] = {1024, 1025, 1ull << 15, (1ull << 15) + 1, 1ull << 28};
  for (uint64_t m : caps2048) check_ladder(m, 2048u, 12);
  {
    uint32_t slots[6];
    uint64_t offs[6];
    CHECK(pw_bs_ladder(2048, 4096u, 8, 512, slots, offs) == 512 && slots[0] == 0u);  // stays in LDS: no slab table
    CHECK(pw_bs_ladder(2049, 4096u, 8, 512, slots, offs) == 512 + (8ull << 16) && slots[0] == 1u << 16 && slots[1] == 0u);
    CHECK(pw_bs_ladder(1024, 2048u, 12, 0, slots, offs) == 0 && slots[0] == 0u);
    CHECK(pw_bs_ladder(1025, 2048u, 12, 0, slots, offs) == (12ull << 16) && slots[0] == 1u << 16 && slots[1] == 0u);
    CHECK(pw_bs_ladder((1ull << 15) + 1, 4096u, 8, 0, slots, offs) == (8ull << 16) + (8ull << 20) && slots[1] == 1u << 20 && slots[2] == 0u);
    CHECK(pw_bs_ladder(1ull << 28, 4096u, 8, 0, slots, offs) > (8ull << 29) && slots[5] == 1u << 29);
  }

  // pw_deadline_ticks: 0 = no limit, at least one tick otherwise, saturated from 1.8e19 ticks upwards
  CHECK(pw_deadline_ticks(0.0, 100000u) == 0ull);
  CHECK(pw_deadline_ticks(-1.0, 100000u) == 0ull);
  CHECK(pw_deadline_ticks(1e-12, 100000u) == 1ull);
  CHECK(pw_deadline_ticks(1.0, 100000u) == 100000000ull);
  CHECK(pw_deadline_ticks(2.5, 100000u) == 250000000ull);
  CHECK(pw_deadline_ticks(1e30, 100000u) == never);
  CHECK(pw_deadline_ticks(std::numeric_limits<double>::infinity(), 100000u) == never);
  CHECK(pw_deadline_ticks(1.8e19 / 1e8, 100000u) == never);  // exactly the clamp
  CHECK(pw_deadline_ticks(1.7e19 / 1e8, 100000u) < never);   // just below it: converted, not saturated

  // pw_table_slots: the smallest power of two >= 2 * max_states
  CHECK(pw_table_slots(1) == 2);
  CHECK(pw_table_slots(2) == 4);
  CHECK(pw_table_slots(3) == 8);
  CHECK(pw_table_slots(1ull << 28) == 1ull << 29);
  CHECK(pw_table_slots((1ull << 28) - 1) == 1ull << 29);
  CHECK(pw_table_slots((1ull << 28) + 1) == 1ull << 30);
  for (int k = 0; k < 40; k++) CHECK(pw_table_slots(1ull << k) == 2ull << k);  // an exact power of two stays
  for (uint64_t m = 1; m < 5000; m++) {
    const uint64_t s = pw_table_slots(m);
    CHECK((s & (s - 1)) == 0 && s >= 2 * m && s / 2 < 2 * m);
  }

  // pw_pad256
  CHECK(pw_pad256(0) == 0);
  CHECK(pw_pad256(1) == 256);
  CHECK(pw_pad256(255) == 256);
  CHECK(pw_pad256(256) == 256);
  CHECK(pw_pad256(257) == 512);
  CHECK(pw_pad256((1ull << 40) + 1) == (1ull << 40) + 256);

  // pw_npad_ok: 4, 8, 16, 32 and nothing else
  for (int npad = -64; npad <= 128; npad++) CHECK(pw_npad_ok(npad) == (npad == 4 || npad == 8 || npad == 16 || npad == 32));

  // pw_value_ok: each kind of rule at its two edges and one step beyond
  {
    const int64_t lo = std::numeric_limits<int64_t>::min(), hi = std::numeric_limits<int64_t>::max();
    const PwValueRule r02{PW_VALUE_RANGE, 0, 2, 0};
    CHECK(!pw_value_ok(r02, -1) && pw_value_ok(r02, 0) && pw_value_ok(r02, 1) && pw_value_ok(r02, 2) && !pw_value_ok(r02, 3));
    CHECK(!pw_value_ok(r02, lo) && !pw_value_ok(r02, hi));
    const PwValueRule r20{PW_VALUE_RANGE, 0, 1 << 20, 0};
    CHECK(!pw_value_ok(r20, -1) && pw_value_ok(r20, 0) && pw_value_ok(r20, 1 << 20) && !pw_value_ok(r20, (1 << 20) + 1));
    CHECK(!pw_value_ok(r20, int64_t(1) << 32));  // (no truncation to 32 bits: 2^32 is not 0)
    const PwValueRule s02{PW_VALUE_SET, 0, 2, 2};  // {0, 2}: a set of two repeats a member
    CHECK(!pw_value_ok(s02, -1) && pw_value_ok(s02, 0) && !pw_value_ok(s02, 1) && pw_value_ok(s02, 2) && !pw_value_ok(s02, 3));
    const PwValueRule s048{PW_VALUE_SET, 0, 4, 8};
    CHECK(!pw_value_ok(s048, -1) && pw_value_ok(s048, 0) && !pw_value_ok(s048, 1) && !pw_value_ok(s048, 3) && pw_value_ok(s048, 4) &&
          !pw_value_ok(s048, 5) && !pw_value_ok(s048, 7) && pw_value_ok(s048, 8) && !pw_value_ok(s048, 9));
    const PwValueRule sm{PW_VALUE_SET, -1, 0, 2};  // {-1, 0, 2}: the negative member
    CHECK(!pw_value_ok(sm, -2) && pw_value_ok(sm, -1) && pw_value_ok(sm, 0) && !pw_value_ok(sm, 1) && pw_value_ok(sm, 2) && !pw_value_ok(sm, 3));
    const PwValueRule s023{PW_VALUE_SET, 0, 2, 3};
    CHECK(!pw_value_ok(s023, -1) && pw_value_ok(s023, 0) && !pw_value_ok(s023, 1) && pw_value_ok(s023, 2) && pw_value_ok(s023, 3) &&
          !pw_value_ok(s023, 4));
    const PwValueRule nn{PW_VALUE_NONNEG, 0, 0, 0};
    CHECK(!pw_value_ok(nn, lo) && !pw_value_ok(nn, -1) && pw_value_ok(nn, 0) && pw_value_ok(nn, 1) && pw_value_ok(nn, hi));
    const PwValueRule any{PW_VALUE_ANY, 0, 0, 0};
    CHECK(pw_value_ok(any, lo) && pw_value_ok(any, -1) && pw_value_ok(any, 0) && pw_value_ok(any, hi));
    // a read-only setting accepts nothing, and neither does the pure test of a rule that is code
    const PwValueKind closed[] = {PW_VALUE_READ_ONLY, PW_VALUE_CUSTOM};
    for (PwValueKind k : closed) {
      const PwValueRule none{k, 0, 2, 0};
      CHECK(!pw_value_ok(none, lo) && !pw_value_ok(none, -1) && !pw_value_ok(none, 0) && !pw_value_ok(none, 1) && !pw_value_ok(none, hi));
    }
  }

  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}

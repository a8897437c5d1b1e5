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

int main() {
  const unsigned long long never = ~0ull;
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

  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}

// pw_start_pool.inc -- K27: the level below K25, the start state WITHIN a puzzle, chosen on the device inside autoreset.  A pool
// is a flat list of start states (pos, puzzle, level) grouped once by (puzzle, level); pw_start_pool_arm notes which environments
// the next PW_STEP_AUTORESET step will reset, pw_start_pool_draw gives those a state of their puzzle's band of levels, and
// pw_start_pool_update_bands moves the band of every puzzle with the success rate of an EpisodeStats block.  Part of the single
// translation unit pw_kernels.hip (included there after pw_curriculum.inc: uses mix64 and check_launch).
//
// Everything is integer arithmetic: the results are exact and independent of launch geometry.  Every launch runs on the caller's
// stream, allocates nothing, never waits and can be captured.  One lane per environment (arm, draw) or per puzzle (bands); no
// atomics, no LDS, no loop besides the copy of a state, which is unrolled.
// (the two streams, seed ^ PW_START_POOL_K_DRAW and seed ^ PW_START_POOL_K_KEEP: include/pushworld_amd.h)

// ------------------------------------------------------------------------------------------------------------------ arm
__global__ __launch_bounds__(256) void pw_start_pool_arm_kernel(const uint8_t* term, const uint8_t* trunc, uint8_t* pending,
                                                                int32_t n) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n) return;
  pending[i] = (term[i] | trunc[i]) != 0 ? 1 : 0;
}

// ----------------------------------------------------------------------------------------------------------------- draw
struct StartPoolDrawArgs {
  const int8_t* pool_pos;      // [S][npad][2]
  const int32_t* pool_level;   // [S]
  const int32_t* order;        // [S]
  const uint32_t* start;       // [start_words]
  const int64_t* lvl_off;      // [P]
  const int32_t* max_level;    // [P]
  int64_t start_words;
  int32_t num_entries;         // S
  int32_t num_puzzles;         // P
  const int32_t* puzzle_id;    // [n]
  const uint8_t* mask;         // [n] or NULL
  int32_t n, npad;
  uint64_t seed;
  uint32_t* counter;           // [n]
  uint32_t keep_q16;
  int32_t lo, hi;              // the band, unless ...
  const int32_t* band;         // ... [P][2] per puzzle, unless ...
  const int32_t* lo_n;         // ... [n] each: a band per environment
  const int32_t* hi_n;
  int8_t* pos;                 // [n][npad][2]
  int32_t* steps;
  uint8_t* term;               // or NULL
  uint8_t* trunc;              // or NULL
  int32_t* out_entry;
  int32_t* out_level;
};

__global__ __launch_bounds__(256) void pw_start_pool_draw_kernel(StartPoolDrawArgs a) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= a.n) return;
  if (a.mask && a.mask[i] == 0) return;
  const int32_t p = a.puzzle_id[i];
  int32_t ml = -1;
  int64_t off = 0;
  if (p >= 0 && p < a.num_puzzles) {
    ml = a.max_level[p];
    off = a.lvl_off[p];
  }
  // (a puzzle's words must lie inside `start`: a pool that says otherwise is read as a puzzle without entries)
  if (ml < 0 || off < 0 || off + ml + 2 > a.start_words) {
    a.out_entry[i] = -1;
    a.out_level[i] = -1;
    return;
  }
  int32_t lo, hi;
  if (a.lo_n) {
    lo = a.lo_n[i];
    hi = a.hi_n[i];
  } else if (a.band) {
    lo = a.band[2 * static_cast<int64_t>(p)];
    hi = a.band[2 * static_cast<int64_t>(p) + 1];
  } else {
    lo = a.lo;
    hi = a.hi;
  }
  if (hi < 0) hi = ml;
  hi = max(hi, lo);
  lo = min(max(lo, 0), ml);
  hi = min(max(hi, 0), ml);
  const uint32_t first = a.start[off + lo], end = a.start[off + hi + 1];
  if (end <= first || end > static_cast<uint32_t>(a.num_entries)) {  // an empty band
    a.out_entry[i] = -1;
    a.out_level[i] = -1;
    return;
  }
  const uint32_t ctr = a.counter[i] + 1u;
  a.counter[i] = ctr;
  if (a.keep_q16 > 0u &&
      static_cast<uint32_t>(mix64(a.seed ^ PW_START_POOL_K_KEEP, static_cast<uint64_t>(i), ctr) >> 48) < a.keep_q16) {
    a.out_entry[i] = -1;  // the environment keeps the state it has
    a.out_level[i] = -1;
    return;
  }
  // floor(r * count / 2^64): uniform over the band's entries to 2^-32
  const uint32_t u = static_cast<uint32_t>(
      __umul64hi(mix64(a.seed ^ PW_START_POOL_K_DRAW, static_cast<uint64_t>(i), ctr), static_cast<uint64_t>(end - first)));
  const int32_t entry = a.order[first + u];
  if (entry < 0 || entry >= a.num_entries) {  // (never, for a pool grouped by this library)
    a.out_entry[i] = -1;
    a.out_level[i] = -1;
    return;
  }
  // npad pairs = 2 npad bytes: 8 (npad 4) or a multiple of 16; both sides are aligned to that by their layout
  const int8_t* src = a.pool_pos + static_cast<int64_t>(entry) * a.npad * 2;
  int8_t* dst = a.pos + i * a.npad * 2;
  if (a.npad == 4) {
    *reinterpret_cast<uint2*>(dst) = *reinterpret_cast<const uint2*>(src);
  } else {
#pragma unroll
    for (int q = 0; q < 4; q++)
      if (8 * q < a.npad) reinterpret_cast<uint4*>(dst)[q] = reinterpret_cast<const uint4*>(src)[q];
  }
  a.steps[i] = 0;
  if (a.term) a.term[i] = 0;
  if (a.trunc) a.trunc[i] = 0;
  a.out_entry[i] = entry;
  a.out_level[i] = a.pool_level[entry];
}

// ---------------------------------------------------------------------------------------------------------------- bands
struct StartPoolBandsArgs {
  const int32_t* max_level;  // [P]
  const long long* stats;    // [P][PW_EPISODE_STATS]
  long long* base;           // [P][PW_EPISODE_STATS]
  int32_t* band;             // [P][2]
  int8_t* delta;             // [P] or NULL
  int32_t num_puzzles;
  int32_t min_episodes;
  uint32_t up_q16, down_q16;
  int32_t step, width, hi_min, lo_min;
};

__device__ __forceinline__ int64_t pool_min(int64_t x, int64_t y) { return x < y ? x : y; }
__device__ __forceinline__ int64_t pool_max(int64_t x, int64_t y) { return x > y ? x : y; }

__global__ __launch_bounds__(256) void pw_start_pool_update_bands_kernel(StartPoolBandsArgs a) {
  const int64_t p = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (p >= a.num_puzzles) return;
  const int64_t ml = a.max_level[p];
  if (ml < 0) return;
  const long long* st = a.stats + p * PW_EPISODE_STATS;
  long long* bs = a.base + p * PW_EPISODE_STATS;
  const long long nd = st[0] - bs[0], sd = st[1] - bs[1];
  uint64_t n = nd > 0 ? static_cast<uint64_t>(nd) : 0u, s = sd > 0 ? static_cast<uint64_t>(sd) : 0u;
  if (s > n) s = n;
  if (n < static_cast<uint64_t>(a.min_episodes)) return;  // the record keeps growing: base stays
  const int bits = 64 - __clzll(static_cast<long long>(n));  // bit_length(n), n >= 1 here
  const int k = bits > 20 ? bits - 20 : 0;
  n >>= k;  // < 2^20: the products below stay under 2^37
  s >>= k;
  int64_t lo = a.band[2 * p], hi = a.band[2 * p + 1];
  if (hi < 0) hi = ml;
  const int64_t hi_in = hi;
  if (s * 65536u >= static_cast<uint64_t>(a.up_q16) * n) {
    hi = pool_min(hi + a.step, ml);
  } else if (s * 65536u < static_cast<uint64_t>(a.down_q16) * n) {
    hi = pool_max(hi - a.step, pool_min(a.hi_min, ml));
  }
  if (a.width > 0) lo = pool_max(a.lo_min, hi - a.width + 1);
  // (hi stays inside int32: it moves towards a bound that is one, or it keeps the int32 it was read as)
  a.band[2 * p] = static_cast<int32_t>(lo);
  a.band[2 * p + 1] = static_cast<int32_t>(hi);
#pragma unroll
  for (int c = 0; c < PW_EPISODE_STATS; c++) bs[c] = st[c];
  if (a.delta) a.delta[p] = hi > hi_in ? 1 : (hi < hi_in ? -1 : 0);
}

// ------------------------------------------------------------------------------------------------------------ host side
extern "C" {

int pw_start_pool_arm(PwEngine* e, const uint8_t* terminated, const uint8_t* truncated, uint8_t* pending, int32_t n,
                      void* stream) try {
  if (!e) return pw_fail(PW_EINVAL, "pw_start_pool_arm: null engine");
  if (!terminated) return pw_fail(PW_EINVAL, "pw_start_pool_arm: null terminated");
  if (!truncated) return pw_fail(PW_EINVAL, "pw_start_pool_arm: null truncated");
  if (!pending) return pw_fail(PW_EINVAL, "pw_start_pool_arm: null pending");
  if (n < 0) return pw_fail(PW_EINVAL, "pw_start_pool_arm: n must be >= 0");
  if (n == 0) return PW_OK;
  PwDeviceGuard guard(e->set->device);
  const dim3 grid(static_cast<unsigned>((static_cast<int64_t>(n) + 255) / 256)), block(256);
  hipLaunchKernelGGL(pw_start_pool_arm_kernel, grid, block, 0, static_cast<hipStream_t>(stream), terminated, truncated, pending, n);
  return check_launch("pw_start_pool_arm");
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_start_pool_draw(PwEngine* e, const int8_t* pool_pos, const int32_t* pool_level, const int32_t* order,
                       const uint32_t* start, int64_t start_words, const int64_t* lvl_off, const int32_t* max_level,
                       int32_t num_entries, const int32_t* puzzle_id, const uint8_t* mask, int32_t n, uint64_t seed,
                       uint32_t* counter, uint32_t keep_q16, int32_t lo, int32_t hi, const int32_t* band, const int32_t* lo_n,
                       const int32_t* hi_n, int8_t* pos, int32_t* steps, uint8_t* terminated, uint8_t* truncated,
                       int32_t* out_entry, int32_t* out_level, void* stream) try {
  if (!e) return pw_fail(PW_EINVAL, "pw_start_pool_draw: null engine");
  if (!pool_pos) return pw_fail(PW_EINVAL, "pw_start_pool_draw: null pool_pos");
  if (!pool_level) return pw_fail(PW_EINVAL, "pw_start_pool_draw: null pool_level");
  if (!order) return pw_fail(PW_EINVAL, "pw_start_pool_draw: null order");
  if (!start) return pw_fail(PW_EINVAL, "pw_start_pool_draw: null start");
  if (start_words < 1) return pw_fail(PW_EINVAL, "pw_start_pool_draw: start_words must be >= 1");
  if (!lvl_off) return pw_fail(PW_EINVAL, "pw_start_pool_draw: null lvl_off");
  if (!max_level) return pw_fail(PW_EINVAL, "pw_start_pool_draw: null max_level");
  if (num_entries < 1) return pw_fail(PW_EINVAL, "pw_start_pool_draw: num_entries must be >= 1");
  if (!puzzle_id) return pw_fail(PW_EINVAL, "pw_start_pool_draw: null puzzle_id");
  if (n < 0) return pw_fail(PW_EINVAL, "pw_start_pool_draw: n must be >= 0");
  if (!counter) return pw_fail(PW_EINVAL, "pw_start_pool_draw: null counter");
  if (keep_q16 > 65536u) return pw_fail(PW_EINVAL, "pw_start_pool_draw: keep_q16 must be in 0 .. 65536");
  if ((lo_n == nullptr) != (hi_n == nullptr)) return pw_fail(PW_EINVAL, "pw_start_pool_draw: lo_n and hi_n go together");
  if (!pos) return pw_fail(PW_EINVAL, "pw_start_pool_draw: null pos");
  if (!steps) return pw_fail(PW_EINVAL, "pw_start_pool_draw: null steps");
  if (!out_entry) return pw_fail(PW_EINVAL, "pw_start_pool_draw: null out_entry");
  if (!out_level) return pw_fail(PW_EINVAL, "pw_start_pool_draw: null out_level");
  if (n == 0) return PW_OK;
  PwDeviceGuard guard(e->set->device);
  StartPoolDrawArgs a{pool_pos, pool_level, order, start, lvl_off, max_level, start_words, num_entries, e->set->count,
                      puzzle_id, mask, n, e->np, seed, counter, keep_q16, lo, hi, band, lo_n, hi_n, pos, steps, terminated,
                      truncated, out_entry, out_level};
  const dim3 grid(static_cast<unsigned>((static_cast<int64_t>(n) + 255) / 256)), block(256);
  hipLaunchKernelGGL(pw_start_pool_draw_kernel, grid, block, 0, static_cast<hipStream_t>(stream), a);
  return check_launch("pw_start_pool_draw");
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_start_pool_update_bands(PwEngine* e, const int32_t* max_level, const int64_t* stats, int64_t* base, int32_t* band,
                               int8_t* delta, int32_t min_episodes, uint32_t up_q16, uint32_t down_q16, int32_t step,
                               int32_t width, int32_t hi_min, int32_t lo_min, void* stream) try {
  if (!e) return pw_fail(PW_EINVAL, "pw_start_pool_update_bands: null engine");
  if (!max_level) return pw_fail(PW_EINVAL, "pw_start_pool_update_bands: null max_level");
  if (!stats) return pw_fail(PW_EINVAL, "pw_start_pool_update_bands: null stats");
  if (!base) return pw_fail(PW_EINVAL, "pw_start_pool_update_bands: null base");
  if (!band) return pw_fail(PW_EINVAL, "pw_start_pool_update_bands: null band");
  if (min_episodes < 1) return pw_fail(PW_EINVAL, "pw_start_pool_update_bands: min_episodes must be >= 1");
  if (up_q16 > 65536u) return pw_fail(PW_EINVAL, "pw_start_pool_update_bands: up_q16 must be in 0 .. 65536");
  if (down_q16 > 65536u) return pw_fail(PW_EINVAL, "pw_start_pool_update_bands: down_q16 must be in 0 .. 65536");
  if (up_q16 < down_q16) return pw_fail(PW_EINVAL, "pw_start_pool_update_bands: up_q16 must not be below down_q16");
  if (step < 1) return pw_fail(PW_EINVAL, "pw_start_pool_update_bands: step must be >= 1");
  if (width < 0) return pw_fail(PW_EINVAL, "pw_start_pool_update_bands: width must be >= 0");
  if (e->set->count < 1) return PW_OK;
  PwDeviceGuard guard(e->set->device);
  StartPoolBandsArgs a{max_level, reinterpret_cast<const long long*>(stats), reinterpret_cast<long long*>(base), band, delta,
                       e->set->count, min_episodes, up_q16, down_q16, step, width, hi_min, lo_min};
  const dim3 grid(static_cast<unsigned>((static_cast<int64_t>(e->set->count) + 255) / 256)), block(256);
  hipLaunchKernelGGL(pw_start_pool_update_bands_kernel, grid, block, 0, static_cast<hipStream_t>(stream), a);
  return check_launch("pw_start_pool_update_bands");
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

}  // extern "C"

// pw_solution_batch.inc -- exact cost-to-go tables of MANY small puzzles in one launch (DESIGN.md K13).
// Included from pw_kernels.hip after pw_solution.inc (uses pw_batch_set.inc's state words, closed set, slot table
// and lookup, and the table-only lane step).
//
// pw_search_solve (K12) gives ONE puzzle its table with a launch per pass and per sweep: at the sizes of the Level-0 pool it
// is launch bound.  pw_solve_batch is the backward half in the form of pw_search_batch (K5b): persistent workgroups of 256
// take puzzles off a device counter and do everything for a puzzle inside the kernel --
//   1. an exhaustive breadth-first search over PwBatchSet<true> (one 64-bit word per state, closed set in LDS that moves up
//      the 2^16 / 2^20 / ... ladder of the workgroup's slab, "grow before the layer"), which does NOT stop at a goal state;
//      every slot of the closed set also holds the store index of its state (a uint32 next to the table);
//   2. the successor pass: the lane step again for every state and action, looked up (read only) in the closed set;
//   3. backward sweeps over succ and a uint16 cost array: sweep k settles every unsettled state with a successor of cost
//      k - 1; a barrier between sweeps instead of K12's launch, a workgroup flag in LDS ends them;
//   4. action bits (K12's definitions), the counts, and -- when the caller's row pool has room -- the rows: key, succ,
//      cost, acts copied out with coalesced stores, plus a per-item open-addressing table of row numbers for the query.
// Rows are reserved with one atomicAdd per puzzle, so WHICH offset a puzzle gets depends on the schedule; so does the
// numbering of the states inside a breadth-first layer.  No result depends on either: rows are found by state.
// pw_solve_batch_query maps live states of a mixed batch to rows in one capturable launch.

#define PW_SB_BUILT 0
#define PW_SB_TOO_MANY 2
#define PW_SB_NOT_SEARCHED 3
#define PW_SB_SUMMARY_ONLY 4
#define PW_SB_COST_RANGE 5
#define PW_SB_INTERNAL 6

struct SolveBatchArgs {
  const PwPuzzleHeader* hdrs;
  const uint8_t* blob;
  const uint64_t* ovl;
  const PwOvlDir* ovl_dir;
  const int32_t* puzzles;  // [n] set indices, or NULL = 0 .. n - 1
  int32_t n;
  int32_t num_puzzles;
  uint32_t max_states;
  uint8_t* slab;           // gridDim.x slabs of slab_bytes: state store, succ, cost, then the HBM tables
  uint64_t slab_bytes;
  uint32_t level_slots[6]; // slots of table level 1 .. (0 = no such level); level 0 is the LDS table
  uint64_t level_off[6];   // byte offsets in the slab: level_slots keys (8 bytes), then level_slots store indices (4 bytes)
  uint64_t succ_off, cost_off;
  uint32_t* next;          // work counter
  unsigned long long* counters;  // [0] rows of every built table (what a pool that stores them all needs), [1] lookup slots
                                 // reserved, [2] successors missing from an exhausted closed set
  uint8_t* status;
  int32_t* summary;        // [n][5]
  int64_t* row_off;        // [n]
  int64_t* slot_off;       // [n]
  uint8_t* slot_log2;      // [n]
  int32_t* item_of_puzzle; // [num_puzzles]
  int64_t rows_cap, slots_cap;
  unsigned long long* pool_key;
  int32_t* pool_succ;
  uint16_t* pool_cost;
  uint8_t* pool_acts;
  uint32_t* pool_slots;
};

__global__ __launch_bounds__(256) void pw_solve_batch_kernel(SolveBatchArgs a) {
  __shared__ unsigned long long s_tab[PW_BS_LDS_SLOTS];
  __shared__ uint32_t s_idx[PW_BS_LDS_SLOTS];
  __shared__ uint32_t s_total, s_overflow, s_goals, s_dead, s_missing, s_flag[3], s_log2;
  __shared__ int32_t s_item;
  __shared__ long long s_row, s_slot;
  const int tid = threadIdx.x;
  uint8_t* slab = a.slab + static_cast<uint64_t>(blockIdx.x) * a.slab_bytes;
  unsigned long long* store = reinterpret_cast<unsigned long long*>(slab);
  int32_t* succ = reinterpret_cast<int32_t*>(slab + a.succ_off);
  uint16_t* cost = reinterpret_cast<uint16_t*>(slab + a.cost_off);
  for (;;) {
    const int item = pw_bs_next_item(a.next, &s_item);
    if (item >= a.n) return;
    const int pid = pw_clamp_pid(a.puzzles ? a.puzzles[item] : item, a.num_puzzles);
    const PwPuzzleHeader* h = a.hdrs + pid;
    const int N = h->N;
    int status = -1;
    if (!pw_bs_fits(h, a.ovl_dir, pid)) status = PW_SB_NOT_SEARCHED;  // the caller's pw_search_solve
    uint32_t total = 0, max_cost = 0;
    if (status < 0) {
      LanePuzzleT<const uint64_t*, 2> p;
      uint32_t OT[8];
      pw_bs_puzzle(a.hdrs, a.blob, a.ovl, a.ovl_dir, pid, p, OT);

      PwBatchSet<true> set;
      set.start(s_tab, s_idx, PW_BS_LDS_SLOTS);
      // A state word holds the first N movables and zeros beyond: whatever the 16-byte init row holds there stays out of the
      // key (the lane step never touches a movable beyond N, so the zeros stay; pw_solve_batch_query packs the same way).
      const uint64_t keep = pw_sb_keep(N);
      uint32_t P0[4];
      pw_bs_load_init(h, P0);
      const uint64_t k0 = pw_bs_pack(P0) & keep;
      uint64_t gkey, gmask;
      pw_bs_goal_word(h, gkey, gmask);
      if (tid == 0) {
        s_total = 1u;
        s_overflow = 0u;
        s_goals = 0u;
        s_dead = 0u;
        s_missing = 0u;
        s_flag[0] = s_flag[1] = s_flag[2] = 0u;
        store[0] = k0;
      }
      __syncthreads();
      if (tid == 0) set.put(k0, 0u);
      uint32_t begin = 0u, end = 1u;
      // ---- 1. the whole reachable space (goal states are expanded like any other)
      for (;;) {
        __syncthreads();
        // (workgroup-uniform: `end` was read from s_total between two barriers, as in pw_search_batch_kernel)
        const uint32_t cur = end, L = end - begin;
        // everything this layer can add must fit at half load
        if (set.grow(min(static_cast<uint64_t>(cur) + 4ull * L, static_cast<uint64_t>(a.max_states)), a.level_slots, a.level_off,
                     slab, store, cur))
          __syncthreads();  // (uniform) the rehash is complete
        for (uint32_t i = begin + tid; i < end; i += 256u) {
          uint32_t PP[4];
          pw_bs_unpack(store[i], PP);
#pragma unroll 1
          for (int act = 0; act < 4; act++) {
            LaneEnv<8> s;
            pw_bs_fresh_env(PP, s);
            if (!lane_step<8>(p, h, OT, s, act, 0u, -1)) continue;  // nothing moved: the parent itself
            uint32_t idx;
            (void)set.claim(pw_bs_pack(s.P) & keep, store, a.max_states, &s_total, &s_overflow, idx);
          }
        }
        __threadfence();
        __syncthreads();
        if (s_overflow) {
          status = PW_SB_TOO_MANY;
          break;
        }
        begin = end;
        end = s_total;
        if (begin == end) break;  // exhausted
      }
      total = min(status == PW_SB_TOO_MANY ? s_total : end, a.max_states);
      if (status < 0) {
        // ---- 2. successors (local indices) and the costs' starting values
        for (uint32_t i0 = 0; i0 < total; i0 += 256u) {  // (whole rounds: the ballot below needs every lane)
          const uint32_t i = i0 + tid;
          bool goal = false;
          if (i < total) {
            const uint64_t key = store[i];
            uint32_t PP[4];
            pw_bs_unpack(key, PP);
            int4 out = make_int4(static_cast<int>(i), static_cast<int>(i), static_cast<int>(i), static_cast<int>(i));
#pragma unroll 1
            for (int act = 0; act < 4; act++) {
              LaneEnv<8> s;
              pw_bs_fresh_env(PP, s);
              if (!lane_step<8>(p, h, OT, s, act, 0u, -1)) continue;
              uint32_t r = pw_bs_find(set.tab, set.tidx, set.cap - 1u, pw_bs_pack(s.P) & keep);
              if (r >= total) {  // not in an exhausted closed set: counted, the item's status says so
                atomicAdd(&s_missing, 1u);
                r = i;
              }
              out.x = act == 0 ? static_cast<int>(r) : out.x;
              out.y = act == 1 ? static_cast<int>(r) : out.y;
              out.z = act == 2 ? static_cast<int>(r) : out.z;
              out.w = act == 3 ? static_cast<int>(r) : out.w;
            }
            reinterpret_cast<int4*>(succ)[i] = out;
            goal = (key & gmask) == gkey;
            cost[i] = goal ? 0 : PW_SOLVE_INF;
          }
          const unsigned long long m = __ballot(goal);
          if ((tid & (PW_WAVE - 1)) == 0 && m) atomicAdd(&s_goals, static_cast<uint32_t>(__popcll(m)));
        }
        __syncthreads();
        if (s_missing) status = PW_SB_INTERNAL;
        // ---- 3. backward sweeps.  Sweep k raises flag k % 3 and clears flag (k + 1) % 3, which was last read before the
        // barrier that ended sweep k - 1: one barrier per sweep.  (A cost written by sweep k is k, never k - 1, so reading it
        // while others write is harmless.)  k = 65535 only looks: the value it would write is the "none" mark itself.
        if (status < 0 && s_goals) {
          for (uint32_t k = 1; k <= PW_SOLVE_INF; k++) {
            if (tid == 0) s_flag[(k + 1u) % 3u] = 0u;
            const uint32_t want = k - 1u;
            bool any = false;
            for (uint32_t i = tid; i < total; i += 256u) {
              if (cost[i] != PW_SOLVE_INF) continue;
              const int4 s = reinterpret_cast<const int4*>(succ)[i];
              if (cost[s.x] == want || cost[s.y] == want || cost[s.z] == want || cost[s.w] == want) {
                if (k < PW_SOLVE_INF) cost[i] = static_cast<uint16_t>(k);
                any = true;
              }
            }
            if (any) s_flag[k % 3u] = 1u;
            __syncthreads();
            if (!s_flag[k % 3u]) break;
            if (k == PW_SOLVE_INF) {
              status = PW_SB_COST_RANGE;
              break;
            }
            max_cost = k;
          }
        }
      }
    }
    // ---- 4. rows for the table, when there is one and the pool has room
    __syncthreads();
    const bool built = status < 0;
    if (tid == 0) {
      long long row = -1, slot = -1;
      uint32_t lg = 4;
      if (built) {
        row = static_cast<long long>(atomicAdd(&a.counters[0], static_cast<unsigned long long>(total)));
        while ((1ull << lg) < 2ull * total) lg++;
        if (row + static_cast<long long>(total) <= a.rows_cap) {
          slot = static_cast<long long>(atomicAdd(&a.counters[1], 1ull << lg));
          if (slot + (1ll << lg) > a.slots_cap) slot = -1;
        }
        if (slot < 0) row = -1;
      }
      if (status == PW_SB_INTERNAL) atomicAdd(&a.counters[2], static_cast<unsigned long long>(s_missing));
      s_row = row;
      s_slot = slot;
      s_log2 = lg;
    }
    __syncthreads();
    const long long row = s_row;
    const bool stored = row >= 0;
    if (built) {
      uint32_t* slots = stored ? a.pool_slots + s_slot : nullptr;
      const uint32_t smask = (1u << s_log2) - 1u;
      if (stored) pw_sb_slots_clear(slots, smask);
      for (uint32_t i0 = 0; i0 < total; i0 += 256u) {
        const uint32_t i = i0 + tid;
        bool dead = false;
        if (i < total) {
          const uint32_t c = cost[i];
          dead = c == PW_SOLVE_INF;
          if (stored) {
            // bit a: action a is optimal (moves, and its successor is one step nearer); bit 4 + a: safe (pw_solve_acts_kernel)
            const int4 s = reinterpret_cast<const int4*>(succ)[i];
            const int32_t t[4] = {s.x, s.y, s.z, s.w};
            uint32_t bits = 0;
#pragma unroll
            for (int act = 0; act < 4; act++) {
              const uint32_t ct = cost[t[act]];
              if (ct != PW_SOLVE_INF) bits |= 16u << act;
              if (c != 0u && c != PW_SOLVE_INF && t[act] != static_cast<int32_t>(i) && ct + 1u == c) bits |= 1u << act;
            }
            a.pool_key[row + i] = store[i];
            reinterpret_cast<int4*>(a.pool_succ)[row + i] = s;
            a.pool_cost[row + i] = static_cast<uint16_t>(c);
            a.pool_acts[row + i] = static_cast<uint8_t>(bits);
          }
        }
        const unsigned long long m = __ballot(dead);
        if ((tid & (PW_WAVE - 1)) == 0 && m) atomicAdd(&s_dead, static_cast<uint32_t>(__popcll(m)));
      }
      if (stored) pw_sb_slots_fill(slots, smask, store, total);  // (uniform: s_row)
    }
    __syncthreads();
    if (tid == 0) {
      const bool valid = built;
      int32_t* sum = a.summary + static_cast<int64_t>(item) * 5;
      sum[0] = static_cast<int32_t>(total);
      sum[1] = valid ? static_cast<int32_t>(s_goals) : 0;
      sum[2] = valid ? static_cast<int32_t>(s_dead) : 0;
      sum[3] = valid ? static_cast<int32_t>(max_cost) : 0;
      sum[4] = valid ? (cost[0] == PW_SOLVE_INF ? -1 : static_cast<int32_t>(cost[0])) : -1;
      a.status[item] = static_cast<uint8_t>(built ? (stored ? PW_SB_BUILT : PW_SB_SUMMARY_ONLY) : status);
      a.row_off[item] = row;
      a.slot_off[item] = stored ? s_slot : -1;
      a.slot_log2[item] = static_cast<uint8_t>(s_log2);
      if (stored) atomicMax(&a.item_of_puzzle[pid], item);  // (a puzzle listed twice: the higher item answers the queries)
    }
  }
}

// ---- query: live states of a mixed batch -> rows -------------------------------------------------------------------------------
struct SolveBatchQueryArgs {
  SolveBatchTables t;
  const int32_t* puzzle_id;  // [n]
  const int8_t* pos;         // [n][npad][2]
  const uint8_t* item_mask;  // or NULL
  int32_t npad, n;
  int32_t* out_index;
  int32_t* out_cost;
  uint8_t* out_acts;
};

// what row `idx` of the table at `base` answers (pw_sb_lookup's pair): the cost to go, -1 a dead end, -2 not in the table
// (pw_sb_lookup's two negative answers, -1 and PW_SB_NOTABLE, both read -2 / no action bits)
__device__ __forceinline__ int32_t pw_sb_row_cost(const SolveBatchTables& t, int64_t base, int64_t idx) {
  if (idx < 0) return -2;
  const uint32_t c = t.pool_cost[base + idx];
  return c == PW_SOLVE_INF ? -1 : static_cast<int32_t>(c);
}
__device__ __forceinline__ uint32_t pw_sb_row_acts(const SolveBatchTables& t, int64_t base, int64_t idx) {
  return idx >= 0 ? t.pool_acts[base + idx] : 0u;
}

__global__ __launch_bounds__(256) void pw_solve_batch_query_kernel(SolveBatchQueryArgs a) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= a.n) return;
  if (a.item_mask && a.item_mask[i] == 0) return;
  int64_t base;
  const int64_t idx = pw_sb_lookup(a.t, a.puzzle_id[i], a.pos + i * a.npad * 2, a.npad, base);
  if (idx == PW_SB_NOTABLE) return;  // no stored table for this puzzle: another table's item, untouched
  if (a.out_index) a.out_index[i] = static_cast<int32_t>(idx);
  if (a.out_cost) a.out_cost[i] = pw_sb_row_cost(a.t, base, idx);
  if (a.out_acts) a.out_acts[i] = static_cast<uint8_t>(pw_sb_row_acts(a.t, base, idx));
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
// (tests/test_solution_batch_host.py builds the head of this struct -- eng .. n -- by hand to reach the "no run yet" checks
//  without a device: keep those five members first and in this order)
struct PwSolveBatch {
  PwEngine* eng;
  int64_t rows_cap, slots_cap;
  int32_t n_cap, n;  // items the per-item arrays hold / items of the last run (0: no run yet)
  unsigned long long* d_key;
  int32_t* d_succ;
  uint16_t* d_cost;
  uint8_t* d_acts;
  uint32_t* d_slots;
  uint8_t* d_status;
  int32_t* d_summary;
  int64_t* d_row_off;
  int64_t* d_slot_off;
  uint8_t* d_slot_log2;
  int32_t* d_item_of_puzzle;
  unsigned long long* d_counters;
  // host copies of the last run's status / summary / row_off, fetched by the first pw_solve_batch_read after it
  bool host_valid;
  std::vector<uint8_t> h_status;
  std::vector<int32_t> h_summary;
  std::vector<int64_t> h_row_off;
  // cost index of the last run's stored tables (pw_solve_batch_index, csrc/pw_table_sample.inc); new members go HERE, at the end
  bool index_valid;
  int32_t* d_rows_by_cost;   // [rows_cap], parallel to the pool: item i's permutation of its rows at row_off[i]
  uint32_t* d_cost_start;    // ragged: max_cost + 3 words per stored item
  int64_t* d_cs_off;         // [n] where an item's cost_start begins, -1: none
  std::vector<int64_t> h_cs_off;
};

// the stored tables as a query sees them (pw_solve_batch_query, pw_guide_step)
static SolveBatchTables solve_batch_tables(const PwSolveBatch* b) {
  SolveBatchTables t;
  t.hdrs = b->eng->set->d_headers;
  t.num_puzzles = b->eng->set->count;
  t.item_of_puzzle = b->d_item_of_puzzle;
  t.row_off = b->d_row_off;
  t.slot_off = b->d_slot_off;
  t.slot_log2 = b->d_slot_log2;
  t.pool_key = b->d_key;
  t.pool_cost = b->d_cost;
  t.pool_acts = b->d_acts;
  t.pool_slots = b->d_slots;
  return t;
}

static void solve_batch_free_index(PwSolveBatch* b) {
  void* bufs[] = {b->d_rows_by_cost, b->d_cost_start, b->d_cs_off};
  for (void* p : bufs)
    if (p) (void)hipFree(p);
  b->d_rows_by_cost = nullptr;
  b->d_cost_start = nullptr;
  b->d_cs_off = nullptr;
  b->index_valid = false;
}

// host copies of the last run's status / summary / row_off, once per run (synchronises `st` then): what the item offsets are
// is only known on the device
static int solve_batch_host_copies(PwSolveBatch* b, hipStream_t st, const char* fn) {
  if (b->host_valid) return PW_OK;
  const size_t n = static_cast<size_t>(b->n);
  b->h_status.resize(n);
  b->h_summary.resize(n * 5);
  b->h_row_off.resize(n);
  hipError_t err = hipMemcpyAsync(b->h_status.data(), b->d_status, n, hipMemcpyDeviceToHost, st);
  if (err == hipSuccess) err = hipMemcpyAsync(b->h_summary.data(), b->d_summary, n * 20, hipMemcpyDeviceToHost, st);
  if (err == hipSuccess) err = hipMemcpyAsync(b->h_row_off.data(), b->d_row_off, n * 8, hipMemcpyDeviceToHost, st);
  if (err == hipSuccess) err = hipStreamSynchronize(st);
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string(fn) + ": " + hipGetErrorString(err));
  b->host_valid = true;
  return PW_OK;
}

static void solve_batch_free_items(PwSolveBatch* b) {
  void* bufs[] = {b->d_slots, b->d_status, b->d_summary, b->d_row_off, b->d_slot_off, b->d_slot_log2};
  for (void* p : bufs)
    if (p) (void)hipFree(p);
  b->d_slots = nullptr;
  b->d_status = nullptr;
  b->d_summary = nullptr;
  b->d_row_off = nullptr;
  b->d_slot_off = nullptr;
  b->d_slot_log2 = nullptr;
  b->n_cap = 0;
  b->slots_cap = 0;
}

extern "C" {

void pw_solve_batch_destroy(PwSolveBatch* b) {
  if (!b) return;
  PwDeviceGuard guard(b->eng->set->device);
  solve_batch_free_items(b);
  solve_batch_free_index(b);
  void* bufs[] = {b->d_key, b->d_succ, b->d_cost, b->d_acts, b->d_item_of_puzzle, b->d_counters};
  for (void* p : bufs)
    if (p) (void)hipFree(p);
  delete b;
}

int pw_solve_batch_create(PwEngine* e, int64_t rows_cap, PwSolveBatch** out) try {
  if (!e) return pw_fail(PW_EINVAL, "pw_solve_batch_create: null engine");
  if (!out) return pw_fail(PW_EINVAL, "pw_solve_batch_create: null out");
  if (rows_cap < 0 || rows_cap > (1ll << 40)) return pw_fail(PW_EINVAL, "pw_solve_batch_create: rows_cap must be in 0 .. 2^40");
  if (!e->d_ovl || !e->d_ovl_dir)
    return pw_fail(PW_EINVAL, "pw_solve_batch_create needs the engine's overlap tables (PW_OPT_STEP_TABLES)");
  PwSolveBatch* b = new (std::nothrow) PwSolveBatch();
  if (!b) return pw_fail(PW_ENOMEM, "out of memory");
  b->eng = e;
  b->rows_cap = rows_cap;
  PwDeviceGuard guard(e->set->device);
  PwHipChain c(guard.status());
  const size_t rows = static_cast<size_t>(rows_cap);
  c.alloc_nonzero(&b->d_key, rows * 8);
  c.alloc_nonzero(&b->d_succ, rows * 16);
  c.alloc_nonzero(&b->d_cost, rows * 2);
  c.alloc_nonzero(&b->d_acts, rows);
  c.alloc_nonzero(&b->d_item_of_puzzle, static_cast<size_t>(e->set->count) * 4);
  c.alloc_nonzero(&b->d_counters, 32);
  if (!c.ok()) {
    pw_solve_batch_destroy(b);
    return pw_hip_fail("pw_solve_batch_create", c.err);
  }
  *out = b;
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_solve_batch_run(PwSolveBatch* b, const int32_t* puzzles, int32_t n, int64_t max_states_each, void* stream) try {
  if (!b) return pw_fail(PW_EINVAL, "pw_solve_batch_run: null handle");
  if (n < 1) return pw_fail(PW_EINVAL, "pw_solve_batch_run: n must be >= 1");
  if (max_states_each < 1 || max_states_each > (1ll << 28))
    return pw_fail(PW_EINVAL, "pw_solve_batch_run: max_states_each must be in 1 .. 2^28");
  PwEngine* e = b->eng;
  PwDeviceGuard guard(e->set->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  b->host_valid = false;
  b->index_valid = false;  // the cost index goes with the run it was built from (its arrays are freed by the next build)
  if (n > b->n_cap) {  // the per-item arrays and the lookup pool (4 slots per row + 16 per item always hold what the rows hold)
    if (hipStreamSynchronize(st) != hipSuccess) return pw_fail(PW_EDEVICE, "pw_solve_batch_run: stream error");
    solve_batch_free_items(b);
    b->n = 0;
    const size_t items = static_cast<size_t>(n);
    const int64_t slots_cap = b->rows_cap ? 4 * b->rows_cap + 16 * static_cast<int64_t>(n) : 0;
    PwHipChain c;
    c.alloc_nonzero(&b->d_slots, static_cast<size_t>(slots_cap) * 4);
    c.alloc_nonzero(&b->d_status, items);
    c.alloc_nonzero(&b->d_summary, items * 20);
    c.alloc_nonzero(&b->d_row_off, items * 8);
    c.alloc_nonzero(&b->d_slot_off, items * 8);
    c.alloc_nonzero(&b->d_slot_log2, items);
    if (!c.ok()) {
      solve_batch_free_items(b);
      return pw_hip_fail("pw_solve_batch_run", c.err);
    }
    b->n_cap = n;
    b->slots_cap = slots_cap;
  }
  SolveBatchArgs a;
  a.hdrs = e->set->d_headers;
  a.blob = e->set->d_blob;
  a.ovl = e->d_ovl;
  a.ovl_dir = e->d_ovl_dir;
  a.puzzles = puzzles;
  a.n = n;
  a.num_puzzles = e->set->count;
  a.max_states = static_cast<uint32_t>(max_states_each);
  // slab of one workgroup: the state store, succ, cost, then tables of 2^16, 2^20, 2^22 ... slots up to >= 2 * max_states,
  // 12 bytes per slot (the key and the store index of its state)
  uint64_t off = pw_pad256(static_cast<uint64_t>(max_states_each) * 8);
  a.succ_off = off;
  off += pw_pad256(static_cast<uint64_t>(max_states_each) * 16);
  a.cost_off = off;
  off += pw_pad256(static_cast<uint64_t>(max_states_each) * 2);
  a.slab_bytes = pw_bs_ladder(static_cast<uint64_t>(max_states_each), PW_BS_LDS_SLOTS, 12, off, a.level_slots, a.level_off);
  // persistent workgroups by pw_search_batch's rule; the slabs are the engine's, shared with pw_search_batch
  int64_t groups = 0;
  if (int rc = engine_search_slab(e, n, a.slab_bytes, st, "pw_solve_batch_run", &groups, &a.slab, &a.next)) return rc;
  a.counters = b->d_counters;
  a.status = b->d_status;
  a.summary = b->d_summary;
  a.row_off = b->d_row_off;
  a.slot_off = b->d_slot_off;
  a.slot_log2 = b->d_slot_log2;
  a.item_of_puzzle = b->d_item_of_puzzle;
  a.rows_cap = b->rows_cap;
  a.slots_cap = b->slots_cap;
  a.pool_key = b->d_key;
  a.pool_succ = b->d_succ;
  a.pool_cost = b->d_cost;
  a.pool_acts = b->d_acts;
  a.pool_slots = b->d_slots;
  hipError_t err = hipMemsetAsync(a.next, 0, 4, st);
  if (err == hipSuccess) err = hipMemsetAsync(b->d_counters, 0, 32, st);
  if (err == hipSuccess) err = hipMemsetAsync(b->d_item_of_puzzle, 0xFF, static_cast<size_t>(e->set->count) * 4, st);
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string("pw_solve_batch_run: ") + hipGetErrorString(err));
  hipLaunchKernelGGL(pw_solve_batch_kernel, dim3(static_cast<unsigned>(groups)), dim3(256), 0, st, a);
  b->n = n;
  return check_launch("pw_solve_batch_run");
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_solve_batch_results(PwSolveBatch* b, const uint8_t** status, const int32_t** summary, const int64_t** row_off) try {
  if (!b) return pw_fail(PW_EINVAL, "pw_solve_batch_results: null handle");
  if (b->n < 1) return pw_fail(PW_EINVAL, "pw_solve_batch_results: no run yet (call pw_solve_batch_run)");
  if (status) *status = b->d_status;
  if (summary) *summary = b->d_summary;
  if (row_off) *row_off = b->d_row_off;
  return b->n;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_solve_batch_copy_results(PwSolveBatch* b, uint8_t* status, int32_t* summary, int64_t* row_off, void* stream) try {
  if (!b) return pw_fail(PW_EINVAL, "pw_solve_batch_copy_results: null handle");
  if (b->n < 1) return pw_fail(PW_EINVAL, "pw_solve_batch_copy_results: no run yet (call pw_solve_batch_run)");
  PwDeviceGuard guard(b->eng->set->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t n = static_cast<size_t>(b->n);
  hipError_t err = hipSuccess;
  if (status) err = hipMemcpyAsync(status, b->d_status, n, hipMemcpyDeviceToDevice, st);
  if (err == hipSuccess && summary) err = hipMemcpyAsync(summary, b->d_summary, n * 20, hipMemcpyDeviceToDevice, st);
  if (err == hipSuccess && row_off) err = hipMemcpyAsync(row_off, b->d_row_off, n * 8, hipMemcpyDeviceToDevice, st);
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string("pw_solve_batch_copy_results: ") + hipGetErrorString(err));
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_solve_batch_totals(PwSolveBatch* b, int64_t totals[3], void* stream) try {
  if (!b) return pw_fail(PW_EINVAL, "pw_solve_batch_totals: null handle");
  if (!totals) return pw_fail(PW_EINVAL, "pw_solve_batch_totals: null totals");
  if (b->n < 1) return pw_fail(PW_EINVAL, "pw_solve_batch_totals: no run yet (call pw_solve_batch_run)");
  PwDeviceGuard guard(b->eng->set->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  unsigned long long host[3] = {0, 0, 0};
  hipError_t err = hipMemcpyAsync(host, b->d_counters, sizeof(host), hipMemcpyDeviceToHost, st);
  if (err == hipSuccess) err = hipStreamSynchronize(st);
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string("pw_solve_batch_totals: ") + hipGetErrorString(err));
  for (int k = 0; k < 3; k++) totals[k] = static_cast<int64_t>(host[k]);
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_solve_batch_read(PwSolveBatch* b, int32_t item, int64_t first, int64_t count, uint64_t* key, int32_t* succ,
                        uint16_t* cost, uint8_t* acts, void* stream) try {
  if (!b) return pw_fail(PW_EINVAL, "pw_solve_batch_read: null handle");
  if (b->n < 1) return pw_fail(PW_EINVAL, "pw_solve_batch_read: no run yet (call pw_solve_batch_run)");
  if (item < 0 || item >= b->n) return pw_fail(PW_EINVAL, "pw_solve_batch_read: item out of bounds");
  if (first < 0 || count < 0) return pw_fail(PW_EINVAL, "pw_solve_batch_read: row range out of bounds");
  PwDeviceGuard guard(b->eng->set->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (int rc = solve_batch_host_copies(b, st, "pw_solve_batch_read")) return rc;
  const size_t it = static_cast<size_t>(item);
  if (b->h_status[it] != PW_SB_BUILT || b->h_row_off[it] < 0)
    return pw_fail(PW_EINVAL, "pw_solve_batch_read: the item has no stored rows (status " + std::to_string(b->h_status[it]) + ")");
  if (first + count > b->h_summary[it * 5]) return pw_fail(PW_EINVAL, "pw_solve_batch_read: row range out of bounds");
  if (count == 0) return PW_OK;
  const int64_t base = b->h_row_off[it] + first;
  const size_t c = static_cast<size_t>(count);
  hipError_t err = hipSuccess;
  if (key) err = hipMemcpyAsync(key, b->d_key + base, c * 8, hipMemcpyDeviceToDevice, st);
  if (err == hipSuccess && succ) err = hipMemcpyAsync(succ, b->d_succ + base * 4, c * 16, hipMemcpyDeviceToDevice, st);
  if (err == hipSuccess && cost) err = hipMemcpyAsync(cost, b->d_cost + base, c * 2, hipMemcpyDeviceToDevice, st);
  if (err == hipSuccess && acts) err = hipMemcpyAsync(acts, b->d_acts + base, c, hipMemcpyDeviceToDevice, st);
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string("pw_solve_batch_read: ") + hipGetErrorString(err));
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_solve_batch_query(PwSolveBatch* b, const int32_t* puzzle_id, const int8_t* pos, int32_t npad, const uint8_t* mask,
                         int32_t n, int32_t* index, int32_t* cost, uint8_t* acts, void* stream) try {
  if (!b) return pw_fail(PW_EINVAL, "pw_solve_batch_query: null handle");
  if (n < 1) return pw_fail(PW_EINVAL, "pw_solve_batch_query: n must be >= 1");
  if (!puzzle_id) return pw_fail(PW_EINVAL, "pw_solve_batch_query: null puzzle_id");
  if (!pos) return pw_fail(PW_EINVAL, "pw_solve_batch_query: null pos");
  if (int rc = pw_check_npad("pw_solve_batch_query: ", npad)) return rc;
  if (b->n < 1) return pw_fail(PW_EINVAL, "pw_solve_batch_query: no run yet (call pw_solve_batch_run)");
  PwDeviceGuard guard(b->eng->set->device);
  SolveBatchQueryArgs a;
  a.t = solve_batch_tables(b);
  a.puzzle_id = puzzle_id;
  a.pos = pos;
  a.item_mask = mask;
  a.npad = npad;
  a.n = n;
  a.out_index = index;
  a.out_cost = cost;
  a.out_acts = acts;
  const dim3 grid(static_cast<unsigned>((static_cast<int64_t>(n) + 255) / 256)), block(256);
  hipLaunchKernelGGL(pw_solve_batch_query_kernel, grid, block, 0, static_cast<hipStream_t>(stream), a);
  return check_launch("pw_solve_batch_query");
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

}  // extern "C"

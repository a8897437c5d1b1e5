// pw_table_sample.inc -- drawing from the cost-to-go tables on the device (DESIGN.md K14).
// Included from pw_kernels.hip after pw_solution_batch.inc (uses PwSearch, PwSolveBatch, pw_bs_unpack and mix64).
//
// K12 (pw_search_solve) and K13 (pw_solve_batch_run) leave exact tables in device memory and answer lookups.  This file makes
// them a data source:
//   cost index   the rows of every stored table grouped by cost-to-go: rows_by_cost (a permutation of the table's rows, cost 0
//                first, the dead ends last) and cost_start (bucket c = [cost_start[c], cost_start[c + 1])) -- a histogram, a
//                scan and a scatter with atomics, three launches for all tables of a handle;
//   sample       one thread per environment draws a row uniformly from a band of costs and writes its state as a reset would;
//   plans        one thread per item walks acts / succ from a row down to cost 0.
// The kernels are written once, against a TABLE VIEW: where succ / cost / acts and the index of the table of an item live, its
// first row, and how a row decodes into a state.  kBatch = true resolves the view per item from the puzzle id (K13: rows of
// a pool, the state is the 64-bit key), kBatch = false is the one table of a search (K12: the state is the store's row).
// The draws over pushes (pw_push_draw.inc and its users, K20 / K26) share the stream constants, the three state helpers, the scan
// kernel and table_sample_checks of this file.

#define PW_TABLE_K_SAMPLE 0xA0761D6478BD642Full  // seed ^ this: the stream of the sample draws (include/pushworld_amd.h)
#define PW_TABLE_K_PLAN 0xE7037ED1A0B428DBull    // seed ^ this: the stream of the tie breaks of the plans

// Where the tables of a handle live.  Members of the other form are NULL / 0.
struct TableSrc {
  const int32_t* succ;   // [rows][4]
  const uint16_t* cost;  // [rows]
  const uint8_t* acts;   // [rows]
  int32_t* rows_by_cost;  // [rows]: the cost index, next to the rows it permutes (row numbers within the table)
  uint32_t* cost_start;   // K12: [max_cost + 3]; K13: ragged over the items, item i at cs_off[i]
  // K13: one table per stored item
  const PwPuzzleHeader* hdrs;
  const int32_t* item_of_puzzle;  // [num_puzzles], -1: no stored table
  const int64_t* row_off;         // [items]
  const int32_t* summary;         // [items][5]: states, goal states, dead ends, largest finite cost, cost of the start
  const int64_t* cs_off;          // [items]: where the item's cost_start begins, -1 when it has none
  const unsigned long long* key;  // [rows]: the state word
  int32_t num_puzzles, items;
  // K12: the one table
  const uint32_t* states;  // [rows][nw]: two movables per word, x | y << 8 each (the engine's int8 pairs)
  int64_t rows;
  int32_t puzzle, nw, n_mov, max_cost;
};

struct TableView {
  int64_t base;        // first row of the table in succ / cost / acts / rows_by_cost / key
  int64_t rows;
  uint32_t* cs;        // its cost_start: max_cost + 3 entries
  int32_t max_cost, n_mov;
};

// the table `item` (K13) / the table (K12); false: nothing stored or indexed there
template <bool kBatch>
__device__ __forceinline__ bool table_view_of_item(const TableSrc& s, int32_t item, TableView& v) {
  if (kBatch) {
    if (item < 0 || item >= s.items) return false;
    v.base = s.row_off[item];
    if (v.base < 0) return false;
    v.cs = nullptr;
    if (s.cs_off) {  // (NULL: no index yet -- the plans do without)
      const int64_t off = s.cs_off[item];
      if (off < 0) return false;
      v.cs = s.cost_start + off;
    }
    v.rows = s.summary[static_cast<int64_t>(item) * 5];
    v.max_cost = s.summary[static_cast<int64_t>(item) * 5 + 3];
    v.n_mov = 0;  // (the caller knows the puzzle)
    return true;
  }
  v.base = 0;
  v.rows = s.rows;
  v.max_cost = s.max_cost;
  v.cs = s.cost_start;
  v.n_mov = s.n_mov;
  return true;
}

// the table that answers for environment i; false: another table's environment (the caller leaves it untouched)
template <bool kBatch>
__device__ __forceinline__ bool table_view_of_env(const TableSrc& s, const int32_t* puzzle_id, int64_t i, TableView& v) {
  if (kBatch) {
    const int32_t pid = puzzle_id[i];
    if (pid < 0 || pid >= s.num_puzzles) return false;
    if (!table_view_of_item<true>(s, s.item_of_puzzle[pid], v)) return false;
    v.n_mov = s.hdrs[pid].N;
    return true;
  }
  if (puzzle_id && puzzle_id[i] != s.puzzle) return false;
  return table_view_of_item<false>(s, 0, v);
}

// The three state helpers of every draw (K14 here, K20 / K26 in pw_push_draw.inc).  A state in the engine's layout is 16 words of
// two movables each (x, y int8 pairs), zeros from movable n_mov on.
// store words -> state: `nw` words at src, two movables per word
__device__ __forceinline__ void table_store_state(const uint32_t* src, int nw, int n_mov, uint32_t (&w)[16]) {
#pragma unroll
  for (int k = 0; k < 16; k++) {
    uint32_t word = 0u;
    if (k < nw && 2 * k < n_mov) {
      word = src[k];
      if (2 * k + 1 >= n_mov) word &= 0xffffu;
    }
    w[k] = word;
  }
}

// 64-bit key -> state (the key holds zeros beyond the puzzle's movables)
__device__ __forceinline__ void table_key_state(uint64_t key, uint32_t (&w)[16]) {
  uint32_t P[4];
  pw_bs_unpack(key, P);
#pragma unroll
  for (int k = 0; k < 16; k++) w[k] = k < 4 ? P[k] : 0u;
}

// state -> npad pairs at dst, with 8-byte (npad 4) or 16-byte stores
__device__ __forceinline__ void table_write_state(int8_t* dst, int32_t npad, const uint32_t (&w)[16]) {
  if (npad == 4) {
    *reinterpret_cast<uint2*>(dst) = make_uint2(w[0], w[1]);
  } else {
#pragma unroll
    for (int q = 0; q < 4; q++)
      if (8 * q < npad) reinterpret_cast<uint4*>(dst)[q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
  }
}

// row -> state
template <bool kBatch>
__device__ __forceinline__ void table_row_state(const TableSrc& s, const TableView& v, int64_t row, uint32_t (&w)[16]) {
  if (kBatch)
    table_key_state(s.key[v.base + row], w);
  else
    table_store_state(s.states + row * s.nw, s.nw, v.n_mov, w);
}

// ---- cost index ---------------------------------------------------------------------------------------------------------------
// Bucket of a row: its cost, the dead ends (0xFFFF) as bucket max_cost + 1.  With m = max_cost + 3 words per table:
//   histogram   word b + 2 counts bucket b (b <= max_cost; the last bucket's count is never needed)
//   scan        inclusive, in place: word b + 1 = rows in the buckets below b = the start of bucket b
//   scatter     word b + 1 is bucket b's cursor (atomicAdd); when every row is placed it holds the start of bucket b + 1
// so the words end as cost_start itself, without a second array.  Which row of a bucket gets which place is the schedule's.
// Workgroup g works on table g / chunks, rows (g % chunks) * 256 + tid, + chunks * 256, ...
template <bool kBatch>
__global__ __launch_bounds__(256) void pw_table_index_count_kernel(TableSrc s, uint32_t chunks) {
  TableView v;
  if (!table_view_of_item<kBatch>(s, static_cast<int32_t>(blockIdx.x / chunks), v)) return;
  const int64_t stride = static_cast<int64_t>(chunks) * 256;
  for (int64_t r = static_cast<int64_t>(blockIdx.x % chunks) * 256 + threadIdx.x; r < v.rows; r += stride) {
    const uint32_t c = s.cost[v.base + r];
    if (c <= static_cast<uint32_t>(v.max_cost)) atomicAdd(&v.cs[c + 2u], 1u);
  }
}

// The scan of every cost index (K14 both forms, K20, K26): one workgroup per table, in place and inclusive.  The pooled tables of a
// batch: table g's words start at cs_off[g] (< 0: nothing stored or indexed there) and are max_cost[g * stride] + 3 of them.  The one
// table of a search: cs_off and max_cost are NULL, the words start at 0 and are max_cost_one + 3.
__global__ __launch_bounds__(256) void pw_table_index_scan_kernel(uint32_t* cost_start, const int64_t* cs_off, const int32_t* max_cost,
                                                                   int32_t stride, int32_t max_cost_one) {
  __shared__ uint32_t part[256];
  const int64_t off = cs_off ? cs_off[blockIdx.x] : 0;
  if (off < 0) return;  // (workgroup-uniform)
  uint32_t* cs = cost_start + off;
  const int32_t mc = max_cost ? max_cost[static_cast<int64_t>(blockIdx.x) * stride] : max_cost_one;
  const uint32_t m = static_cast<uint32_t>(mc) + 3u, tid = threadIdx.x;
  uint32_t carry = 0;
  for (uint32_t c0 = 0; c0 < m; c0 += 256u) {
    const uint32_t k = c0 + tid;
    part[tid] = k < m ? cs[k] : 0u;
    __syncthreads();
    for (uint32_t d = 1; d < 256u; d <<= 1) {
      const uint32_t t = tid >= d ? part[tid - d] : 0u;
      __syncthreads();
      part[tid] += t;
      __syncthreads();
    }
    if (k < m) cs[k] = part[tid] + carry;
    carry += part[255];
    __syncthreads();  // (part is rewritten by the next round)
  }
}

template <bool kBatch>
__global__ __launch_bounds__(256) void pw_table_index_scatter_kernel(TableSrc s, uint32_t chunks) {
  TableView v;
  if (!table_view_of_item<kBatch>(s, static_cast<int32_t>(blockIdx.x / chunks), v)) return;
  const int64_t stride = static_cast<int64_t>(chunks) * 256;
  for (int64_t r = static_cast<int64_t>(blockIdx.x % chunks) * 256 + threadIdx.x; r < v.rows; r += stride) {
    const uint32_t c = s.cost[v.base + r];
    const uint32_t b = c <= static_cast<uint32_t>(v.max_cost) ? c : static_cast<uint32_t>(v.max_cost) + 1u;
    const uint32_t at = atomicAdd(&v.cs[b + 1u], 1u);
    if (at < v.rows) s.rows_by_cost[v.base + at] = static_cast<int32_t>(r);  // (always, for a table whose summary is its own)
  }
}

// ---- sample: one start state per environment, drawn from a band of costs ---------------------------------------------------------
struct TableSampleArgs {
  TableSrc src;
  const int32_t* puzzle_id;  // [n]; K12: or NULL
  const uint8_t* item_mask;  // [n] or NULL
  int32_t npad, n;
  uint64_t seed;
  uint32_t* counter;         // [n]
  int32_t lo, hi;            // the band, unless ...
  const int32_t* lo_n;       // ... [n] each: a band per environment
  const int32_t* hi_n;
  int8_t* pos;               // [n][npad][2]
  int32_t* steps;
  uint8_t* term;             // or NULL
  uint8_t* trunc;            // or NULL
  int32_t* out_row;
  int32_t* out_cost;
};

template <bool kBatch>
__global__ __launch_bounds__(256) void pw_table_sample_kernel(TableSampleArgs a) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= a.n) return;
  if (a.item_mask && a.item_mask[i] == 0) return;
  TableView v;
  if (!table_view_of_env<kBatch>(a.src, a.puzzle_id, i, v)) return;  // another table's environment: untouched
  if (v.n_mov > a.npad) return;                                      // (a state that does not fit the layout: no table here)
  const int32_t mc = v.max_cost;
  const uint32_t finite = v.cs[mc + 1];  // rows below the dead-end bucket
  if (finite == 0u) {                    // nothing can be solved from any state of this puzzle
    a.out_row[i] = -1;
    a.out_cost[i] = -1;
    return;
  }
  int32_t lo = a.lo_n ? a.lo_n[i] : a.lo, hi = a.hi_n ? a.hi_n[i] : a.hi;
  hi = max(hi, lo);
  lo = min(max(lo, 0), mc);
  hi = min(max(hi, 0), mc);
  const uint32_t first = v.cs[lo], count = v.cs[hi + 1] - first;
  if (count == 0u || first + count > v.rows) {  // (no table built by this library: every cost up to max_cost has a row)
    a.out_row[i] = -1;
    a.out_cost[i] = -1;
    return;
  }
  const uint32_t ctr = a.counter[i] + 1u;
  a.counter[i] = ctr;
  const uint64_t r = mix64(a.seed ^ PW_TABLE_K_SAMPLE, static_cast<uint64_t>(i), ctr);
  // floor(r * count / 2^64): uniform over the band's rows to 2^-32
  const uint32_t u = static_cast<uint32_t>(__umul64hi(r, static_cast<uint64_t>(count)));
  const int64_t row = a.src.rows_by_cost[v.base + first + u];
  uint32_t w[16];
  table_row_state<kBatch>(a.src, v, row, w);
  table_write_state(a.pos + i * a.npad * 2, a.npad, w);
  a.steps[i] = 0;
  if (a.term) a.term[i] = 0;
  if (a.trunc) a.trunc[i] = 0;
  a.out_row[i] = static_cast<int32_t>(row);
  a.out_cost[i] = static_cast<int32_t>(a.src.cost[v.base + row]);
}

// ---- plans: a shortest plan from every given row ---------------------------------------------------------------------------------
struct TablePlansArgs {
  TableSrc src;
  const int32_t* index;      // [n] rows, as the query returns them
  const int32_t* puzzle_id;  // [n]; K12: or NULL
  const uint8_t* item_mask;  // [n] or NULL
  int32_t n, tie, plan_cap;
  uint64_t seed;
  uint8_t* plans;            // [n][plan_cap]
  int32_t* plan_len;         // [n]
};

template <bool kBatch>
__global__ __launch_bounds__(256) void pw_table_plans_kernel(TablePlansArgs a) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= a.n) return;
  if (a.item_mask && a.item_mask[i] == 0) return;
  TableView v;
  int64_t cur = a.index[i];
  if (!table_view_of_env<kBatch>(a.src, a.puzzle_id, i, v) || cur < 0 || cur >= v.rows) {
    a.plan_len[i] = -1;
    return;
  }
  const uint32_t c = a.src.cost[v.base + cur];
  if (c == PW_SOLVE_INF) {
    a.plan_len[i] = -1;
    return;
  }
  if (c > static_cast<uint32_t>(a.plan_cap)) {
    a.plan_len[i] = -2;
    return;
  }
  uint8_t* plan = a.plans + i * a.plan_cap;
  uint32_t t = 0;
  for (; t < c; t++) {  // (a plan is as long as its start's cost: every step goes one cost down)
    uint32_t bits = a.src.acts[v.base + cur] & 15u;
    if (bits == 0u) break;  // (only at cost 0)
    if (a.tie) {
      const uint64_t r = mix64(a.seed ^ PW_TABLE_K_PLAN, static_cast<uint64_t>(i), t);
      const uint32_t j = static_cast<uint32_t>(__umul64hi(r, static_cast<uint64_t>(__popc(bits))));
      for (uint32_t q = 0; q < j; q++) bits &= bits - 1u;  // the j-th set bit
    }
    const int act = __ffs(bits) - 1;
    plan[t] = static_cast<uint8_t>(act);
    cur = a.src.succ[(v.base + cur) * 4 + act];
  }
  a.plan_len[i] = static_cast<int32_t>(t);
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
static TableSrc table_src(const PwSolveBatch* b) {
  TableSrc s = {};
  s.succ = b->d_succ;
  s.cost = b->d_cost;
  s.acts = b->d_acts;
  s.rows_by_cost = b->d_rows_by_cost;
  s.cost_start = b->d_cost_start;
  s.hdrs = b->eng->set->d_headers;
  s.item_of_puzzle = b->d_item_of_puzzle;
  s.row_off = b->d_row_off;
  s.summary = b->d_summary;
  s.cs_off = b->index_valid ? b->d_cs_off : nullptr;
  s.key = b->d_key;
  s.num_puzzles = b->eng->set->count;
  s.items = b->n;
  return s;
}

static TableSrc table_src(const PwSearch* p) {
  TableSrc s = {};
  s.succ = p->d_succ;
  s.cost = p->d_cost;
  s.acts = p->d_acts;
  s.rows_by_cost = p->d_rows_by_cost;
  s.cost_start = p->d_cost_start;
  s.states = p->d_states;
  s.rows = p->table_states;
  s.puzzle = p->puzzle;
  s.nw = p->NW;
  s.n_mov = p->N;
  s.max_cost = static_cast<int32_t>(p->table_max_cost);
  return s;
}

// the three launches of the index over `tables` tables of at most `max_rows` rows; cost_start is zero
template <bool kBatch>
static void table_index_launch(const TableSrc& s, int64_t tables, int64_t max_rows, hipStream_t st) {
  // rows of a table over up to 1024 workgroups (K12: one large table) -- or one workgroup per table when there are many
  int64_t chunks = std::min<int64_t>(1024, std::max<int64_t>(1, (max_rows + 1023) / 1024));
  while (chunks > 1 && tables * chunks > (1ll << 30)) chunks /= 2;
  const dim3 grid(static_cast<unsigned>(tables * chunks)), block(256);
  hipLaunchKernelGGL(pw_table_index_count_kernel<kBatch>, grid, block, 0, st, s, static_cast<uint32_t>(chunks));
  hipLaunchKernelGGL(pw_table_index_scan_kernel, dim3(static_cast<unsigned>(tables)), block, 0, st, s.cost_start, s.cs_off,
                     kBatch ? s.summary + 3 : nullptr, 5, s.max_cost);
  hipLaunchKernelGGL(pw_table_index_scatter_kernel<kBatch>, grid, block, 0, st, s, static_cast<uint32_t>(chunks));
}

// out_name: what the entry point calls the drawn index (out_row; the push tables' out_state)
static int table_sample_checks(const char* fn, int32_t n, int32_t npad, const uint32_t* counter, int32_t lo, int32_t hi,
                               const int32_t* lo_n, const int32_t* hi_n, const int8_t* pos, const int32_t* steps,
                               const int32_t* out_row, const int32_t* out_cost, const char* out_name = "out_row") {
  const std::string f(fn);
  if (n < 1) return pw_fail(PW_EINVAL, f + ": n must be >= 1");
  if (!pos) return pw_fail(PW_EINVAL, f + ": null pos");
  if (!steps) return pw_fail(PW_EINVAL, f + ": null steps");
  if (!counter) return pw_fail(PW_EINVAL, f + ": null counter");
  if (!out_row || !out_cost) return pw_fail(PW_EINVAL, f + ": null " + out_name + " / out_cost");
  if (int rc = pw_check_npad(f + ": ", npad)) return rc;
  if ((lo_n == nullptr) != (hi_n == nullptr)) return pw_fail(PW_EINVAL, f + ": the band arrays lo and hi come together");
  if (!lo_n && (lo < 0 || lo > hi)) return pw_fail(PW_EINVAL, f + ": the cost band needs 0 <= lo <= hi");
  return PW_OK;
}

static int table_plans_checks(const char* fn, const int32_t* index, int32_t n, int32_t tie, const uint8_t* plans,
                              int32_t plan_cap, const int32_t* plan_len) {
  const std::string f(fn);
  if (n < 1) return pw_fail(PW_EINVAL, f + ": n must be >= 1");
  if (!index) return pw_fail(PW_EINVAL, f + ": null index");
  if (!plans || !plan_len) return pw_fail(PW_EINVAL, f + ": null plans / plan_len");
  if (plan_cap < 1) return pw_fail(PW_EINVAL, f + ": plan_cap must be >= 1");
  if (tie != 0 && tie != 1) return pw_fail(PW_EINVAL, f + ": tie must be 0 (lowest) or 1 (uniform)");
  return PW_OK;
}

extern "C" {

int pw_solve_batch_index(PwSolveBatch* b, void* stream) try {
  if (!b) return pw_fail(PW_EINVAL, "pw_solve_batch_index: null handle");
  if (b->n < 1) return pw_fail(PW_EINVAL, "pw_solve_batch_index: no run yet (call pw_solve_batch_run)");
  if (b->index_valid) return PW_OK;
  PwDeviceGuard guard(b->eng->set->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (int rc = solve_batch_host_copies(b, st, "pw_solve_batch_index")) return rc;  // (the one synchronisation)
  const size_t n = static_cast<size_t>(b->n);
  b->h_cs_off.assign(n, -1);
  int64_t words = 0, max_rows = 0;
  for (size_t it = 0; it < n; it++) {
    if (b->h_status[it] != PW_SB_BUILT || b->h_row_off[it] < 0) continue;
    b->h_cs_off[it] = words;
    words += static_cast<int64_t>(b->h_summary[it * 5 + 3]) + 3;
    max_rows = std::max<int64_t>(max_rows, b->h_summary[it * 5]);
  }
  solve_batch_free_index(b);
  PwHipChain c;  // (no allocation of zero bytes: at least 16)
  const size_t cs_bytes = std::max<size_t>(static_cast<size_t>(words) * 4, 16);
  c.alloc(&b->d_rows_by_cost, std::max<size_t>(static_cast<size_t>(b->rows_cap) * 4, 16));
  c.alloc(&b->d_cost_start, cs_bytes);
  c.alloc(&b->d_cs_off, std::max<size_t>(n * 8, 16));
  c.then([&] { return hipMemsetAsync(b->d_cost_start, 0, cs_bytes, st); });
  c.then([&] { return hipMemcpyAsync(b->d_cs_off, b->h_cs_off.data(), n * 8, hipMemcpyHostToDevice, st); });
  if (!c.ok()) {
    solve_batch_free_index(b);
    return pw_hip_fail("pw_solve_batch_index", c.err);
  }
  if (words > 0) {
    TableSrc src = table_src(b);
    src.cs_off = b->d_cs_off;  // (not valid for the other entry points until the launches are queued)
    table_index_launch<true>(src, b->n, max_rows, st);
  }
  if (int rc = check_launch("pw_solve_batch_index")) {
    solve_batch_free_index(b);
    return rc;
  }
  b->index_valid = true;
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_solve_batch_index_read(PwSolveBatch* b, int32_t item, int32_t* rows_by_cost, uint32_t* cost_start, void* stream) try {
  if (!b) return pw_fail(PW_EINVAL, "pw_solve_batch_index_read: null handle");
  if (b->n < 1) return pw_fail(PW_EINVAL, "pw_solve_batch_index_read: no run yet (call pw_solve_batch_run)");
  if (!b->index_valid) return pw_fail(PW_EINVAL, "pw_solve_batch_index_read: no index yet (call pw_solve_batch_index)");
  if (item < 0 || item >= b->n) return pw_fail(PW_EINVAL, "pw_solve_batch_index_read: item out of bounds");
  const size_t it = static_cast<size_t>(item);
  if (b->h_cs_off[it] < 0)
    return pw_fail(PW_EINVAL, "pw_solve_batch_index_read: the item has no stored rows (status " + std::to_string(b->h_status[it]) + ")");
  PwDeviceGuard guard(b->eng->set->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t rows = static_cast<size_t>(b->h_summary[it * 5]), words = static_cast<size_t>(b->h_summary[it * 5 + 3]) + 3;
  hipError_t err = hipSuccess;
  if (rows_by_cost && rows)
    err = hipMemcpyAsync(rows_by_cost, b->d_rows_by_cost + b->h_row_off[it], rows * 4, hipMemcpyDeviceToDevice, st);
  if (err == hipSuccess && cost_start)
    err = hipMemcpyAsync(cost_start, b->d_cost_start + b->h_cs_off[it], words * 4, hipMemcpyDeviceToDevice, st);
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string("pw_solve_batch_index_read: ") + hipGetErrorString(err));
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_solve_batch_sample(PwSolveBatch* b, const int32_t* puzzle_id, const uint8_t* mask, int32_t n, int32_t npad, uint64_t seed,
                          uint32_t* counter, int32_t lo, int32_t hi, const int32_t* lo_n, const int32_t* hi_n, int8_t* pos,
                          int32_t* steps, uint8_t* term, uint8_t* trunc, int32_t* out_row, int32_t* out_cost, void* stream) try {
  if (!b) return pw_fail(PW_EINVAL, "pw_solve_batch_sample: null handle");
  if (!puzzle_id) return pw_fail(PW_EINVAL, "pw_solve_batch_sample: null puzzle_id");
  if (int rc = table_sample_checks("pw_solve_batch_sample", n, npad, counter, lo, hi, lo_n, hi_n, pos, steps, out_row, out_cost))
    return rc;
  if (b->n < 1) return pw_fail(PW_EINVAL, "pw_solve_batch_sample: no run yet (call pw_solve_batch_run)");
  if (!b->index_valid) return pw_fail(PW_EINVAL, "pw_solve_batch_sample: no index yet (call pw_solve_batch_index)");
  PwDeviceGuard guard(b->eng->set->device);
  TableSampleArgs a = {table_src(b), puzzle_id, mask, npad, n, seed, counter, lo, hi, lo_n, hi_n, pos, steps, term, trunc,
                       out_row, out_cost};
  const dim3 grid(static_cast<unsigned>((static_cast<int64_t>(n) + 255) / 256)), block(256);
  hipLaunchKernelGGL(pw_table_sample_kernel<true>, grid, block, 0, static_cast<hipStream_t>(stream), a);
  return check_launch("pw_solve_batch_sample");
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_solve_batch_plans(PwSolveBatch* b, const int32_t* index, const int32_t* puzzle_id, const uint8_t* mask, int32_t n,
                         int32_t tie, uint64_t seed, uint8_t* plans, int32_t plan_cap, int32_t* plan_len, void* stream) try {
  if (!b) return pw_fail(PW_EINVAL, "pw_solve_batch_plans: null handle");
  if (!puzzle_id) return pw_fail(PW_EINVAL, "pw_solve_batch_plans: null puzzle_id");
  if (int rc = table_plans_checks("pw_solve_batch_plans", index, n, tie, plans, plan_cap, plan_len)) return rc;
  if (b->n < 1) return pw_fail(PW_EINVAL, "pw_solve_batch_plans: no run yet (call pw_solve_batch_run)");
  PwDeviceGuard guard(b->eng->set->device);
  TablePlansArgs a = {table_src(b), index, puzzle_id, mask, n, tie, plan_cap, seed, plans, plan_len};
  const dim3 grid(static_cast<unsigned>((static_cast<int64_t>(n) + 255) / 256)), block(256);
  hipLaunchKernelGGL(pw_table_plans_kernel<true>, grid, block, 0, static_cast<hipStream_t>(stream), a);
  return check_launch("pw_solve_batch_plans");
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_search_table_index(PwSearch* s, void* stream) try {
  if (!s) return pw_fail(PW_EINVAL, "pw_search_table_index: null search");
  if (!s->solved) return pw_fail(PW_EINVAL, "pw_search_table_index: no table (call pw_search_solve after the search is exhausted)");
  if (s->index_valid) return PW_OK;
  PwDeviceGuard guard(s->eng->set->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t words = static_cast<size_t>(s->table_max_cost) + 3;
  hipError_t err = hipMalloc(reinterpret_cast<void**>(&s->d_rows_by_cost), static_cast<size_t>(s->table_states) * 4);
  if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&s->d_cost_start), words * 4);
  if (err == hipSuccess) err = hipMemsetAsync(s->d_cost_start, 0, words * 4, st);
  if (err != hipSuccess) {
    search_index_discard(s);
    return pw_hip_fail("pw_search_table_index", err);
  }
  table_index_launch<false>(table_src(s), 1, s->table_states, st);
  if (int rc = check_launch("pw_search_table_index")) {
    search_index_discard(s);
    return rc;
  }
  s->index_valid = true;
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_search_table_index_read(PwSearch* s, int32_t* rows_by_cost, uint32_t* cost_start, void* stream) try {
  if (!s) return pw_fail(PW_EINVAL, "pw_search_table_index_read: null search");
  if (!s->solved)
    return pw_fail(PW_EINVAL, "pw_search_table_index_read: no table (call pw_search_solve after the search is exhausted)");
  if (!s->index_valid) return pw_fail(PW_EINVAL, "pw_search_table_index_read: no index yet (call pw_search_table_index)");
  PwDeviceGuard guard(s->eng->set->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t err = hipSuccess;
  if (rows_by_cost)
    err = hipMemcpyAsync(rows_by_cost, s->d_rows_by_cost, static_cast<size_t>(s->table_states) * 4, hipMemcpyDeviceToDevice, st);
  if (err == hipSuccess && cost_start)
    err = hipMemcpyAsync(cost_start, s->d_cost_start, (static_cast<size_t>(s->table_max_cost) + 3) * 4, hipMemcpyDeviceToDevice, st);
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string("pw_search_table_index_read: ") + hipGetErrorString(err));
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_search_table_sample(PwSearch* s, const int32_t* puzzle_id, const uint8_t* mask, int32_t n, int32_t npad, uint64_t seed,
                           uint32_t* counter, int32_t lo, int32_t hi, const int32_t* lo_n, const int32_t* hi_n, int8_t* pos,
                           int32_t* steps, uint8_t* term, uint8_t* trunc, int32_t* out_row, int32_t* out_cost, void* stream) try {
  if (!s) return pw_fail(PW_EINVAL, "pw_search_table_sample: null search");
  if (int rc = table_sample_checks("pw_search_table_sample", n, npad, counter, lo, hi, lo_n, hi_n, pos, steps, out_row, out_cost))
    return rc;
  if (npad < s->N) return pw_fail(PW_EINVAL, "pw_search_table_sample: npad is smaller than the puzzle's number of movables");
  if (!s->solved) return pw_fail(PW_EINVAL, "pw_search_table_sample: no table (call pw_search_solve after the search is exhausted)");
  if (!s->index_valid) return pw_fail(PW_EINVAL, "pw_search_table_sample: no index yet (call pw_search_table_index)");
  PwDeviceGuard guard(s->eng->set->device);
  TableSampleArgs a = {table_src(s), puzzle_id, mask, npad, n, seed, counter, lo, hi, lo_n, hi_n, pos, steps, term, trunc,
                       out_row, out_cost};
  const dim3 grid(static_cast<unsigned>((static_cast<int64_t>(n) + 255) / 256)), block(256);
  hipLaunchKernelGGL(pw_table_sample_kernel<false>, grid, block, 0, static_cast<hipStream_t>(stream), a);
  return check_launch("pw_search_table_sample");
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_search_table_plans(PwSearch* s, const int32_t* index, const int32_t* puzzle_id, const uint8_t* mask, int32_t n,
                          int32_t tie, uint64_t seed, uint8_t* plans, int32_t plan_cap, int32_t* plan_len, void* stream) try {
  if (!s) return pw_fail(PW_EINVAL, "pw_search_table_plans: null search");
  if (int rc = table_plans_checks("pw_search_table_plans", index, n, tie, plans, plan_cap, plan_len)) return rc;
  if (!s->solved) return pw_fail(PW_EINVAL, "pw_search_table_plans: no table (call pw_search_solve after the search is exhausted)");
  PwDeviceGuard guard(s->eng->set->device);
  TablePlansArgs a = {table_src(s), index, puzzle_id, mask, n, tie, plan_cap, seed, plans, plan_len};
  const dim3 grid(static_cast<unsigned>((static_cast<int64_t>(n) + 255) / 256)), block(256);
  hipLaunchKernelGGL(pw_table_plans_kernel<false>, grid, block, 0, static_cast<hipStream_t>(stream), a);
  return check_launch("pw_search_table_plans");
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

}  // extern "C"

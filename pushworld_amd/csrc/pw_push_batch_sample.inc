// pw_push_batch_sample.inc -- K26: drawing from the BATCHED cost-to-go tables over pushes on the device (DESIGN.md K26).
// Part of the single translation unit pw_kernels.hip, included there after pw_push_solution_batch.inc (uses PwPushSolveBatch and
// its pools, pw_bs_unpack, the stream constants and the argument checks of pw_table_sample.inc, push_table_bucket and
// push_table_store_words of pw_push_table_sample.inc, mix64 and rocprim's radix sort).
//
// K22 (pw_push_solve_batch_run) leaves the tables of many small puzzles in two pools.  This file makes them a data source, in the
// form K20 gave the one-puzzle table and K14 gave the move-level batch:
//   cost index   per stored item the STATES grouped by cost-to-go: states_by_cost (a permutation of the item's state numbers,
//                cost 0 first, the dead ends last, ASCENDING 64-BIT KEY inside a bucket) and cost_start.  K22's state numbers
//                inside a layer are the schedule's, the key -- the packed canonical state -- is not: position p of a bucket
//                holds the same STATE in every run.  One key kernel ((bucket word of the item) << 32 | state number per state,
//                and the histogram), a stable radix sort by key, a stable radix sort by the bucket word, one kernel that
//                keeps the state numbers, one scan per item;
//   sample       ONE launch for a mixed batch, one thread per environment: a state drawn uniformly from a band of costs of the
//                environment's own item and written as a reset would;
//   plans        ONE launch, one thread per item: best / the optimal rows and succ from a state down to cost 0;
//   emit         ONE launch, one thread per (item, step): one flat demonstration row, read off the keys -- no flood and no step.
// A node's key IS its canonical state, so the unpacked key (zeros beyond the puzzle's N: pw_sb_keep) is the state.
// Every loop is bounded by the items, a state's rows, plan_cap, the start's cost or an item's max_cost + 3 words.  No kernel
// waits on another workgroup, there is no device assert, and every store is a plain or vector store.

struct PushBatchDrawSrc {
  const PwPuzzleHeader* hdrs;
  int32_t num_puzzles;
  const int32_t* item_of_puzzle;  // [num_puzzles], -1: no stored table
  const int32_t* summary;         // [items][6]
  const int64_t* state_off;       // [items]
  const int64_t* row_off;
  const unsigned long long* pool_key;
  const int64_t* pool_srow;
  const int32_t* pool_cost;
  const int32_t* pool_best;
  const int32_t* pool_succ;
  const uint16_t* pool_from;
  const uint8_t* pool_action;
  const uint8_t* pool_flags;
  const int64_t* ix_off;          // [items], or NULL: no index
  const int64_t* cs_off;
  const int32_t* states_by_cost;
  const uint32_t* cost_start;
};

// the stored item that answers for puzzle `pid`, -1: none here
__device__ __forceinline__ int32_t push_batch_item(const PushBatchDrawSrc& s, int32_t pid) {
  if (pid < 0 || pid >= s.num_puzzles) return -1;
  const int32_t item = s.item_of_puzzle[pid];
  return item >= 0 && s.state_off[item] >= 0 && s.row_off[item] >= 0 ? item : -1;
}

// key -> the engine's layout: 16 words of two movables each (the key holds zeros beyond the puzzle's movables)
__device__ __forceinline__ void push_batch_key_words(uint64_t key, uint32_t (&w)[16]) {
  uint32_t P[4];
  pw_bs_unpack(key, P);
#pragma unroll
  for (int k = 0; k < 16; k++) w[k] = k < 4 ? P[k] : 0u;
}

// ---- cost index ---------------------------------------------------------------------------------------------------------------
// Workgroup g works on item g / chunks, states (g % chunks) * 256 + tid, + chunks * 256, ...  State r of an item whose index
// starts at ix and whose cost_start starts at word cs: key[ix + r] = its 64-bit key, val[ix + r] = (cs + bucket) << 32 | r, and
// word cs + bucket + 1 counts the bucket.  (cs + bucket ascends with (item, bucket): the second sort groups by both at once.)
__global__ __launch_bounds__(256) void pw_push_batch_index_key_kernel(PushBatchDrawSrc s, int32_t items, uint32_t chunks,
                                                                       uint32_t* cost_start, unsigned long long* key,
                                                                       unsigned long long* val) {
  const int32_t item = static_cast<int32_t>(blockIdx.x / chunks);
  if (item >= items) return;
  const int64_t ix = s.ix_off[item];
  if (ix < 0) return;
  const int64_t cs = s.cs_off[item], base = s.state_off[item];
  const int64_t S = s.summary[static_cast<int64_t>(item) * 6];
  const int32_t mc = s.summary[static_cast<int64_t>(item) * 6 + 4];
  const int64_t stride = static_cast<int64_t>(chunks) * 256;
  for (int64_t r = static_cast<int64_t>(blockIdx.x % chunks) * 256 + threadIdx.x; r < S; r += stride) {
    const uint32_t b = push_table_bucket(s.pool_cost[base + r], mc);
    key[ix + r] = s.pool_key[base + r];
    val[ix + r] = (static_cast<unsigned long long>(cs + b) << 32) | static_cast<unsigned long long>(r);
    atomicAdd(&cost_start[cs + b + 1u], 1u);
  }
}

__global__ __launch_bounds__(256) void pw_push_batch_index_keep_kernel(const unsigned long long* val, int64_t total,
                                                                        int32_t* states_by_cost) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i < total) states_by_cost[i] = static_cast<int32_t>(static_cast<uint32_t>(val[i]));
}

// one workgroup per item: the inclusive scan of its max_cost + 3 words, in place (K14's scan)
__global__ __launch_bounds__(256) void pw_push_batch_index_scan_kernel(PushBatchDrawSrc s, uint32_t* cost_start) {
  __shared__ uint32_t part[256];
  const int32_t item = static_cast<int32_t>(blockIdx.x);
  const int64_t cs_off = s.cs_off[item];
  if (cs_off < 0) return;  // (workgroup-uniform)
  uint32_t* cs = cost_start + cs_off;
  const uint32_t m = static_cast<uint32_t>(s.summary[static_cast<int64_t>(item) * 6 + 4] + 3), tid = threadIdx.x;
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

// ---- sample: one start state per environment, drawn from a band of costs of its own item ---------------------------------------
struct PushBatchSampleArgs {
  PushBatchDrawSrc src;
  const int32_t* puzzle_id;  // [n]
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
  int32_t* out_state;
  int32_t* out_cost;
};

__global__ __launch_bounds__(256) void pw_push_batch_sample_kernel(PushBatchSampleArgs a) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= a.n) return;
  if (a.item_mask && a.item_mask[i] == 0) return;
  const int32_t item = push_batch_item(a.src, a.puzzle_id[i]);
  if (item < 0) return;  // no stored table for this puzzle here: another table's environment, untouched
  const int64_t ix = a.src.ix_off[item];
  if (ix < 0) return;    // (a stored item is indexed: never)
  const int64_t S = a.src.summary[static_cast<int64_t>(item) * 6], sbase = a.src.state_off[item];
  const int32_t mc = a.src.summary[static_cast<int64_t>(item) * 6 + 4];
  const uint32_t* cs = a.src.cost_start + a.src.cs_off[item];
  const uint32_t finite = mc >= 0 ? cs[mc + 1] : 0u;  // states below the dead-end bucket
  if (finite == 0u) {  // nothing can be solved from any state of this item
    a.out_state[i] = -1;
    a.out_cost[i] = -1;
    return;
  }
  int32_t lo = a.lo_n ? a.lo_n[i] : a.lo, hi = a.hi_n ? a.hi_n[i] : a.hi;
  hi = max(hi, lo);
  lo = min(max(lo, 0), mc);
  hi = min(max(hi, 0), mc);
  const uint32_t first = cs[lo], end = cs[hi + 1];
  if (end <= first || end > S) {  // an empty band (an item without goal states in its store has no state of cost 0)
    a.out_state[i] = -1;
    a.out_cost[i] = -1;
    return;
  }
  const uint32_t count = end - first;
  const uint32_t ctr = a.counter[i] + 1u;
  a.counter[i] = ctr;
  const uint64_t r = mix64(a.seed ^ PW_TABLE_K_SAMPLE, static_cast<uint64_t>(i), ctr);
  // floor(r * count / 2^64): uniform over the band's states to 2^-32
  const uint32_t u = static_cast<uint32_t>(__umul64hi(r, static_cast<uint64_t>(count)));
  const int64_t state = a.src.states_by_cost[ix + first + u];
  if (state < 0 || state >= S) {  // (never, for an index built by this library)
    a.out_state[i] = -1;
    a.out_cost[i] = -1;
    return;
  }
  uint32_t w[16];
  push_batch_key_words(a.src.pool_key[sbase + state], w);
  push_table_store_words(a.pos + i * a.npad * 2, a.npad, w);
  a.steps[i] = 0;
  if (a.term) a.term[i] = 0;
  if (a.trunc) a.trunc[i] = 0;
  a.out_state[i] = static_cast<int32_t>(state);
  a.out_cost[i] = a.src.pool_cost[sbase + state];
}

// ---- plans: a fewest-pushes plan from every given state ------------------------------------------------------------------------
struct PushBatchPlansArgs {
  PushBatchDrawSrc src;
  const int32_t* index;      // [n] states within the item, as the query returns them
  const int32_t* puzzle_id;  // [n]
  const uint8_t* item_mask;  // [n] or NULL
  int32_t n, tie, plan_cap;
  uint64_t seed;
  int8_t* plan_from;         // [n][plan_cap][2]
  uint8_t* plan_action;      // [n][plan_cap]
  int32_t* plan_state;       // [n][plan_cap] or NULL
  int32_t* plan_len;         // [n]
};

__global__ __launch_bounds__(256) void pw_push_batch_plans_kernel(PushBatchPlansArgs a) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= a.n) return;
  if (a.item_mask && a.item_mask[i] == 0) return;
  const PushBatchDrawSrc& t = a.src;
  const int32_t item = push_batch_item(t, a.puzzle_id[i]);
  int64_t cur = a.index[i];
  const int64_t S = item >= 0 ? t.summary[static_cast<int64_t>(item) * 6] : 0;
  if (item < 0 || cur < 0 || cur >= S) {
    a.plan_len[i] = -1;
    return;
  }
  const int64_t sbase = t.state_off[item], rbase = t.row_off[item];
  const int32_t c = t.pool_cost[sbase + cur];
  if (c < 0) {
    a.plan_len[i] = -1;
    return;
  }
  if (c > a.plan_cap) {
    a.plan_len[i] = -2;
    return;
  }
  const int64_t base = i * a.plan_cap;
  int32_t step = 0;
  while (step < c) {  // (a plan is as long as its start's cost: every push goes one cost down)
    const int64_t r0 = rbase + t.pool_srow[sbase + cur], r1 = rbase + t.pool_srow[sbase + cur + 1];
    int64_t r = -1;
    if (a.tie) {
      uint32_t k = 0;
      for (int64_t q = r0; q < r1; q++) k += (t.pool_flags[q] >> 1) & 1u;
      if (k > 0u) {
        const uint64_t h = mix64(a.seed ^ PW_TABLE_K_PLAN, static_cast<uint64_t>(i), static_cast<uint64_t>(step));
        uint32_t j = static_cast<uint32_t>(__umul64hi(h, static_cast<uint64_t>(k)));
        for (int64_t q = r0; q < r1 && r < 0; q++)
          if (t.pool_flags[q] & 2) {
            if (j == 0u) r = q;
            j--;
          }
      }
    } else {
      const int32_t k = t.pool_best[sbase + cur];
      if (k >= 0 && r0 + k < r1) r = r0 + k;
    }
    if (r < 0) break;  // (only at cost 0: never inside the loop)
    reinterpret_cast<uint16_t*>(a.plan_from)[base + step] = t.pool_from[r];
    a.plan_action[base + step] = t.pool_action[r];
    if (a.plan_state) a.plan_state[base + step] = static_cast<int32_t>(cur);
    step++;
    if (t.pool_flags[r] & 1) break;  // a goal row ends the plan, whatever its successor is
    const int32_t nxt = t.pool_succ[r];
    if (nxt < 0 || nxt >= S) break;  // (an optimal row is safe: never)
    cur = nxt;
  }
  a.plan_len[i] = step;
}

// ---- emit: every push of every plan becomes one flat demonstration row -----------------------------------------------------------
struct PushBatchEmitArgs {
  PushBatchDrawSrc src;
  const int32_t* puzzle_id;  // [n]
  const uint8_t* item_mask;  // [n] or NULL
  int32_t n, npad, plan_cap;
  const int8_t* plan_from;
  const uint8_t* plan_action;
  const int32_t* plan_state;
  const int32_t* plan_len;
  const int8_t* pos;      // [n][npad][2] the items' live states, or NULL: the stored ones
  const int64_t* offset;  // [n + 1]
  int64_t rows_cap;
  int32_t* row_item;
  int32_t* row_t;
  int32_t* row_state;
  int8_t* row_from;
  uint8_t* row_action;
  int32_t* row_cost;
  int8_t* row_pos;        // [rows_cap][npad][2]
  uint32_t* dropped;
};

// thread g handles step g % plan_cap of item g / plan_cap
__global__ __launch_bounds__(256) void pw_push_batch_emit_kernel(PushBatchEmitArgs a) {
  const int64_t g = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  const int64_t i = g / a.plan_cap;
  const int32_t step = static_cast<int32_t>(g - i * a.plan_cap);
  if (i >= a.n) return;
  if (a.item_mask && a.item_mask[i] == 0) return;
  const int32_t item = push_batch_item(a.src, a.puzzle_id[i]);
  if (item < 0) return;  // another table's item
  const int32_t len = min(a.plan_len[i], a.plan_cap);
  if (step >= len) return;  // (len <= 0: no plan)
  const int64_t at = i * a.plan_cap + step, row = a.offset[i] + step;
  const int64_t state = a.plan_state[at];
  if (row < 0 || row >= a.rows_cap || state < 0 || state >= a.src.summary[static_cast<int64_t>(item) * 6]) {
    atomicAdd(a.dropped, 1u);  // (a state outside the item: not a plan of this table)
    return;
  }
  uint32_t w[16];
  if (step == 0 && a.pos) {
    const uint32_t* live = reinterpret_cast<const uint32_t*>(a.pos + i * a.npad * 2);
#pragma unroll
    for (int k = 0; k < 16; k++) w[k] = 2 * k < a.npad ? live[k] : 0u;
  } else {
    push_batch_key_words(a.src.pool_key[a.src.state_off[item] + state], w);
    if (step > 0) {
      // where the push before this one left the agent: a push move displaces its push set, the agent included, by one cell
      const uint32_t fxy = reinterpret_cast<const uint16_t*>(a.plan_from)[at - 1];
      const uint32_t act = a.plan_action[at - 1];
      const int dx = act == 0u ? -1 : (act == 1u ? 1 : 0), dy = act == 2u ? -1 : (act == 3u ? 1 : 0);
      const uint32_t x = static_cast<uint32_t>(static_cast<int>(static_cast<int8_t>(fxy & 0xffu)) + dx) & 0xffu;
      const uint32_t y = static_cast<uint32_t>(static_cast<int>(static_cast<int8_t>(fxy >> 8)) + dy) & 0xffu;
      w[0] = (w[0] & 0xffff0000u) | x | (y << 8);
    }
  }
  push_table_store_words(a.row_pos + row * a.npad * 2, a.npad, w);
  a.row_item[row] = static_cast<int32_t>(i);
  a.row_t[row] = step;
  a.row_state[row] = static_cast<int32_t>(state);
  reinterpret_cast<int16_t*>(a.row_from)[row] = reinterpret_cast<const int16_t*>(a.plan_from)[at];
  a.row_action[row] = a.plan_action[at];
  a.row_cost[row] = len - step;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
static PushBatchDrawSrc push_batch_draw_src(const PwPushSolveBatch* b) {
  PushBatchDrawSrc s{};
  s.hdrs = b->eng->set->d_headers;
  s.num_puzzles = b->eng->set->count;
  s.item_of_puzzle = b->d_item_of_puzzle;
  s.summary = b->d_summary;
  s.state_off = b->d_state_off;
  s.row_off = b->d_row_off;
  s.pool_key = b->d_key;
  s.pool_srow = b->d_srow;
  s.pool_cost = b->d_cost;
  s.pool_best = b->d_best;
  s.pool_succ = b->d_succ;
  s.pool_from = b->d_from;
  s.pool_action = b->d_action;
  s.pool_flags = b->d_flags;
  s.ix_off = b->index_valid ? b->d_ix_off : nullptr;
  s.cs_off = b->index_valid ? b->d_cs_off : nullptr;
  s.states_by_cost = b->index_valid ? b->d_states_by_cost : nullptr;
  s.cost_start = b->index_valid ? b->d_cost_start : nullptr;
  return s;
}

// what every draw needs of the handle: a run whose pools can hold a table
static int push_batch_draw_checks(const PwPushSolveBatch* b, const std::string& f) {
  if (b->n < 1) return pw_fail(PW_EINVAL, f + ": no run yet (call pw_push_solve_batch_run)");
  if (b->states_cap < 1 || b->rows_cap < 0 || !b->d_key)
    return pw_fail(PW_EINVAL, f + ": nothing stored (the handle was created with empty pools: summaries only)");
  return PW_OK;
}

extern "C" {

int pw_push_solve_batch_index(PwPushSolveBatch* b, void* stream) try {
  const std::string f("pw_push_solve_batch_index");
  if (!b) return pw_fail(PW_EINVAL, f + ": null handle");
  if (int rc = push_batch_draw_checks(b, f)) return rc;
  if (b->index_valid) return PW_OK;
  PwDeviceGuard guard(b->eng->set->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (int rc = push_solve_batch_host_copies(b, st, f.c_str())) return rc;  // (the synchronisation that sizes the arrays)
  const size_t n = static_cast<size_t>(b->n);
  b->h_ix_off.assign(n, -1);
  b->h_cs_off.assign(n, -1);
  int64_t total = 0, words = 0, max_states = 0;
  int32_t max_cost = -1;
  for (size_t it = 0; it < n; it++) {
    if (b->h_status[it] != PW_SB_BUILT || b->h_state_off[it] < 0 || b->h_row_off[it] < 0) continue;
    const int64_t S = b->h_summary[it * 6];
    const int32_t mc = b->h_summary[it * 6 + 4];
    if (S < 0 || mc < -1 || b->h_state_off[it] + S > b->states_cap) continue;  // (never: a stored item lies inside the pool)
    b->h_ix_off[it] = total;
    b->h_cs_off[it] = words;
    total += S;
    words += static_cast<int64_t>(mc) + 3;
    max_states = std::max(max_states, S);
    max_cost = std::max(max_cost, mc);
  }
  if (total < 1) return pw_fail(PW_EINVAL, f + ": nothing stored (no item of the last run has a stored table)");
  if (total >= (1ll << 31) || words >= (1ll << 31)) return pw_fail(PW_EINVAL, f + ": more than 2^31 - 1 states or buckets");
  push_solve_batch_index_discard(b);
  const size_t ns = static_cast<size_t>(total), cs_bytes = static_cast<size_t>(words) * 4;
  int word_bits = 1;
  while (static_cast<uint64_t>(words) >> word_bits) word_bits++;  // the bucket words are 0 .. words - 1
  const int key_bits = 8 * std::min(std::max(b->eng->set->max_n, 1), 8);  // movable j at bits 8 j: nothing above the set's N
  struct Release {
    void* p = nullptr;
    ~Release() {
      if (p) (void)hipFree(p);
    }
  } work;
  unsigned long long* none = nullptr;
  size_t sort1 = 0, sort2 = 0;
  hipError_t err = rocprim::radix_sort_pairs(nullptr, sort1, none, none, none, none, ns, 0, key_bits, st);
  if (err == hipSuccess) err = rocprim::radix_sort_keys(nullptr, sort2, none, none, ns, 32, 32 + word_bits, st);
  const size_t sort_bytes = std::max<size_t>(pw_pad256(std::max(sort1, sort2)), 256), col = pw_pad256(ns * 8);
  // the workspace: the keys, the sorted keys, the values, the sorted values and the sorts' own
  PwHipChain c(err);
  c.alloc(&work.p, 4 * col + sort_bytes);
  c.alloc(&b->d_states_by_cost, std::max<size_t>(ns * 4, 16));
  c.alloc(&b->d_cost_start, std::max<size_t>(cs_bytes, 16));
  c.alloc(&b->d_ix_off, std::max<size_t>(n * 8, 16));
  c.alloc(&b->d_cs_off, std::max<size_t>(n * 8, 16));
  c.then([&] { return hipMemsetAsync(b->d_cost_start, 0, cs_bytes, st); });
  c.then([&] { return hipMemcpyAsync(b->d_ix_off, b->h_ix_off.data(), n * 8, hipMemcpyHostToDevice, st); });
  c.then([&] { return hipMemcpyAsync(b->d_cs_off, b->h_cs_off.data(), n * 8, hipMemcpyHostToDevice, st); });
  if (!c.ok()) {
    push_solve_batch_index_discard(b);
    return pw_hip_fail(f, c.err);
  }
  uint8_t* base = static_cast<uint8_t*>(work.p);
  unsigned long long* key = reinterpret_cast<unsigned long long*>(base);
  unsigned long long* key_sorted = reinterpret_cast<unsigned long long*>(base + col);
  unsigned long long* val = reinterpret_cast<unsigned long long*>(base + 2 * col);
  unsigned long long* val_sorted = reinterpret_cast<unsigned long long*>(base + 3 * col);
  void* sort_tmp = base + 4 * col;
  PushBatchDrawSrc src = push_batch_draw_src(b);
  src.ix_off = b->d_ix_off;  // (not valid for the other entry points until the launches are queued)
  src.cs_off = b->d_cs_off;
  // an item's states over up to 64 workgroups -- one workgroup per item when there are many items
  int64_t chunks = std::min<int64_t>(64, std::max<int64_t>(1, (max_states + 1023) / 1024));
  while (chunks > 1 && static_cast<int64_t>(n) * chunks > (1ll << 30)) chunks /= 2;
  const dim3 block(256);
  hipLaunchKernelGGL(pw_push_batch_index_key_kernel, dim3(static_cast<unsigned>(static_cast<int64_t>(n) * chunks)), block, 0, st, src,
                     b->n, static_cast<uint32_t>(chunks), b->d_cost_start, key, val);
  // by key (stable), then by the bucket word (stable: ascending key inside a bucket); `key` is free for the second result
  err = rocprim::radix_sort_pairs(sort_tmp, sort1, key, key_sorted, val, val_sorted, ns, 0, key_bits, st);
  if (err == hipSuccess) err = rocprim::radix_sort_keys(sort_tmp, sort2, val_sorted, key, ns, 32, 32 + word_bits, st);
  if (err == hipSuccess) {
    hipLaunchKernelGGL(pw_push_batch_index_keep_kernel, dim3(static_cast<unsigned>((total + 255) / 256)), block, 0, st, key, total,
                       b->d_states_by_cost);
    hipLaunchKernelGGL(pw_push_batch_index_scan_kernel, dim3(static_cast<unsigned>(n)), block, 0, st, src, b->d_cost_start);
  }
  int rc = err == hipSuccess ? check_launch(f.c_str()) : pw_fail(PW_EDEVICE, f + ": radix sort: " + hipGetErrorString(err));
  // the workspace is freed when this returns: nothing in flight may read it
  if (hipStreamSynchronize(st) != hipSuccess && rc == PW_OK) rc = pw_fail(PW_EDEVICE, f + ": hipStreamSynchronize failed");
  if (rc != PW_OK) {
    push_solve_batch_index_discard(b);
    return rc;
  }
  b->index_valid = true;
  b->index_max_cost = max_cost;
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_push_solve_batch_index_read(PwPushSolveBatch* b, int32_t item, int32_t* states_by_cost, uint32_t* cost_start,
                                   void* stream) try {
  const std::string f("pw_push_solve_batch_index_read");
  if (!b) return pw_fail(PW_EINVAL, f + ": null handle");
  if (int rc = push_batch_draw_checks(b, f)) return rc;
  if (!b->index_valid) return pw_fail(PW_EINVAL, f + ": no index yet (call pw_push_solve_batch_index)");
  if (item < 0 || item >= b->n) return pw_fail(PW_EINVAL, f + ": item out of bounds");
  const size_t it = static_cast<size_t>(item);
  if (b->h_ix_off[it] < 0)
    return pw_fail(PW_EINVAL, f + ": the item has no stored table (status " + std::to_string(b->h_status[it]) + ")");
  PwDeviceGuard guard(b->eng->set->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t S = static_cast<size_t>(b->h_summary[it * 6]), words = static_cast<size_t>(b->h_summary[it * 6 + 4] + 3);
  hipError_t err = hipSuccess;
  if (states_by_cost && S)
    err = hipMemcpyAsync(states_by_cost, b->d_states_by_cost + b->h_ix_off[it], S * 4, hipMemcpyDeviceToDevice, st);
  if (err == hipSuccess && cost_start)
    err = hipMemcpyAsync(cost_start, b->d_cost_start + b->h_cs_off[it], words * 4, hipMemcpyDeviceToDevice, st);
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, f + ": " + hipGetErrorString(err));
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_push_solve_batch_sample(PwPushSolveBatch* b, const int32_t* puzzle_id, const uint8_t* mask, int32_t n, int32_t npad,
                               uint64_t seed, uint32_t* counter, int32_t lo, int32_t hi, const int32_t* lo_n, const int32_t* hi_n,
                               int8_t* pos, int32_t* steps, uint8_t* term, uint8_t* trunc, int32_t* out_state, int32_t* out_cost,
                               void* stream) try {
  const std::string f("pw_push_solve_batch_sample");
  if (!b) return pw_fail(PW_EINVAL, f + ": null handle");
  if (!puzzle_id) return pw_fail(PW_EINVAL, f + ": null puzzle_id");
  if (int rc = table_sample_checks(f.c_str(), n, npad, counter, lo, hi, lo_n, hi_n, pos, steps, out_state, out_cost, "out_state"))
    return rc;
  if (int rc = push_batch_draw_checks(b, f)) return rc;
  if (!b->index_valid) return pw_fail(PW_EINVAL, f + ": no index yet (call pw_push_solve_batch_index)");
  if (npad < b->eng->set->max_n) return pw_fail(PW_EINVAL, f + ": npad is smaller than the set's largest number of movables");
  PwDeviceGuard guard(b->eng->set->device);
  PushBatchSampleArgs a = {push_batch_draw_src(b), puzzle_id, mask, npad, n, seed, counter, lo, hi, lo_n, hi_n, pos, steps, term,
                           trunc, out_state, out_cost};
  const dim3 grid(static_cast<unsigned>((static_cast<int64_t>(n) + 255) / 256)), block(256);
  hipLaunchKernelGGL(pw_push_batch_sample_kernel, grid, block, 0, static_cast<hipStream_t>(stream), a);
  return check_launch(f.c_str());
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_push_solve_batch_plans(PwPushSolveBatch* b, const int32_t* index, const int32_t* puzzle_id, const uint8_t* mask, int32_t n,
                              int32_t tie, uint64_t seed, int8_t* plan_from, uint8_t* plan_action, int32_t* plan_state,
                              int32_t plan_cap, int32_t* plan_len, void* stream) try {
  const std::string f("pw_push_solve_batch_plans");
  if (!b) return pw_fail(PW_EINVAL, f + ": null handle");
  if (n < 1) return pw_fail(PW_EINVAL, f + ": n must be >= 1");
  if (!index) return pw_fail(PW_EINVAL, f + ": null index");
  if (!puzzle_id) return pw_fail(PW_EINVAL, f + ": null puzzle_id");
  if (!plan_from || !plan_action || !plan_len) return pw_fail(PW_EINVAL, f + ": null plan_from / plan_action / plan_len");
  if (plan_cap < 1) return pw_fail(PW_EINVAL, f + ": plan_cap must be >= 1");
  if (tie != 0 && tie != 1) return pw_fail(PW_EINVAL, f + ": tie must be 0 (lowest) or 1 (uniform)");
  if (int rc = push_batch_draw_checks(b, f)) return rc;
  PwDeviceGuard guard(b->eng->set->device);
  PushBatchPlansArgs a = {push_batch_draw_src(b), index, puzzle_id, mask, n, tie, plan_cap, seed, plan_from, plan_action,
                          plan_state, plan_len};
  const dim3 grid(static_cast<unsigned>((static_cast<int64_t>(n) + 255) / 256)), block(256);
  hipLaunchKernelGGL(pw_push_batch_plans_kernel, grid, block, 0, static_cast<hipStream_t>(stream), a);
  return check_launch(f.c_str());
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_push_solve_batch_emit(PwPushSolveBatch* b, const int32_t* puzzle_id, const uint8_t* mask, int32_t n, int32_t npad,
                             const int8_t* plan_from, const uint8_t* plan_action, const int32_t* plan_state, int32_t plan_cap,
                             const int32_t* plan_len, const int8_t* pos, const int64_t* offset, int64_t rows_cap,
                             int32_t* row_item, int32_t* row_t, int32_t* row_state, int8_t* row_from, uint8_t* row_action,
                             int32_t* row_cost, int8_t* row_pos, uint32_t* dropped, void* stream) try {
  const std::string f("pw_push_solve_batch_emit");
  if (!b) return pw_fail(PW_EINVAL, f + ": null handle");
  if (n < 1) return pw_fail(PW_EINVAL, f + ": n must be >= 1");
  if (!puzzle_id) return pw_fail(PW_EINVAL, f + ": null puzzle_id");
  if (!pw_npad_ok(npad)) return pw_fail(PW_EINVAL, f + ": npad must be 4, 8, 16 or 32");
  if (!plan_from || !plan_action || !plan_state || !plan_len)
    return pw_fail(PW_EINVAL, f + ": null plan_from / plan_action / plan_state / plan_len");
  if (plan_cap < 1) return pw_fail(PW_EINVAL, f + ": plan_cap must be >= 1");
  if (!offset) return pw_fail(PW_EINVAL, f + ": null offset");
  if (rows_cap < 0) return pw_fail(PW_EINVAL, f + ": rows_cap must be >= 0");
  if (rows_cap > 0 && (!row_item || !row_t || !row_state || !row_from || !row_action || !row_cost || !row_pos))
    return pw_fail(PW_EINVAL, f + ": null row output");  // (rows_cap 0: every row is dropped, the arrays are never written)
  if (!dropped) return pw_fail(PW_EINVAL, f + ": null dropped");
  if ((static_cast<int64_t>(n) * plan_cap + 255) / 256 > 0x7fffffffll)
    return pw_fail(PW_EINVAL, f + ": n * plan_cap is beyond one launch (split the items)");
  if (int rc = push_batch_draw_checks(b, f)) return rc;
  if (npad < b->eng->set->max_n) return pw_fail(PW_EINVAL, f + ": npad is smaller than the set's largest number of movables");
  PwDeviceGuard guard(b->eng->set->device);
  PushBatchEmitArgs a = {push_batch_draw_src(b), puzzle_id, mask, n, npad, plan_cap, plan_from, plan_action, plan_state, plan_len,
                         pos, offset, rows_cap, row_item, row_t, row_state, row_from, row_action, row_cost, row_pos, dropped};
  const int64_t threads = static_cast<int64_t>(n) * plan_cap;
  const dim3 grid(static_cast<unsigned>((threads + 255) / 256)), block(256);
  hipLaunchKernelGGL(pw_push_batch_emit_kernel, grid, block, 0, static_cast<hipStream_t>(stream), a);
  return check_launch(f.c_str());
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

}  // extern "C"

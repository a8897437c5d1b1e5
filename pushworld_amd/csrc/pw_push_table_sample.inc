// pw_push_table_sample.inc -- K20: drawing from the cost-to-go tables over pushes on the device (DESIGN.md K20).
// Part of the single translation unit pw_kernels.hip, included there after pw_push_table.inc (uses PwPushSearch, PushTableArgs,
// the scan kernel and the stream constants of pw_table_sample.inc, mix64 and rocprim's radix sort).
//
// K18 (pw_push_search_solve) leaves an exact table over the canonical states of a search over pushes in device memory.  This
// file makes it a data source, in K14's form:
//   cost index   the STATES grouped by cost-to-go: states_by_cost (a permutation of the store indices, cost 0 first, the dead
//                ends last, ascending store index inside a bucket) and cost_start -- a key per state and a histogram, one
//                stable radix sort of (bucket, store index), one scan;
//   sample       one thread per environment draws a state uniformly from a band of costs and writes it as a reset would;
//   plans        one thread per item walks best / the optimal rows and succ from a state down to cost 0;
//   emit         one thread per (item, step) writes one flat demonstration row: the push, the cost to go and the state the push
//                is made from, read off the store -- no flood and no step function.
// Every loop is bounded by the items, a state's rows, plan_cap or the start's cost.  No kernel waits on another workgroup, and
// there is no device assert.

struct PushTableDrawSrc {
  PushTableArgs t;
  const int8_t* pos;            // the store: [states][snpad][2] the states as reached
  const int32_t* states_by_cost;  // [states], or NULL: no index
  const uint32_t* cost_start;     // [max_cost + 3]
  int32_t snpad, n_mov, puzzle, max_cost;
};

// the bucket of a state: its cost, the dead ends after the largest finite cost
__device__ __forceinline__ uint32_t push_table_bucket(int32_t cost, int32_t max_cost) {
  return cost >= 0 && cost <= max_cost ? static_cast<uint32_t>(cost) : static_cast<uint32_t>(max_cost + 1);
}

// store state -> the engine's layout: 16 words of two movables each (x, y int8 pairs), zeros from movable n_mov on
__device__ __forceinline__ void push_table_state_words(const PushTableDrawSrc& s, int64_t state, uint32_t (&w)[16]) {
  const uint32_t* src = reinterpret_cast<const uint32_t*>(s.pos + state * s.snpad * 2);
  const int nw = s.snpad / 2;
#pragma unroll
  for (int k = 0; k < 16; k++) {
    uint32_t word = 0u;
    if (k < nw && 2 * k < s.n_mov) {
      word = src[k];
      if (2 * k + 1 >= s.n_mov) word &= 0xffffu;
    }
    w[k] = word;
  }
}

// 16 words -> npad pairs at dst, with 8-byte (npad 4) or 16-byte stores
__device__ __forceinline__ void push_table_store_words(int8_t* dst, int32_t npad, const uint32_t (&w)[16]) {
  if (npad == 4) {
    *reinterpret_cast<uint2*>(dst) = make_uint2(w[0], w[1]);
  } else {
#pragma unroll
    for (int q = 0; q < 4; q++)
      if (8 * q < npad) reinterpret_cast<uint4*>(dst)[q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
  }
}

// ---- cost index ---------------------------------------------------------------------------------------------------------------
// key[i] = the bucket of state i, val[i] = i, and word b + 1 of cost_start counts bucket b (b = 0 .. max_cost + 1): their
// inclusive scan over the max_cost + 3 words is cost_start itself.  The stable sort of (key, val) by key is states_by_cost.
__global__ __launch_bounds__(256) void pw_push_table_index_key_kernel(const int32_t* cost, int64_t states, int32_t max_cost,
                                                                       uint32_t* key, int32_t* val, uint32_t* cost_start) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= states) return;
  const uint32_t b = push_table_bucket(cost[i], max_cost);
  key[i] = b;
  val[i] = static_cast<int32_t>(i);
  atomicAdd(&cost_start[b + 1u], 1u);
}

// ---- sample: one start state per environment, drawn from a band of costs ---------------------------------------------------------
struct PushTableSampleArgs {
  PushTableDrawSrc src;
  const int32_t* puzzle_id;  // [n] or NULL
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

__global__ __launch_bounds__(256) void pw_push_table_sample_kernel(PushTableSampleArgs a) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= a.n) return;
  if (a.item_mask && a.item_mask[i] == 0) return;
  if (a.puzzle_id && a.puzzle_id[i] != a.src.puzzle) return;  // another table's environment: untouched
  const int32_t mc = a.src.max_cost;
  const int64_t S = a.src.t.states;
  const uint32_t finite = mc >= 0 ? a.src.cost_start[mc + 1] : 0u;  // states below the dead-end bucket
  if (finite == 0u) {  // nothing can be solved from any state of this table
    a.out_state[i] = -1;
    a.out_cost[i] = -1;
    return;
  }
  int32_t lo = a.lo_n ? a.lo_n[i] : a.lo, hi = a.hi_n ? a.hi_n[i] : a.hi;
  hi = max(hi, lo);
  lo = min(max(lo, 0), mc);
  hi = min(max(hi, 0), mc);
  const uint32_t first = a.src.cost_start[lo], end = a.src.cost_start[hi + 1];
  if (end <= first || end > S) {  // an empty band (a table without goal states in its store has no state of cost 0)
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
  const int64_t state = a.src.states_by_cost[first + u];
  if (state < 0 || state >= S) {  // (never, for an index built by this library)
    a.out_state[i] = -1;
    a.out_cost[i] = -1;
    return;
  }
  uint32_t w[16];
  push_table_state_words(a.src, state, w);
  push_table_store_words(a.pos + i * a.npad * 2, a.npad, w);
  a.steps[i] = 0;
  if (a.term) a.term[i] = 0;
  if (a.trunc) a.trunc[i] = 0;
  a.out_state[i] = static_cast<int32_t>(state);
  a.out_cost[i] = a.src.t.cost[state];
}

// ---- plans: a fewest-pushes plan from every given state --------------------------------------------------------------------------
struct PushTablePlansArgs {
  PushTableDrawSrc src;
  const int32_t* index;      // [n] store indices, as the query returns them
  const int32_t* puzzle_id;  // [n] or NULL
  const uint8_t* item_mask;  // [n] or NULL
  int32_t n, tie, plan_cap;
  uint64_t seed;
  int8_t* plan_from;         // [n][plan_cap][2]
  uint8_t* plan_action;      // [n][plan_cap]
  int32_t* plan_state;       // [n][plan_cap] or NULL
  int32_t* plan_len;         // [n]
};

__global__ __launch_bounds__(256) void pw_push_table_plans_kernel(PushTablePlansArgs a) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= a.n) return;
  if (a.item_mask && a.item_mask[i] == 0) return;
  const PushTableArgs& t = a.src.t;
  int64_t cur = a.index[i];
  if ((a.puzzle_id && a.puzzle_id[i] != a.src.puzzle) || cur < 0 || cur >= t.states) {
    a.plan_len[i] = -1;
    return;
  }
  const int32_t c = t.cost[cur];
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
    const int64_t r0 = t.row_off[cur], r1 = t.row_off[cur + 1];
    int64_t r = -1;
    if (a.tie) {
      uint32_t k = 0;
      for (int64_t q = r0; q < r1; q++) k += (t.flags[q] >> 1) & 1u;
      if (k > 0u) {
        const uint64_t h = mix64(a.seed ^ PW_TABLE_K_PLAN, static_cast<uint64_t>(i), static_cast<uint64_t>(step));
        uint32_t j = static_cast<uint32_t>(__umul64hi(h, static_cast<uint64_t>(k)));
        for (int64_t q = r0; q < r1 && r < 0; q++)
          if (t.flags[q] & 2) {
            if (j == 0u) r = q;
            j--;
          }
      }
    } else {
      const int32_t k = t.best[cur];
      if (k >= 0 && r0 + k < r1) r = r0 + k;
    }
    if (r < 0) break;  // (only at cost 0: never inside the loop)
    reinterpret_cast<int16_t*>(a.plan_from)[base + step] = reinterpret_cast<const int16_t*>(t.from)[r];
    a.plan_action[base + step] = t.action[r];
    if (a.plan_state) a.plan_state[base + step] = static_cast<int32_t>(cur);
    step++;
    if (t.flags[r] & 1) break;  // a goal row ends the plan, whatever its successor is
    const int32_t nxt = t.succ[r];
    if (nxt < 0 || nxt >= t.states) break;  // (an optimal row is safe: never)
    cur = nxt;
  }
  a.plan_len[i] = step;
}

// ---- emit: every push of every plan becomes one flat demonstration row -----------------------------------------------------------
struct PushTableEmitArgs {
  PushTableDrawSrc src;
  const int32_t* puzzle_id;  // [n] or NULL
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
__global__ __launch_bounds__(256) void pw_push_table_emit_kernel(PushTableEmitArgs a) {
  const int64_t g = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  const int64_t i = g / a.plan_cap;
  const int32_t step = static_cast<int32_t>(g - i * a.plan_cap);
  if (i >= a.n) return;
  if (a.item_mask && a.item_mask[i] == 0) return;
  if (a.puzzle_id && a.puzzle_id[i] != a.src.puzzle) return;
  const int32_t len = min(a.plan_len[i], a.plan_cap);
  if (step >= len) return;  // (len <= 0: no plan)
  const int64_t at = i * a.plan_cap + step, row = a.offset[i] + step;
  const int64_t state = a.plan_state[at];
  if (row < 0 || row >= a.rows_cap || state < 0 || state >= a.src.t.states) {  // (a state outside the store: not a plan of this table)
    atomicAdd(a.dropped, 1u);
    return;
  }
  uint32_t w[16];
  if (step == 0 && a.pos) {
    const uint32_t* live = reinterpret_cast<const uint32_t*>(a.pos + i * a.npad * 2);
#pragma unroll
    for (int k = 0; k < 16; k++) w[k] = 2 * k < a.npad ? live[k] : 0u;
  } else {
    push_table_state_words(a.src, state, w);
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
static PushTableDrawSrc push_table_draw_src(PwPushSearch* s) {
  PushTableDrawSrc d{};
  d.t = push_table_args(s);
  d.pos = s->d_pos;
  d.states_by_cost = s->t_index_valid ? s->d_t_states_by_cost : nullptr;
  d.cost_start = s->t_index_valid ? s->d_t_cost_start : nullptr;
  d.snpad = s->npad;
  d.n_mov = s->N;
  d.puzzle = s->puzzle;
  d.max_cost = static_cast<int32_t>(s->t_info[4]);
  return d;
}

extern "C" {

int pw_push_search_table_index(PwPushSearch* s, void* stream) try {
  const std::string f("pw_push_search_table_index");
  if (!s) return pw_fail(PW_EINVAL, f + ": null search");
  if (!s->t_solved) return pw_fail(PW_EINVAL, f + ": no table (call pw_push_search_solve after the search is exhausted)");
  if (s->t_index_valid) return PW_OK;
  PwDeviceGuard guard(s->eng->set->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t S = s->t_states;
  const int32_t mc = static_cast<int32_t>(s->t_info[4]);
  const size_t ns = static_cast<size_t>(S), words = static_cast<size_t>(mc + 3);
  int bits = 1;
  while ((static_cast<uint64_t>(mc) + 1ull) >> bits) bits++;  // the keys are 0 .. max_cost + 1
  struct Release {
    void* p = nullptr;
    ~Release() {
      if (p) (void)hipFree(p);
    }
  } work;
  uint32_t* none = nullptr;
  int32_t* nonev = nullptr;
  size_t sort_bytes = 0;
  hipError_t err = rocprim::radix_sort_pairs(nullptr, sort_bytes, none, none, nonev, nonev, ns, 0, bits, st);
  sort_bytes = std::max<size_t>(pw_pad256(sort_bytes), 256);
  // the workspace: the keys, the sorted keys, the values and the sort's own
  if (err == hipSuccess) err = hipMalloc(&work.p, 3 * pw_pad256(ns * 4) + sort_bytes);
  if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&s->d_t_states_by_cost), std::max<size_t>(ns * 4, 16));
  if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&s->d_t_cost_start), std::max<size_t>(words * 4, 16));
  if (err == hipSuccess) err = hipMemsetAsync(s->d_t_cost_start, 0, words * 4, st);
  if (err != hipSuccess) {
    push_table_index_discard(s);
    return pw_hip_fail(f, err);
  }
  uint8_t* base = static_cast<uint8_t*>(work.p);
  uint32_t* key = reinterpret_cast<uint32_t*>(base);
  uint32_t* key_sorted = reinterpret_cast<uint32_t*>(base + pw_pad256(ns * 4));
  int32_t* val = reinterpret_cast<int32_t*>(base + 2 * pw_pad256(ns * 4));
  void* sort_tmp = base + 3 * pw_pad256(ns * 4);
  const dim3 grid(static_cast<unsigned>((S + 255) / 256)), block(256);
  hipLaunchKernelGGL(pw_push_table_index_key_kernel, grid, block, 0, st, s->d_t_cost, S, mc, key, val, s->d_t_cost_start);
  err = rocprim::radix_sort_pairs(sort_tmp, sort_bytes, key, key_sorted, val, s->d_t_states_by_cost, ns, 0, bits, st);
  TableSrc scan{};  // the scan of pw_table_sample.inc over this table's max_cost + 3 words
  scan.cost_start = s->d_t_cost_start;
  scan.max_cost = mc;
  if (err == hipSuccess) hipLaunchKernelGGL(pw_table_index_scan_kernel<false>, dim3(1), block, 0, st, scan);
  int rc = err == hipSuccess ? check_launch(f.c_str()) : pw_fail(PW_EDEVICE, f + ": radix sort: " + hipGetErrorString(err));
  // the workspace is freed when this returns: nothing in flight may read it
  if (hipStreamSynchronize(st) != hipSuccess && rc == PW_OK) rc = pw_fail(PW_EDEVICE, f + ": hipStreamSynchronize failed");
  if (rc != PW_OK) {
    push_table_index_discard(s);
    return rc;
  }
  s->t_index_valid = true;
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_push_search_table_index_read(PwPushSearch* s, int32_t* states_by_cost, uint32_t* cost_start, void* stream) try {
  const std::string f("pw_push_search_table_index_read");
  if (!s) return pw_fail(PW_EINVAL, f + ": null search");
  if (!s->t_solved) return pw_fail(PW_EINVAL, f + ": no table (call pw_push_search_solve after the search is exhausted)");
  if (!s->t_index_valid) return pw_fail(PW_EINVAL, f + ": no index yet (call pw_push_search_table_index)");
  PwDeviceGuard guard(s->eng->set->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t err = hipSuccess;
  if (states_by_cost && s->t_states > 0)
    err = hipMemcpyAsync(states_by_cost, s->d_t_states_by_cost, static_cast<size_t>(s->t_states) * 4, hipMemcpyDeviceToDevice, st);
  if (err == hipSuccess && cost_start)
    err = hipMemcpyAsync(cost_start, s->d_t_cost_start, static_cast<size_t>(s->t_info[4] + 3) * 4, hipMemcpyDeviceToDevice, st);
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, f + ": " + hipGetErrorString(err));
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_push_search_table_sample(PwPushSearch* s, const int32_t* puzzle_id, const uint8_t* mask, int32_t n, int32_t npad,
                                uint64_t seed, uint32_t* counter, int32_t lo, int32_t hi, const int32_t* lo_n, const int32_t* hi_n,
                                int8_t* pos, int32_t* steps, uint8_t* term, uint8_t* trunc, int32_t* out_state, int32_t* out_cost,
                                void* stream) try {
  if (!s) return pw_fail(PW_EINVAL, "pw_push_search_table_sample: null search");
  if (int rc = table_sample_checks("pw_push_search_table_sample", n, npad, counter, lo, hi, lo_n, hi_n, pos, steps, out_state,
                                   out_cost, "out_state"))
    return rc;
  if (npad < s->N) return pw_fail(PW_EINVAL, "pw_push_search_table_sample: npad is smaller than the puzzle's number of movables");
  if (!s->t_solved)
    return pw_fail(PW_EINVAL, "pw_push_search_table_sample: no table (call pw_push_search_solve after the search is exhausted)");
  if (!s->t_index_valid) return pw_fail(PW_EINVAL, "pw_push_search_table_sample: no index yet (call pw_push_search_table_index)");
  PwDeviceGuard guard(s->eng->set->device);
  PushTableSampleArgs a = {push_table_draw_src(s), puzzle_id, mask, npad, n, seed, counter, lo, hi, lo_n, hi_n, pos, steps, term,
                           trunc, out_state, out_cost};
  const dim3 grid(static_cast<unsigned>((static_cast<int64_t>(n) + 255) / 256)), block(256);
  hipLaunchKernelGGL(pw_push_table_sample_kernel, grid, block, 0, static_cast<hipStream_t>(stream), a);
  return check_launch("pw_push_search_table_sample");
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_push_search_table_plans(PwPushSearch* s, const int32_t* index, const int32_t* puzzle_id, const uint8_t* mask, int32_t n,
                               int32_t tie, uint64_t seed, int8_t* plan_from, uint8_t* plan_action, int32_t* plan_state,
                               int32_t plan_cap, int32_t* plan_len, void* stream) try {
  const std::string f("pw_push_search_table_plans");
  if (!s) return pw_fail(PW_EINVAL, f + ": null search");
  if (n < 1) return pw_fail(PW_EINVAL, f + ": n must be >= 1");
  if (!index) return pw_fail(PW_EINVAL, f + ": null index");
  if (!plan_from || !plan_action || !plan_len) return pw_fail(PW_EINVAL, f + ": null plan_from / plan_action / plan_len");
  if (plan_cap < 1) return pw_fail(PW_EINVAL, f + ": plan_cap must be >= 1");
  if (tie != 0 && tie != 1) return pw_fail(PW_EINVAL, f + ": tie must be 0 (lowest) or 1 (uniform)");
  if (!s->t_solved) return pw_fail(PW_EINVAL, f + ": no table (call pw_push_search_solve after the search is exhausted)");
  PwDeviceGuard guard(s->eng->set->device);
  PushTablePlansArgs a = {push_table_draw_src(s), index, puzzle_id, mask, n, tie, plan_cap, seed, plan_from, plan_action,
                          plan_state, plan_len};
  const dim3 grid(static_cast<unsigned>((static_cast<int64_t>(n) + 255) / 256)), block(256);
  hipLaunchKernelGGL(pw_push_table_plans_kernel, grid, block, 0, static_cast<hipStream_t>(stream), a);
  return check_launch(f.c_str());
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_push_search_table_emit(PwPushSearch* s, const int32_t* puzzle_id, const uint8_t* mask, int32_t n, int32_t npad,
                              const int8_t* plan_from, const uint8_t* plan_action, const int32_t* plan_state, int32_t plan_cap,
                              const int32_t* plan_len, const int8_t* pos, const int64_t* offset, int64_t rows_cap,
                              int32_t* row_item, int32_t* row_t, int32_t* row_state, int8_t* row_from, uint8_t* row_action,
                              int32_t* row_cost, int8_t* row_pos, uint32_t* dropped, void* stream) try {
  const std::string f("pw_push_search_table_emit");
  if (!s) return pw_fail(PW_EINVAL, f + ": null search");
  if (n < 1) return pw_fail(PW_EINVAL, f + ": n must be >= 1");
  if (int rc = pw_check_npad(f + ": ", npad)) return rc;
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
  if (npad < s->N) return pw_fail(PW_EINVAL, f + ": npad is smaller than the puzzle's number of movables");
  if (!s->t_solved) return pw_fail(PW_EINVAL, f + ": no table (call pw_push_search_solve after the search is exhausted)");
  PwDeviceGuard guard(s->eng->set->device);
  PushTableEmitArgs a = {push_table_draw_src(s), puzzle_id, mask, n, npad, plan_cap, plan_from, plan_action, plan_state, plan_len,
                         pos, offset, rows_cap, row_item, row_t, row_state, row_from, row_action, row_cost, row_pos, dropped};
  const int64_t threads = static_cast<int64_t>(n) * plan_cap;
  const dim3 grid(static_cast<unsigned>((threads + 255) / 256)), block(256);
  hipLaunchKernelGGL(pw_push_table_emit_kernel, grid, block, 0, static_cast<hipStream_t>(stream), a);
  return check_launch(f.c_str());
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

}  // extern "C"

// pw_push_batch_sample.inc -- K26: drawing from the BATCHED cost-to-go tables over pushes on the device (DESIGN.md K26).
// Part of the single translation unit pw_kernels.hip, included there after pw_push_draw.inc and pw_push_solution_batch.inc (uses
// PwPushSolveBatch and its pools, the draw kernels, their checks and push_table_bucket of pw_push_draw.inc, the scan kernel and
// the sample checks of pw_table_sample.inc and rocprim's radix sort).
//
// K22 (pw_push_solve_batch_run) leaves the tables of many small puzzles in two pools.  This file makes them a data source, in the
// form K20 gave the one-puzzle table and K14 gave the move-level batch:
//   cost index   per stored item the STATES grouped by cost-to-go: states_by_cost (a permutation of the item's state numbers,
//                cost 0 first, the dead ends last, ASCENDING 64-BIT KEY inside a bucket) and cost_start.  K22's state numbers
//                inside a layer are the schedule's, the key -- the packed canonical state -- is not: position p of a bucket
//                holds the same STATE in every run.  One key kernel ((bucket word of the item) << 32 | state number per state,
//                and the histogram), a stable radix sort by key, a stable radix sort by the bucket word, one kernel that
//                keeps the state numbers, one scan per item;
//   sample, plans, emit   ONE launch each for a mixed batch: the kernels of pw_push_draw.inc with kBatch = true, the table
//                resolved per environment through item_of_puzzle, its states decoded from the keys.
// A node's key IS its canonical state, so the unpacked key (zeros beyond the puzzle's N: pw_sb_keep) is the state.
// No kernel waits on another workgroup, there is no device assert, and every store is a plain or vector store.

// ---- cost index ---------------------------------------------------------------------------------------------------------------
// Workgroup g works on item g / chunks, states (g % chunks) * 256 + tid, + chunks * 256, ...  State r of an item whose index
// starts at ix and whose cost_start starts at word cs: key[ix + r] = its 64-bit key, val[ix + r] = (cs + bucket) << 32 | r, and
// word cs + bucket + 1 counts the bucket.  (cs + bucket ascends with (item, bucket): the second sort groups by both at once.)
__global__ __launch_bounds__(256) void pw_push_batch_index_key_kernel(PushDrawSrc s, int32_t items, uint32_t chunks,
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
    const uint32_t b = push_table_bucket(s.cost[base + r], mc);
    key[ix + r] = s.key[base + r];
    val[ix + r] = (static_cast<unsigned long long>(cs + b) << 32) | static_cast<unsigned long long>(r);
    atomicAdd(&cost_start[cs + b + 1u], 1u);
  }
}

__global__ __launch_bounds__(256) void pw_push_batch_index_keep_kernel(const unsigned long long* val, int64_t total,
                                                                        int32_t* states_by_cost) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i < total) states_by_cost[i] = static_cast<int32_t>(static_cast<uint32_t>(val[i]));
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
static PushDrawSrc push_batch_draw_src(const PwPushSolveBatch* b) {
  PushDrawSrc s{};
  s.cost = b->d_cost;
  s.best = b->d_best;
  s.srow = b->d_srow;
  s.succ = b->d_succ;
  s.from = b->d_from;
  s.action = b->d_action;
  s.flags = b->d_flags;
  s.states_by_cost = b->index_valid ? b->d_states_by_cost : nullptr;
  s.cost_start = b->index_valid ? b->d_cost_start : nullptr;
  s.item_of_puzzle = b->d_item_of_puzzle;
  s.summary = b->d_summary;
  s.state_off = b->d_state_off;
  s.row_off = b->d_row_off;
  s.ix_off = b->index_valid ? b->d_ix_off : nullptr;
  s.cs_off = b->index_valid ? b->d_cs_off : nullptr;
  s.key = b->d_key;
  s.num_puzzles = b->eng->set->count;
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
  PushDrawSrc src = push_batch_draw_src(b);
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
    hipLaunchKernelGGL(pw_table_index_scan_kernel, dim3(static_cast<unsigned>(n)), block, 0, st, b->d_cost_start, b->d_cs_off,
                       b->d_summary + 4, 6, 0);
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
  PushSampleArgs a = {push_batch_draw_src(b), puzzle_id, mask, npad, n, seed, counter, lo, hi, lo_n, hi_n, pos, steps, term, trunc,
                      out_state, out_cost};
  return push_draw_launch(pw_push_sample_kernel<true>, n, a, stream, f);
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_push_solve_batch_plans(PwPushSolveBatch* b, const int32_t* index, const int32_t* puzzle_id, const uint8_t* mask, int32_t n,
                              int32_t tie, uint64_t seed, int8_t* plan_from, uint8_t* plan_action, int32_t* plan_state,
                              int32_t plan_cap, int32_t* plan_len, void* stream) try {
  const std::string f("pw_push_solve_batch_plans");
  if (!b) return pw_fail(PW_EINVAL, f + ": null handle");
  if (int rc = push_plans_checks(f, n, index, puzzle_id, true, tie, plan_from, plan_action, plan_cap, plan_len)) return rc;
  if (int rc = push_batch_draw_checks(b, f)) return rc;
  PwDeviceGuard guard(b->eng->set->device);
  PushPlansArgs a = {push_batch_draw_src(b), index, puzzle_id, mask, n, tie, plan_cap, seed, plan_from, plan_action, plan_state,
                     plan_len};
  return push_draw_launch(pw_push_plans_kernel<true>, n, a, stream, f);
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
  PushEmitArgs a = {PushDrawSrc{}, puzzle_id, mask, n, npad, plan_cap, plan_from, plan_action, plan_state, plan_len, pos, offset,
                    rows_cap, row_item, row_t, row_state, row_from, row_action, row_cost, row_pos, dropped};
  if (int rc = push_emit_checks(f, a, true)) return rc;
  if (int rc = push_batch_draw_checks(b, f)) return rc;
  if (npad < b->eng->set->max_n) return pw_fail(PW_EINVAL, f + ": npad is smaller than the set's largest number of movables");
  PwDeviceGuard guard(b->eng->set->device);
  a.src = push_batch_draw_src(b);
  return push_draw_launch(pw_push_emit_kernel<true>, static_cast<int64_t>(n) * plan_cap, a, stream, f);
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

}  // extern "C"

// pw_push_table_sample.inc -- K20: drawing from the cost-to-go tables over pushes on the device (DESIGN.md K20).
// Part of the single translation unit pw_kernels.hip, included there after pw_push_table.inc and pw_push_draw.inc (uses
// PwPushSearch, the draw kernels, their checks and push_table_bucket of pw_push_draw.inc, the scan kernel and the sample checks of
// pw_table_sample.inc and rocprim's radix sort).
//
// K18 (pw_push_search_solve) leaves an exact table over the canonical states of a search over pushes in device memory.  This
// file makes it a data source, in K14's form:
//   cost index   the STATES grouped by cost-to-go: states_by_cost (a permutation of the store indices, cost 0 first, the dead
//                ends last, ascending store index inside a bucket) and cost_start -- a key per state and a histogram, one
//                stable radix sort of (bucket, store index), one scan;
//   sample, plans, emit   the kernels of pw_push_draw.inc with kBatch = false: the one table, its states decoded from the store.
// No kernel waits on another workgroup, and there is no device assert.

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

// ---- host ------------------------------------------------------------------------------------------------------------------------
static PushDrawSrc push_table_draw_src(const PwPushSearch* s) {
  PushDrawSrc d{};
  d.cost = s->d_t_cost;
  d.best = s->d_t_best;
  d.srow = s->d_t_row_off;
  d.succ = s->d_t_succ;
  d.from = reinterpret_cast<const uint16_t*>(s->d_t_from);
  d.action = s->d_t_action;
  d.flags = s->d_t_flags;
  d.states_by_cost = s->t_index_valid ? s->d_t_states_by_cost : nullptr;
  d.cost_start = s->t_index_valid ? s->d_t_cost_start : nullptr;
  d.pos = s->d_pos;
  d.states = s->t_states;
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
  if (err == hipSuccess)
    hipLaunchKernelGGL(pw_table_index_scan_kernel, dim3(1), block, 0, st, s->d_t_cost_start, nullptr, nullptr, 0, mc);
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
  PushSampleArgs a = {push_table_draw_src(s), puzzle_id, mask, npad, n, seed, counter, lo, hi, lo_n, hi_n, pos, steps, term, trunc,
                      out_state, out_cost};
  return push_draw_launch(pw_push_sample_kernel<false>, n, a, stream, "pw_push_search_table_sample");
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_push_search_table_plans(PwPushSearch* s, const int32_t* index, const int32_t* puzzle_id, const uint8_t* mask, int32_t n,
                               int32_t tie, uint64_t seed, int8_t* plan_from, uint8_t* plan_action, int32_t* plan_state,
                               int32_t plan_cap, int32_t* plan_len, void* stream) try {
  const std::string f("pw_push_search_table_plans");
  if (!s) return pw_fail(PW_EINVAL, f + ": null search");
  if (int rc = push_plans_checks(f, n, index, puzzle_id, false, tie, plan_from, plan_action, plan_cap, plan_len)) return rc;
  if (!s->t_solved) return pw_fail(PW_EINVAL, f + ": no table (call pw_push_search_solve after the search is exhausted)");
  PwDeviceGuard guard(s->eng->set->device);
  PushPlansArgs a = {push_table_draw_src(s), index, puzzle_id, mask, n, tie, plan_cap, seed, plan_from, plan_action, plan_state,
                     plan_len};
  return push_draw_launch(pw_push_plans_kernel<false>, n, a, stream, f);
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
  PushEmitArgs a = {PushDrawSrc{}, puzzle_id, mask, n, npad, plan_cap, plan_from, plan_action, plan_state, plan_len, pos, offset,
                    rows_cap, row_item, row_t, row_state, row_from, row_action, row_cost, row_pos, dropped};
  if (int rc = push_emit_checks(f, a, false)) return rc;
  if (npad < s->N) return pw_fail(PW_EINVAL, f + ": npad is smaller than the puzzle's number of movables");
  if (!s->t_solved) return pw_fail(PW_EINVAL, f + ": no table (call pw_push_search_solve after the search is exhausted)");
  PwDeviceGuard guard(s->eng->set->device);
  a.src = push_table_draw_src(s);
  return push_draw_launch(pw_push_emit_kernel<false>, static_cast<int64_t>(n) * plan_cap, a, stream, f);
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

}  // extern "C"

// pw_push_table.inc -- K18: exact cost-to-go tables over the canonical states of an exhausted search over pushes.
// Part of the single translation unit pw_kernels.hip (included there after pw_push_search.inc: the table sits on a PwPushSearch,
// its successor pass is the front half of that search's pass, its query floods through pw_walk_kernel).
//
// Definitions (include/pushworld_amd.h): state i has npush[i] push rows in pw_walk_pushes' order; succ[r] is the store index of
// the row's successor, -1 outside the grid; the value c(r) of a row is 0 for a goal row, else cost[succ[r]], else infinite; cost[i]
// is 0 at a goal state, else 1 + min c(r), -1 where that is infinite; best[i] is the lowest row of the least value.
//
//   successor pass   per `chunk` parents over the whole store: counts, scan, the rows flood, the regions flood of the
//                    successors and the candidates (push_search_front), then a READ-ONLY lookup of every candidate in the
//                    closed set.  The table of the closed set is never written.
//   sweeps           level-synchronous: sweep d, one lane per row, lowers best[state] to the lowest row of value d - 1
//                    (atomicMin) of every state still unset; then one lane per state gives those states cost d.  A sweep after
//                    one that changed nothing changes nothing, so PW_PT_GROUP sweeps are queued per host read.
//   bits             one lane per row: optimal and safe; one lane per state: the counts.
//   query            effective mask, one regions flood of the live states, one lane per item: the lookup of the successor pass
//                    on the live state's packed canonical state, then the walk back along the live map's parent actions.
//
// Every loop is bounded by the rows, the slots of the table, the states or 4 095 steps of a walk.  No kernel waits on another
// workgroup, and there is no device assert.

#define PW_PT_GROUP 8        // sweeps queued per read of the changed-counters
#define PW_PT_UNSET 0x7FFFFFFF  // best[] while the sweeps run
// counters
#define PW_PT_C_MISSING 0
#define PW_PT_C_GOALS 1
#define PW_PT_C_DEAD 2
#define PW_PT_C_CHANGED 4  // .. + PW_PT_GROUP
#define PW_PT_C_WORDS 16

struct PushTableArgs {
  int64_t states, rows;
  int64_t* row_off;
  int32_t* cost;
  int32_t* best;
  int32_t* succ;
  int8_t* from;
  uint8_t* action;
  uint8_t* flags;
  int32_t* row_state;  // [rows] the sweeps' workspace: the state a row belongs to
  uint32_t* counters;
};

// The closed set's entry for a packed canonical state (`word(k)`, fingerprint fp, first slot `slot`): the store index, -1 when
// an empty slot ends the probe (the state is not in the set), -2 when every slot was probed.  Read-only.
template <class Word>
__device__ __forceinline__ int64_t push_table_lookup(const PushSearchArgs& a, uint32_t slot, uint32_t fp, Word word) {
  for (uint64_t step = 0; step < a.slots; step++, slot = (slot + 1u) & a.mask) {
    const unsigned long long v = a.table[slot];
    if (v == 0ull) return -1;
    const uint32_t low = static_cast<uint32_t>(v);
    if (static_cast<uint32_t>(v >> 32) != fp || (low & PW_PS_TENT) != 0u) continue;  // (an exhausted search leaves no tentative entry)
    const int64_t idx = static_cast<int64_t>(low) - 1;
    bool eq = true;
    for (int k = 0; k < a.nw; k++) eq = eq && word(k) == push_search_store_word(a, idx, k);
    if (eq) return idx;
  }
  return -2;
}

__global__ __launch_bounds__(256) void pw_push_table_counts_kernel(const int32_t* npush, int64_t states, int64_t* row_off) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i <= states) row_off[i] = i < states ? npush[i] : 0;  // the scan's last input: row_off[states] becomes the total
}

// ---- the successor pass's last kernel: row r of the pass is row row_off[parent] + k of the table ------------------------------
__global__ __launch_bounds__(256) void pw_push_table_lookup_kernel(PushSearchArgs a, PushTableArgs t) {
  const int64_t r = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (r >= a.rows) return;
  const int32_t item = a.row_item[r];
  const bool listed = item >= 0 && item < a.parents;
  const int64_t parent = a.first + (listed ? item : 0);
  const int64_t dst = t.row_off[parent] + (r - a.f_offset[listed ? item : 0]);
  if (!listed || dst < t.row_off[parent] || dst >= t.row_off[parent + 1]) {  // (the floods list what the store counted: never)
    atomicAdd(&t.counters[PW_PT_C_MISSING], 1u);
    return;
  }
  int64_t idx = -1;
  if (a.s_size[r] > 0) {
    const uint32_t* my = a.cand_state + r * a.nw;
    idx = push_table_lookup(a, a.cand_hash[r], a.cand_fp[r], [&](int k) { return my[k]; });
    if (idx < 0 || idx >= t.states) {  // inside its grid and not closed: the search was not exhausted
      atomicAdd(&t.counters[PW_PT_C_MISSING], 1u);
      idx = -1;
    }
  }
  t.succ[dst] = static_cast<int32_t>(idx);
  reinterpret_cast<int16_t*>(t.from)[dst] = reinterpret_cast<const int16_t*>(a.row_from)[r];
  t.action[dst] = a.row_action[r];
  t.flags[dst] = a.row_goal[r] ? 1 : 0;
  t.row_state[dst] = static_cast<int32_t>(parent);
}

// ---- sweeps --------------------------------------------------------------------------------------------------------------
// the value of a row: 0 for a goal row, the successor's cost, -1 = infinite (a dead, an unset or no successor)
__device__ __forceinline__ int32_t push_table_value(const PushTableArgs& t, int64_t r) {
  if (t.flags[r] & 1) return 0;
  const int32_t s = t.succ[r];
  return s >= 0 ? t.cost[s] : -1;
}

__global__ __launch_bounds__(256) void pw_push_table_init_kernel(PushTableArgs t, const uint8_t* goal) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= t.states) return;
  t.cost[i] = goal[i] ? 0 : -1;
  t.best[i] = PW_PT_UNSET;
}

__global__ __launch_bounds__(256) void pw_push_table_sweep_rows_kernel(PushTableArgs t, int32_t d) {
  const int64_t r = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (r >= t.rows) return;
  const int32_t i = t.row_state[r];
  if (i < 0 || t.cost[i] != -1) return;  // (i < 0: a row no pass wrote -- pw_push_table_bits_kernel reports it)
  if (push_table_value(t, r) == d - 1) atomicMin(&t.best[i], static_cast<int32_t>(r - t.row_off[i]));
}

__global__ __launch_bounds__(256) void pw_push_table_sweep_states_kernel(PushTableArgs t, int32_t d, int32_t slot) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  const bool set = i < t.states && t.cost[i] == -1 && t.best[i] != PW_PT_UNSET;
  if (set) t.cost[i] = d;
  const unsigned long long m = __ballot(set);
  if (m != 0ull && (threadIdx.x & 63) == __ffsll(m) - 1) atomicAdd(&t.counters[PW_PT_C_CHANGED + slot], static_cast<uint32_t>(__popcll(m)));
}

// ---- the row bits and the counts --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pw_push_table_bits_kernel(PushTableArgs t) {
  const int64_t r = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (r >= t.rows) return;
  const int32_t i = t.row_state[r];
  if (i < 0) {
    atomicAdd(&t.counters[PW_PT_C_MISSING], 1u);
    return;
  }
  const int32_t c = push_table_value(t, r), mine = t.cost[i];
  uint8_t f = t.flags[r] & 1;
  if (c >= 0) f |= 4;
  if (c >= 0 && mine > 0 && c == mine - 1) f |= 2;
  t.flags[r] = f;
}

__global__ __launch_bounds__(256) void pw_push_table_finish_kernel(PushTableArgs t) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  const bool in = i < t.states;
  if (in && t.best[i] == PW_PT_UNSET) t.best[i] = -1;
  const int32_t c = in ? t.cost[i] : 1;
  const unsigned long long goals = __ballot(c == 0), dead = __ballot(c == -1);
  if ((threadIdx.x & 63) == 0) {
    if (goals) atomicAdd(&t.counters[PW_PT_C_GOALS], static_cast<uint32_t>(__popcll(goals)));
    if (dead) atomicAdd(&t.counters[PW_PT_C_DEAD], static_cast<uint32_t>(__popcll(dead)));
  }
}

// ---- the query ---------------------------------------------------------------------------------------------------------------
struct PushQueryArgs {
  const int32_t* puzzle_id;
  const int8_t* pos;
  const uint8_t* mask;
  int32_t n, npad, puzzle, n_mov;
  int32_t* ids;   // [n] the table's puzzle
  uint8_t* eff;   // [n] mask && id == puzzle
  const int32_t* size;
  const int8_t* canon;
  const uint16_t* maps;  // or NULL
  int32_t map_h, map_w;
  int32_t* index;
  int32_t* cost;
  int8_t* push_from;
  uint8_t* push_action;
  int32_t* walk;
  int8_t* action;
};

__global__ __launch_bounds__(256) void pw_push_table_mask_kernel(PushQueryArgs q) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= q.n) return;
  q.ids[i] = q.puzzle;
  q.eff[i] = ((!q.mask || q.mask[i] != 0) && (!q.puzzle_id || q.puzzle_id[i] == q.puzzle)) ? 1 : 0;
}

__global__ __launch_bounds__(256) void pw_push_table_query_kernel(PushSearchArgs a, PushTableArgs t, PushQueryArgs q) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= q.n || q.eff[i] == 0) return;  // items of other puzzles and masked items are left untouched
  int64_t idx = -1;
  if (q.size[i] > 0) {  // (-1: a movable outside its grid)
    const uint16_t* src = reinterpret_cast<const uint16_t*>(q.pos) + i * q.npad;
    const uint32_t cxy = reinterpret_cast<const uint16_t*>(q.canon)[i];
    // word k of the live state's packed canonical state: the agent's pair replaced by canon, nothing past the movables
    auto word = [&](int k) -> uint32_t {
      const uint32_t lo = k == 0 ? cxy : src[2 * k];
      const uint32_t hi = 2 * k + 1 < q.n_mov ? src[2 * k + 1] : 0u;
      return lo | (hi << 16);
    };
    unsigned long long h = PW_PS_HASH_SEED;
    for (int k = 0; k < a.nw; k++) h = push_search_hash_word(h, word(k));
    h = push_search_hash_end(h);
    idx = push_table_lookup(a, static_cast<uint32_t>(h) & a.mask, push_search_fp(h, a.fp_bits), word);
    if (idx < 0 || idx >= t.states) idx = -1;
  }
  int32_t cost = -2, walk = -1, act = -1, fxy = 0;
  uint32_t pact = 0xFFu;
  if (idx >= 0) {
    cost = t.cost[idx];
    const int32_t k = t.best[idx];
    if (k >= 0) {
      const int64_t r = t.row_off[idx] + k;
      fxy = reinterpret_cast<const uint16_t*>(t.from)[r];
      pact = t.action[r];
      if (q.maps) {
        // dist(from) in the LIVE state's map, then back along the parent actions to the position at distance 1
        const uint16_t* m = q.maps + i * q.map_h * q.map_w;
        int x = fxy & 0xff, y = (fxy >> 8) & 0xff;
        auto entry = [&](int ex, int ey) -> uint32_t {
          return (ex >= 0 && ey >= 0 && ex < q.map_w && ey < q.map_h) ? m[ey * q.map_w + ex] : 0xFFFFu;
        };
        uint32_t e = entry(x, y);
        if (e != 0xFFFFu) {
          walk = static_cast<int32_t>(e & 0xFFFu);
          for (int step = 0; step < 4095 && e != 0xFFFFu && (e & 0xFFFu) > 1u; step++) {
            const int dir = e >> 12;
            x -= dir == 0 ? -1 : (dir == 1 ? 1 : 0);
            y -= dir == 2 ? -1 : (dir == 3 ? 1 : 0);
            e = entry(x, y);
          }
          if (walk == 0) act = static_cast<int32_t>(pact);
          else if (e != 0xFFFFu && (e & 0xFFFu) == 1u) act = static_cast<int32_t>(e >> 12);
        }
      }
    }
  }
  if (q.index) q.index[i] = static_cast<int32_t>(idx);
  if (q.cost) q.cost[i] = cost;
  if (q.push_from) reinterpret_cast<int16_t*>(q.push_from)[i] = static_cast<int16_t>(fxy);
  if (q.push_action) q.push_action[i] = static_cast<uint8_t>(pact);
  if (q.walk) q.walk[i] = walk;
  if (q.action) q.action[i] = static_cast<int8_t>(act);
}

// the cost index over the table (pw_push_table_sample.inc)
static void push_table_index_discard(PwPushSearch* s) {
  if (s->d_t_states_by_cost) (void)hipFree(s->d_t_states_by_cost);
  if (s->d_t_cost_start) (void)hipFree(s->d_t_cost_start);
  s->d_t_states_by_cost = nullptr;
  s->d_t_cost_start = nullptr;
  s->t_index_valid = false;
}

static void push_table_discard(PwPushSearch* s) {
  push_table_index_discard(s);
  void* bufs[] = {s->d_t_row_off, s->d_t_cost, s->d_t_best, s->d_t_succ, s->d_t_from, s->d_t_action, s->d_t_flags};
  for (void* b : bufs)
    if (b) (void)hipFree(b);
  s->d_t_row_off = nullptr;
  s->d_t_cost = s->d_t_best = s->d_t_succ = nullptr;
  s->d_t_from = nullptr;
  s->d_t_action = s->d_t_flags = nullptr;
  s->t_solved = false;
  s->t_states = s->t_rows = 0;
}

static PushTableArgs push_table_args(PwPushSearch* s) {
  PushTableArgs t{};
  t.states = s->t_states;
  t.rows = s->t_rows;
  t.row_off = s->d_t_row_off;
  t.cost = s->d_t_cost;
  t.best = s->d_t_best;
  t.succ = s->d_t_succ;
  t.from = s->d_t_from;
  t.action = s->d_t_action;
  t.flags = s->d_t_flags;
  return t;
}

extern "C" {

int pw_push_search_solve(PwPushSearch* s, int64_t info_out[5], void* stream) try {
  if (!s) return pw_fail(PW_EINVAL, "pw_push_search_solve: null search");
  if (!info_out) return pw_fail(PW_EINVAL, "pw_push_search_solve: null info");
  if (!s->begun) return pw_fail(PW_EINVAL, "pw_push_search_solve: pw_push_search_begin has not been called");
  if (s->stop_at_goal) return pw_fail(PW_EINVAL, "pw_push_search_solve: the search stops at its goal (begin it with stop_at_goal = 0)");
  if (s->overflow) return pw_fail(PW_EINVAL, "pw_push_search_solve: the state store overflowed (max_states): the space is incomplete");
  if (s->depth < 1 || s->layer_end != s->layer_begin)
    return pw_fail(PW_EINVAL, "pw_push_search_solve: the search is not exhausted (layers are left to expand)");
  PwDeviceGuard guard(s->eng->set->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  push_table_discard(s);
  const int64_t S = s->layer_end;
  struct Release {
    void* p = nullptr;
    ~Release() {
      if (p) (void)hipFree(p);
    }
  } scan_mem, work_mem;
  auto fail = [&](int code, const std::string& msg) {
    (void)hipStreamSynchronize(st);  // nothing in flight reads what is freed
    push_table_discard(s);
    return pw_fail(code, msg);
  };
  auto device_fail = [&](hipError_t e) {
    return fail(pw_hip_code(e), std::string("pw_push_search_solve: ") + hipGetErrorString(e));
  };
  // ---- the row offsets: the scan of the store's push counts --------------------------------------------------------------------
  const size_t ns = static_cast<size_t>(S);
  size_t scan_bytes = 0;
  hipError_t err = rocprim::exclusive_scan(nullptr, scan_bytes, s->d_t_row_off, s->d_t_row_off, static_cast<int64_t>(0), ns + 1,
                                           rocprim::plus<int64_t>(), st);
  scan_bytes = std::max<size_t>(pw_pad256(scan_bytes), 256);
  if (err == hipSuccess) err = hipMalloc(&scan_mem.p, scan_bytes);
  if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&s->d_t_row_off), (ns + 1) * 8);
  if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&s->d_t_cost), ns * 4);
  if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&s->d_t_best), ns * 4);
  if (err != hipSuccess) return device_fail(err);
  const dim3 sgrid(static_cast<unsigned>((S + 1 + 255) / 256)), block(256);
  hipLaunchKernelGGL(pw_push_table_counts_kernel, sgrid, block, 0, st, s->d_npush, S, s->d_t_row_off);
  err = rocprim::exclusive_scan(scan_mem.p, scan_bytes, s->d_t_row_off, s->d_t_row_off, static_cast<int64_t>(0), ns + 1,
                                rocprim::plus<int64_t>(), st);
  int64_t R = 0;
  if (err == hipSuccess) err = hipMemcpyAsync(&R, s->d_t_row_off + S, 8, hipMemcpyDeviceToHost, st);
  if (err == hipSuccess) err = hipStreamSynchronize(st);
  if (err != hipSuccess) return device_fail(err);
  if (R > (1ll << 31) - 1) return fail(PW_ELIMIT, "pw_push_search_solve: more than 2^31 - 1 push rows");
  const size_t nr = static_cast<size_t>(std::max<int64_t>(R, 1));
  if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&s->d_t_succ), nr * 4);
  if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&s->d_t_from), nr * 2);
  if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&s->d_t_action), nr);
  if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&s->d_t_flags), nr);
  // the sweeps' workspace: the row -> state map and the counters
  if (err == hipSuccess) err = hipMalloc(&work_mem.p, nr * 4 + PW_PT_C_WORDS * 4);
  if (err != hipSuccess) return device_fail(err);
  s->t_states = S;
  s->t_rows = R;
  PushTableArgs t = push_table_args(s);
  t.row_state = static_cast<int32_t*>(work_mem.p);
  t.counters = reinterpret_cast<uint32_t*>(t.row_state + nr);
  err = hipMemsetAsync(t.counters, 0, PW_PT_C_WORDS * 4, st);
  if (err == hipSuccess) err = hipMemsetAsync(t.row_state, 0xff, nr * 4, st);  // -1: a row no pass has written
  if (err != hipSuccess) return device_fail(err);
  // ---- the successor pass: one pass per `chunk` parents over the whole store -------------------------------------------------------
  unsigned long long pinfo[PW_PS_I_WORDS] = {0};
  for (int64_t off = 0; off < S; off += s->chunk) {
    PushSearchArgs a = push_search_args(s);
    a.first = off;
    a.parents = static_cast<int32_t>(std::min<int64_t>(s->chunk, S - off));
    const dim3 pgrid(static_cast<unsigned>((a.parents + 255) / 256));
    hipLaunchKernelGGL(pw_push_search_counts_kernel, pgrid, block, 0, st, a);
    size_t tmp = s->f_scan_bytes;
    err = rocprim::exclusive_scan(s->d_f_scan, tmp, s->d_f_offset, s->d_f_offset, static_cast<int64_t>(0),
                                  static_cast<size_t>(a.parents) + 1, rocprim::plus<int64_t>(), st);
    if (err != hipSuccess) return device_fail(err);
    hipLaunchKernelGGL(pw_push_search_stat_kernel, pgrid, block, 0, st, a);
    // the pass's one wait: its row count
    err = hipMemcpyAsync(pinfo, s->d_info, sizeof(pinfo), hipMemcpyDeviceToHost, st);
    if (err == hipSuccess) err = hipStreamSynchronize(st);
    if (err != hipSuccess) return device_fail(err);
    const int64_t T = static_cast<int64_t>(pinfo[PW_PS_I_ROWS]);
    if (T == 0) continue;
    if (T > R) return fail(PW_EDEVICE, "pw_push_search_solve: a pass lists more rows than the store counted (an internal error)");
    if (int rc = push_search_reserve_rows(s, T, st, "pw_push_search_solve")) {
      push_table_discard(s);
      return rc;
    }
    a = push_search_args(s);  // (the row buffers may have moved)
    a.first = off;
    a.parents = static_cast<int32_t>(std::min<int64_t>(s->chunk, S - off));
    a.rows = static_cast<int32_t>(T);
    push_search_front(s, a, s->d_pos + off * s->npad * 2, st);
    hipLaunchKernelGGL(pw_push_table_lookup_kernel, dim3(static_cast<unsigned>((T + 255) / 256)), block, 0, st, a, t);
  }
  // ---- the sweeps ---------------------------------------------------------------------------------------------------------------
  const dim3 tgrid(static_cast<unsigned>((S + 255) / 256)), rgrid(static_cast<unsigned>((R + 255) / 256));
  hipLaunchKernelGGL(pw_push_table_init_kernel, tgrid, block, 0, st, t, s->d_goal);
  uint32_t counters[PW_PT_C_WORDS] = {0};
  int64_t largest = -1, d = 1;
  bool more = R > 0;
  while (more && d <= S) {
    const int group = static_cast<int>(std::min<int64_t>(PW_PT_GROUP, S - d + 1));
    err = hipMemsetAsync(t.counters + PW_PT_C_CHANGED, 0, PW_PT_GROUP * 4, st);
    if (err != hipSuccess) return device_fail(err);
    for (int g = 0; g < group; g++) {
      hipLaunchKernelGGL(pw_push_table_sweep_rows_kernel, rgrid, block, 0, st, t, static_cast<int32_t>(d + g));
      hipLaunchKernelGGL(pw_push_table_sweep_states_kernel, tgrid, block, 0, st, t, static_cast<int32_t>(d + g), g);
    }
    err = hipMemcpyAsync(counters, t.counters, sizeof(counters), hipMemcpyDeviceToHost, st);
    if (err == hipSuccess) err = hipStreamSynchronize(st);
    if (err != hipSuccess) return device_fail(err);
    for (int g = 0; g < group && more; g++) {
      if (counters[PW_PT_C_CHANGED + g] == 0u) more = false;
      else largest = d + g;
    }
    d += group;
  }
  if (R > 0) hipLaunchKernelGGL(pw_push_table_bits_kernel, rgrid, block, 0, st, t);
  hipLaunchKernelGGL(pw_push_table_finish_kernel, tgrid, block, 0, st, t);
  if (int rc = check_launch("pw_push_search_solve")) {
    (void)hipStreamSynchronize(st);
    push_table_discard(s);
    return rc;
  }
  err = hipMemcpyAsync(counters, t.counters, sizeof(counters), hipMemcpyDeviceToHost, st);
  if (err == hipSuccess) err = hipStreamSynchronize(st);
  if (err != hipSuccess) return device_fail(err);
  if (counters[PW_PT_C_MISSING] != 0u)
    return fail(PW_EDEVICE, "pw_push_search_solve: " + std::to_string(counters[PW_PT_C_MISSING]) +
                                " successors are missing from the closed set of an exhausted search (an internal error)");
  if (largest < 0 && counters[PW_PT_C_GOALS] != 0u) largest = 0;
  s->t_info[0] = S;
  s->t_info[1] = R;
  s->t_info[2] = counters[PW_PT_C_GOALS];
  s->t_info[3] = counters[PW_PT_C_DEAD];
  s->t_info[4] = largest;
  for (int k = 0; k < 5; k++) info_out[k] = s->t_info[k];
  s->t_solved = true;
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_push_search_table_read(PwPushSearch* s, int64_t first, int64_t count, int64_t* row_off, int32_t* cost, int32_t* best,
                              void* stream) try {
  if (!s) return pw_fail(PW_EINVAL, "pw_push_search_table_read: null search");
  if (first < 0 || count < 0) return pw_fail(PW_EINVAL, "pw_push_search_table_read: state range out of bounds");
  if (!s->t_solved) return pw_fail(PW_EINVAL, "pw_push_search_table_read: no table (call pw_push_search_solve after the search is exhausted)");
  if (first + count > s->t_states) return pw_fail(PW_EINVAL, "pw_push_search_table_read: state range out of bounds");
  PwDeviceGuard guard(s->eng->set->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t n = static_cast<size_t>(count);
  hipError_t err = hipSuccess;
  if (row_off) err = hipMemcpyAsync(row_off, s->d_t_row_off + first, (n + 1) * 8, hipMemcpyDeviceToDevice, st);
  if (err == hipSuccess && n && cost) err = hipMemcpyAsync(cost, s->d_t_cost + first, n * 4, hipMemcpyDeviceToDevice, st);
  if (err == hipSuccess && n && best) err = hipMemcpyAsync(best, s->d_t_best + first, n * 4, hipMemcpyDeviceToDevice, st);
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string("pw_push_search_table_read: ") + hipGetErrorString(err));
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_push_search_table_rows(PwPushSearch* s, int64_t first, int64_t count, int32_t* succ, int8_t* from, uint8_t* action,
                              uint8_t* flags, void* stream) try {
  if (!s) return pw_fail(PW_EINVAL, "pw_push_search_table_rows: null search");
  if (first < 0 || count < 0) return pw_fail(PW_EINVAL, "pw_push_search_table_rows: row range out of bounds");
  if (!s->t_solved) return pw_fail(PW_EINVAL, "pw_push_search_table_rows: no table (call pw_push_search_solve after the search is exhausted)");
  if (first + count > s->t_rows) return pw_fail(PW_EINVAL, "pw_push_search_table_rows: row range out of bounds");
  if (count == 0) return PW_OK;
  PwDeviceGuard guard(s->eng->set->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t n = static_cast<size_t>(count);
  hipError_t err = hipSuccess;
  auto copy = [&](void* dst, const void* src, size_t bytes) {
    if (err == hipSuccess && dst) err = hipMemcpyAsync(dst, src, n * bytes, hipMemcpyDeviceToDevice, st);
  };
  copy(succ, s->d_t_succ + first, 4);
  copy(from, s->d_t_from + first * 2, 2);
  copy(action, s->d_t_action + first, 1);
  copy(flags, s->d_t_flags + first, 1);
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string("pw_push_search_table_rows: ") + hipGetErrorString(err));
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_push_search_table_query(PwPushSearch* s, const int32_t* puzzle_id, const int8_t* pos, int32_t npad, const uint8_t* mask,
                               int32_t n, int32_t* index, int32_t* cost, int8_t* push_from, uint8_t* push_action, int32_t* walk,
                               int8_t* action, void* stream) try {
  if (!s) return pw_fail(PW_EINVAL, "pw_push_search_table_query: null search");
  if (n < 1) return pw_fail(PW_EINVAL, "pw_push_search_table_query: n must be >= 1");
  if (!pos) return pw_fail(PW_EINVAL, "pw_push_search_table_query: null pos");
  if (int rc = pw_check_npad("pw_push_search_table_query: ", npad)) return rc;
  if (npad < s->eng->set->max_n)
    return pw_fail(PW_EINVAL, "pw_push_search_table_query: npad is smaller than the set's largest number of movables");
  if (!s->t_solved) return pw_fail(PW_EINVAL, "pw_push_search_table_query: no table (call pw_push_search_solve after the search is exhausted)");
  PwDeviceGuard guard(s->eng->set->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool maps = walk != nullptr || action != nullptr;
  const int map_h = std::min(std::max(s->eng->set->max_h, 1), PW_MAX_DIM), map_w = std::min(std::max(s->eng->set->max_w, 1), PW_MAX_DIM);
  const size_t cells = static_cast<size_t>(map_h) * map_w;
  if (n > s->q_cap || (maps && !s->q_maps)) {  // first use or growth: the one synchronisation of the query
    const size_t cap = static_cast<size_t>(std::max(n, s->q_cap));
    const bool with_maps = maps || s->q_maps;
    hipError_t err = hipStreamSynchronize(st);
    if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string("pw_push_search_table_query: ") + hipGetErrorString(err));
    if (s->d_q_mem) (void)hipFree(s->d_q_mem);
    s->d_q_mem = nullptr;
    s->q_cap = 0;
    s->q_maps = false;
    const size_t bytes = pw_pad256(cap * 4) + pw_pad256(cap) + pw_pad256(cap * 4) + pw_pad256(cap * 2) + pw_pad256((cap + 1) * 8) +
                         (with_maps ? pw_pad256(cap * cells * 2) : 0);
    err = hipMalloc(reinterpret_cast<void**>(&s->d_q_mem), bytes);
    if (err != hipSuccess) return pw_hip_fail("pw_push_search_table_query", err);
    s->q_cap = static_cast<int32_t>(cap);
    s->q_maps = with_maps;
  }
  const size_t cap = static_cast<size_t>(s->q_cap);
  uint8_t* base = s->d_q_mem;
  int32_t* d_ids = reinterpret_cast<int32_t*>(base);
  uint8_t* d_eff = base + pw_pad256(cap * 4);
  int32_t* d_size = reinterpret_cast<int32_t*>(d_eff + pw_pad256(cap));
  int8_t* d_canon = reinterpret_cast<int8_t*>(d_size) + pw_pad256(cap * 4);
  int64_t* d_offset = reinterpret_cast<int64_t*>(d_canon + pw_pad256(cap * 2));
  uint16_t* d_maps = maps ? reinterpret_cast<uint16_t*>(reinterpret_cast<uint8_t*>(d_offset) + pw_pad256((cap + 1) * 8)) : nullptr;
  PushQueryArgs q{};
  q.puzzle_id = puzzle_id;
  q.pos = pos;
  q.mask = mask;
  q.n = n;
  q.npad = npad;
  q.puzzle = s->puzzle;
  q.n_mov = s->N;
  q.ids = d_ids;
  q.eff = d_eff;
  q.size = d_size;
  q.canon = d_canon;
  q.maps = d_maps;
  q.map_h = map_h;
  q.map_w = map_w;
  q.index = index;
  q.cost = cost;
  q.push_from = push_from;
  q.push_action = push_action;
  q.walk = walk;
  q.action = action;
  const dim3 grid(static_cast<unsigned>((static_cast<int64_t>(n) + 255) / 256)), block(256);
  hipLaunchKernelGGL(pw_push_table_mask_kernel, grid, block, 0, st, q);
  // every entry of every map: 0xFFFF, the flood overwrites the positions of the regions
  if (d_maps && hipMemsetAsync(d_maps, 0xff, static_cast<size_t>(n) * cells * 2, st) != hipSuccess)
    return pw_fail(PW_EDEVICE, "pw_push_search_table_query: hipMemsetAsync failed");
  WalkArgs w{};
  w.puzzle_id = d_ids;
  w.pos = pos;
  w.mask = d_eff;
  w.n = n;
  w.npad = npad;
  w.emit = 0;
  w.region_size = d_size;
  w.canon = d_canon;
  w.offset = d_offset;
  w.walk_map = d_maps;
  w.map_h = map_h;
  w.map_w = map_w;
  w.next_item = s->d_counter;
  walk_launch(s->eng, w, st);
  hipLaunchKernelGGL(pw_push_table_query_kernel, grid, block, 0, st, push_search_args(s), push_table_args(s), q);
  return check_launch("pw_push_search_table_query");
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

}  // extern "C"

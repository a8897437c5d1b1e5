// pw_solution.inc -- exact cost-to-go tables over an exhausted breadth-first search (DESIGN.md K12).
// Included from pw_kernels.hip after pw_search.inc (uses its PwSearch, SearchArgs, expand kernels and hash functions).
//
// pw_search_* leaves the whole reachable space of a puzzle in the store, numbered in FIFO order, with the closed set that maps a
// state to its number.  It only ever looks forwards.  pw_search_solve adds the backward half, one row per state:
//   succ   the store index of the successor under each of the four actions.  The search's own expand kernels run again over the
//          store, in passes of <= chunk parents into the candidate scratch, and pw_solve_succ_kernel looks every candidate up in
//          the closed set (read only: the bucket walk of the claim kernel without its claims).  A fingerprinted entry carries
//          the index and is verified against the stored words; an exact-key entry is the state itself, so pw_solve_index_kernel
//          first records which state sits in which slot (d_slot_index).  The expand kernels drop the step back to the parent
//          ("the way back"): that successor is the tree parent.
//   cost   level-synchronous sweeps: sweep k settles every unsettled state with a successor of cost k - 1.  A sweep leaves the
//          number it settled in a device word of its own and returns at once when the sweep before it settled nothing, so the
//          host enqueues 16 sweeps at a time and reads their words back once per 16.
//   acts   optimal and safe action bits, from succ and cost.
// pw_search_table_query maps live environment states (the engine's int8 layout) to their rows in one capturable launch.

#define PW_SOLVE_INF 0xFFFFu
#define PW_SOLVE_SWEEPS 65536      // counts[k] = states settled by sweep k (k = 0: the goal states)
#define PW_SOLVE_MISSING 65536     // counts[]: successors / stored states that the closed set does not hold (a bug)
#define PW_SOLVE_DEAD 65537        // counts[]: dead ends
#define PW_SOLVE_WORDS 65540
#define PW_SOLVE_BATCH 16          // sweeps enqueued per readback

// the slot hash of a packed state, as the expand kernels sum it: one term per slot of the lane group (gs of them, the empty
// ones included)
__device__ __forceinline__ uint32_t search_state_hash(const uint32_t* w, int n, int gs) {
  uint32_t t = 0;
  for (int lj = 0; lj < gs; lj++) {
    const uint32_t xy = lj < n ? ((w[lj >> 1] >> (16 * (lj & 1))) & 0xffffu) : 0u;
    t += search_lane_term(xy, static_cast<uint32_t>(lj));
  }
  return search_final(t);
}

// Store index of the state `my` (nw words) in the closed set of an exhausted search, -1 when it is not there.  Read only: the
// bucket walk of pw_search_claim_kernel (an insertion takes the first empty slot on this path, and entries never leave).
template <bool kKey>
__device__ __forceinline__ int64_t search_lookup(const unsigned long long* table, uint32_t mask, uint32_t h, const uint32_t* my,
                                                 int nw, int n, int bx, int by, const uint32_t* states,
                                                 const uint32_t* slot_index) {
  const uint32_t fp = kKey ? 0u : search_fingerprint(my, nw);
  const unsigned long long key = kKey ? search_key(my, n, bx, by) : 0ull;
  uint32_t bucket = h & ~7u;
  for (uint64_t walked = 0; walked <= mask; walked += 8) {
    unsigned long long e[8];
    {
      const uint4* line = reinterpret_cast<const uint4*>(table + bucket);
      const uint4 v0 = line[0], v1 = line[1], v2 = line[2], v3 = line[3];
      e[0] = v0.x | (static_cast<unsigned long long>(v0.y) << 32), e[1] = v0.z | (static_cast<unsigned long long>(v0.w) << 32);
      e[2] = v1.x | (static_cast<unsigned long long>(v1.y) << 32), e[3] = v1.z | (static_cast<unsigned long long>(v1.w) << 32);
      e[4] = v2.x | (static_cast<unsigned long long>(v2.y) << 32), e[5] = v2.z | (static_cast<unsigned long long>(v2.w) << 32);
      e[6] = v3.x | (static_cast<unsigned long long>(v3.y) << 32), e[7] = v3.z | (static_cast<unsigned long long>(v3.w) << 32);
    }
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const unsigned long long v = e[i];
      if (v == 0ull) return -1;
      if (kKey) {
        if (v == key) return static_cast<int64_t>(slot_index[bucket + static_cast<uint32_t>(i)]);
      } else if (static_cast<uint32_t>(v >> 32) == fp && !(static_cast<uint32_t>(v) & PW_S_TENT)) {
        const int64_t idx = static_cast<int64_t>(static_cast<uint32_t>(v)) - 1;
        const uint32_t* other = states + idx * nw;  // the fingerprints agree: the full compare keeps the lookup exact
        bool eq = true;
        for (int k = 0; k < nw; k++) eq = eq && my[k] == other[k];
        if (eq) return idx;
      }
    }
    bucket = (bucket + 8u) & mask;
  }
  return -1;
}

// ---- exact keys: which state sits in which slot -----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pw_solve_index_kernel(SearchArgs a, int n, int gs, int64_t total, uint32_t* slot_index,
                                                             uint32_t* counts) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= total) return;
  const uint32_t* my = a.states + i * a.nw;
  const unsigned long long key = search_key(my, n, a.key_bx, a.key_by);
  uint32_t slot = (search_state_hash(my, n, gs) & a.mask) & ~7u;
  for (uint64_t walked = 0; walked <= a.mask; walked++) {
    const unsigned long long v = a.table[slot];
    if (v == key) {
      slot_index[slot] = static_cast<uint32_t>(i);
      return;
    }
    if (v == 0ull) break;
    slot = (slot + 1u) & a.mask;
  }
  atomicAdd(&counts[PW_SOLVE_MISSING], 1u);
}

// ---- successor indices: one thread per candidate of an expand pass ----------------------------------------------------------
template <bool kKey>
__global__ __launch_bounds__(256) void pw_solve_succ_kernel(SearchArgs a, int n, const uint32_t* slot_index, int32_t* succ,
                                                            uint32_t* counts) {
  const int64_t c = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (c >= a.ncand) return;
  const int64_t pidx = a.first + (c >> 2);
  const uint32_t act = static_cast<uint32_t>(c & 3);
  const uint32_t h = a.cand_hash[c];
  int64_t out = pidx;  // nothing moved
  if (h == PW_S_NONE) {
    // the way back (pw_search_expand_kernel): the agent alone steps back to where the tree parent had it
    const uint32_t came = a.action[pidx];
    if ((came & 0x84u) == 4u && (came & 3u) == (act ^ 1u) && (a.cand_goal[c] & 2u)) out = a.parent[pidx];
  } else {
    out = search_lookup<kKey>(a.table, a.mask, h, a.cand_state + c * a.nw, a.nw, n, a.key_bx, a.key_by, a.states, slot_index);
    if (out < 0) {  // not in an exhausted closed set: counted, reported by pw_search_solve
      atomicAdd(&counts[PW_SOLVE_MISSING], 1u);
      out = pidx;
    }
  }
  succ[pidx * 4 + act] = static_cast<int32_t>(out);
}

// ---- backward propagation -----------------------------------------------------------------------------------------------------
// cost 0 at every goal state (movable j = 1 .. G on goal j - 1; without goals every state is one), "none yet" elsewhere
__global__ __launch_bounds__(256) void pw_solve_init_kernel(SearchArgs a, int64_t total, uint16_t* cost, uint32_t* counts) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  bool goal = false;
  if (i < total) {
    const PwPuzzleHeader* h = a.hdrs + a.puzzle;
    const uint16_t* row = reinterpret_cast<const uint16_t*>(a.states + i * a.nw);
    const uint16_t* g = reinterpret_cast<const uint16_t*>(h->goal);
    goal = true;
    for (int j = 1; j <= h->G; j++) goal = goal && row[j] == g[j - 1];
    cost[i] = goal ? 0 : PW_SOLVE_INF;
  }
  const unsigned long long m = __ballot(goal);
  if ((threadIdx.x & (PW_WAVE - 1)) == 0 && m) atomicAdd(&counts[0], static_cast<uint32_t>(__popcll(m)));
}

// Sweep k: an unsettled state with a successor of cost k - 1 gets cost k.  (A cost written by this sweep is k, never k - 1, so
// reading it while others write is harmless.)  k = 65535 only counts: the value it writes is the "none" mark itself.
__global__ __launch_bounds__(256) void pw_solve_sweep_kernel(const int32_t* succ, uint16_t* cost, int64_t total, uint32_t k,
                                                             uint32_t* counts) {
  if (counts[k - 1] == 0u) return;  // the sweep before settled nothing: neither does this one
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  bool settle = false;
  if (i < total && cost[i] == PW_SOLVE_INF) {
    const int4 s = reinterpret_cast<const int4*>(succ)[i];
    const uint32_t want = k - 1u;
    settle = cost[s.x] == want || cost[s.y] == want || cost[s.z] == want || cost[s.w] == want;
    if (settle) cost[i] = static_cast<uint16_t>(k);
  }
  const unsigned long long m = __ballot(settle);
  if ((threadIdx.x & (PW_WAVE - 1)) == 0 && m) atomicAdd(&counts[k], static_cast<uint32_t>(__popcll(m)));
}

// bit a: action a is optimal (moves, and its successor is one step nearer); bit 4 + a: safe (its successor can still be solved)
__global__ __launch_bounds__(256) void pw_solve_acts_kernel(const int32_t* succ, const uint16_t* cost, int64_t total,
                                                            uint8_t* acts, uint32_t* counts) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  bool dead = false;
  if (i < total) {
    const uint32_t c = cost[i];
    const int4 s = reinterpret_cast<const int4*>(succ)[i];
    const int32_t t[4] = {s.x, s.y, s.z, s.w};
    uint32_t bits = 0;
#pragma unroll
    for (int act = 0; act < 4; act++) {
      const uint32_t ct = cost[t[act]];
      if (ct != PW_SOLVE_INF) bits |= 16u << act;
      if (c != 0u && c != PW_SOLVE_INF && t[act] != i && ct + 1u == c) bits |= 1u << act;
    }
    acts[i] = static_cast<uint8_t>(bits);
    dead = c == PW_SOLVE_INF;
  }
  const unsigned long long m = __ballot(dead);
  if ((threadIdx.x & (PW_WAVE - 1)) == 0 && m) atomicAdd(&counts[PW_SOLVE_DEAD], static_cast<uint32_t>(__popcll(m)));
}

// ---- query: live states -> table rows ------------------------------------------------------------------------------------------
struct TableQueryArgs {
  const unsigned long long* table;
  const uint32_t* states;
  const uint32_t* slot_index;
  const uint16_t* cost;
  const uint8_t* acts;
  uint32_t mask;
  int32_t puzzle, n_mov, nw, gs, bx, by, W, H;
  const int32_t* puzzle_id;  // or NULL: every item is the table's puzzle
  const int8_t* pos;         // [n][npad][2]
  const uint8_t* item_mask;  // or NULL
  int32_t npad, n;
  int32_t* out_index;
  int32_t* out_cost;
  uint8_t* out_acts;
};

template <bool kKey>
__global__ __launch_bounds__(256) void pw_table_query_kernel(TableQueryArgs a) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= a.n) return;
  if (a.puzzle_id && a.puzzle_id[i] != a.puzzle) return;  // another table's item: untouched
  if (a.item_mask && a.item_mask[i] == 0) return;
  const int8_t* row = a.pos + i * a.npad * 2;
  uint32_t w[PW_MAX_OBJECTS / 2];
  bool inside = true;
  uint32_t t = 0;
#pragma unroll
  for (int k = 0; k < PW_MAX_OBJECTS / 2; k++) {
    uint32_t word = 0;
    if (k < a.nw) {
#pragma unroll
      for (int half = 0; half < 2; half++) {
        const int j = 2 * k + half;
        if (j < a.n_mov) {
          const int x = row[2 * j], y = row[2 * j + 1];
          inside = inside && x >= 0 && x < a.W && y >= 0 && y < a.H;
          const uint32_t xy = static_cast<uint32_t>(x & 0xff) | (static_cast<uint32_t>(y & 0xff) << 8);
          word |= xy << (16 * half);
          t += search_lane_term(xy, static_cast<uint32_t>(j));
        }
      }
    }
    w[k] = word;
  }
  for (int j = a.n_mov; j < a.gs; j++) t += search_lane_term(0u, static_cast<uint32_t>(j));
  int64_t idx = -1;
  if (inside)
    idx = search_lookup<kKey>(a.table, a.mask, search_final(t) & a.mask, w, a.nw, a.n_mov, a.bx, a.by, a.states, a.slot_index);
  if (a.out_index) a.out_index[i] = static_cast<int32_t>(idx);
  if (a.out_cost) {
    const uint32_t c = idx >= 0 ? a.cost[idx] : 0u;
    a.out_cost[i] = idx < 0 ? -2 : (c == PW_SOLVE_INF ? -1 : static_cast<int32_t>(c));
  }
  if (a.out_acts) a.out_acts[i] = idx >= 0 ? a.acts[idx] : static_cast<uint8_t>(0);
}

// four points on the stream; a point that could not be recorded makes its intervals read -1
struct SolveEvents {
  hipEvent_t e[4];
  bool ok[4];
  SolveEvents() {
    for (int k = 0; k < 4; k++) ok[k] = hipEventCreate(&e[k]) == hipSuccess;
  }
  ~SolveEvents() {
    for (int k = 0; k < 4; k++)
      if (ok[k]) (void)hipEventDestroy(e[k]);
  }
  void record(int k, hipStream_t st) { ok[k] = ok[k] && hipEventRecord(e[k], st) == hipSuccess; }
  float elapsed(int k) {  // milliseconds from point k to point k + 1 (after the stream was synchronised)
    float ms = -1.0f;
    if (!ok[k] || !ok[k + 1] || hipEventElapsedTime(&ms, e[k], e[k + 1]) != hipSuccess) return -1.0f;
    return ms;
  }
};

extern "C" {

int pw_search_solve(PwSearch* s, int64_t info[4], void* stream) try {
  if (!s) return pw_fail(PW_EINVAL, "pw_search_solve: null search");
  if (!info) return pw_fail(PW_EINVAL, "pw_search_solve: null info");
  if (!s->begun) return pw_fail(PW_EINVAL, "pw_search_solve: pw_search_begin has not been called");
  if (s->width != 0) return pw_fail(PW_EINVAL, "pw_search_solve: needs a breadth-first search (novelty_width 0)");
  if (s->overflow) return pw_fail(PW_EINVAL, "pw_search_solve: the state store overflowed (max_states): the space is incomplete");
  if (!s->exhausted)
    return pw_fail(PW_EINVAL, "pw_search_solve: the search is not exhausted (expand until a layer has no new states)");
  PwDeviceGuard guard(s->eng->set->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  search_table_discard(s);
  const int64_t total = s->layer_end;
  PwHipChain c(guard.status());
  c.alloc(&s->d_succ, static_cast<size_t>(total) * 16);
  c.alloc(&s->d_cost, static_cast<size_t>(total) * 2);
  c.alloc(&s->d_acts, static_cast<size_t>(total));
  c.alloc(&s->d_solve_counts, static_cast<size_t>(PW_SOLVE_WORDS) * 4);
  if (s->use_keys) c.alloc(&s->d_slot_index, static_cast<size_t>(s->table_slots) * 4);
  c.then([&] { return hipMemsetAsync(s->d_solve_counts, 0, static_cast<size_t>(PW_SOLVE_WORDS) * 4, st); });
  if (!c.ok()) {
    search_table_discard(s);
    return pw_hip_fail("pw_search_solve", c.err);
  }
  auto fail = [&](int code, const std::string& msg) {
    search_table_discard(s);
    return pw_fail(code, msg);
  };
  SearchArgs a = search_args(s);
  uint32_t* counts = s->d_solve_counts;
  const unsigned sblocks = static_cast<unsigned>((total + 255) / 256);
  SolveEvents ev;  // device time of the successor pass / the sweeps / the action bits (pw_search_solve_stats)
  ev.record(0, st);
  if (s->use_keys)
    hipLaunchKernelGGL(pw_solve_index_kernel, dim3(sblocks), dim3(256), 0, st, a, s->N, s->gs, total, s->d_slot_index, counts);
  // successor pass: the store again through the expand kernels, chunk parents at a time
  int64_t passes = 0, lane_passes = 0;
  for (int64_t off = 0; off < total; off += s->chunk) {
    a.first = off;
    a.nparents = static_cast<int32_t>(std::min<int64_t>(s->chunk, total - off));
    a.ncand = 4 * a.nparents;
    passes++;
    if (search_launch_expand(s, a, st, true)) lane_passes++;
    const unsigned cblocks = static_cast<unsigned>((a.ncand + 255) / 256);
    if (s->use_keys)
      hipLaunchKernelGGL(pw_solve_succ_kernel<true>, dim3(cblocks), dim3(256), 0, st, a, s->N, s->d_slot_index, s->d_succ, counts);
    else
      hipLaunchKernelGGL(pw_solve_succ_kernel<false>, dim3(cblocks), dim3(256), 0, st, a, s->N, s->d_slot_index, s->d_succ, counts);
  }
  ev.record(1, st);
  hipLaunchKernelGGL(pw_solve_init_kernel, dim3(sblocks), dim3(256), 0, st, a, total, s->d_cost, counts);
  if (int rc = check_launch("pw_search_solve")) {
    search_table_discard(s);
    return rc;
  }
  // sweeps, PW_SOLVE_BATCH at a time; host[0] is the word of the sweep before the batch (the goal states for the first)
  int64_t max_cost = 0;
  uint32_t goals = 0;
  for (uint32_t k = 1; k < PW_SOLVE_SWEEPS;) {
    const uint32_t nb = std::min<uint32_t>(PW_SOLVE_BATCH, PW_SOLVE_SWEEPS - k);
    for (uint32_t j = 0; j < nb; j++)
      hipLaunchKernelGGL(pw_solve_sweep_kernel, dim3(sblocks), dim3(256), 0, st, s->d_succ, s->d_cost, total, k + j, counts);
    uint32_t host[PW_SOLVE_BATCH + 1];
    hipError_t err = hipMemcpyAsync(host, counts + (k - 1), static_cast<size_t>(nb + 1) * 4, hipMemcpyDeviceToHost, st);
    if (err == hipSuccess) err = hipStreamSynchronize(st);
    if (err != hipSuccess) return fail(PW_EDEVICE, std::string("pw_search_solve: ") + hipGetErrorString(err));
    if (k == 1) goals = host[0];
    bool done = host[0] == 0u;
    for (uint32_t j = 0; j < nb && !done; j++) {
      if (host[j + 1] == 0u) done = true;
      else max_cost = k + j;
    }
    if (done) break;
    k += nb;
  }
  if (max_cost >= PW_SOLVE_INF) return fail(PW_ELIMIT, "pw_search_solve: a finite cost of 65535 or more does not fit the table");
  ev.record(2, st);
  hipLaunchKernelGGL(pw_solve_acts_kernel, dim3(sblocks), dim3(256), 0, st, s->d_succ, s->d_cost, total, s->d_acts, counts);
  if (int rc = check_launch("pw_search_solve")) {
    search_table_discard(s);
    return rc;
  }
  ev.record(3, st);
  uint32_t tail[2] = {0, 0};  // missing, dead ends
  hipError_t err = hipMemcpyAsync(tail, counts + PW_SOLVE_MISSING, sizeof(tail), hipMemcpyDeviceToHost, st);
  if (err == hipSuccess) err = hipStreamSynchronize(st);
  if (err != hipSuccess) return fail(PW_EDEVICE, std::string("pw_search_solve: ") + hipGetErrorString(err));
  if (tail[0] != 0u)
    return fail(PW_EDEVICE, "pw_search_solve: " + std::to_string(tail[0]) +
                                " states are missing from the closed set of an exhausted search (internal error)");
  for (int k = 0; k < 3; k++) s->solve_ms[k] = ev.elapsed(k);
  s->solve_passes = passes;
  s->solve_lane_passes = lane_passes;
  s->solved = true;
  s->table_states = total;
  s->table_max_cost = max_cost;
  info[0] = total;
  info[1] = goals;
  info[2] = tail[1];
  info[3] = max_cost;
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_search_solve_stats(PwSearch* s, double stats[5]) try {
  if (!s || !stats) return pw_fail(PW_EINVAL, "pw_search_solve_stats: null argument");
  if (!s->solved) return pw_fail(PW_EINVAL, "pw_search_solve_stats: no table (call pw_search_solve after the search is exhausted)");
  for (int k = 0; k < 3; k++) stats[k] = s->solve_ms[k];
  stats[3] = static_cast<double>(s->solve_passes);
  stats[4] = static_cast<double>(s->solve_lane_passes);
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_search_table_read(PwSearch* s, int64_t first, int64_t count, int32_t* succ, uint16_t* cost, uint8_t* acts,
                         void* stream) try {
  if (!s) return pw_fail(PW_EINVAL, "pw_search_table_read: null search");
  if (first < 0 || count < 0) return pw_fail(PW_EINVAL, "pw_search_table_read: state range out of bounds");
  if (!s->solved) return pw_fail(PW_EINVAL, "pw_search_table_read: no table (call pw_search_solve after the search is exhausted)");
  if (first + count > s->table_states) return pw_fail(PW_EINVAL, "pw_search_table_read: state range out of bounds");
  if (count == 0) return PW_OK;
  PwDeviceGuard guard(s->eng->set->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t n = static_cast<size_t>(count);
  hipError_t err = hipSuccess;
  if (succ) err = hipMemcpyAsync(succ, s->d_succ + first * 4, n * 16, hipMemcpyDeviceToDevice, st);
  if (err == hipSuccess && cost) err = hipMemcpyAsync(cost, s->d_cost + first, n * 2, hipMemcpyDeviceToDevice, st);
  if (err == hipSuccess && acts) err = hipMemcpyAsync(acts, s->d_acts + first, n, hipMemcpyDeviceToDevice, st);
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string("pw_search_table_read: ") + hipGetErrorString(err));
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_search_table_query(PwSearch* s, const int32_t* puzzle_id, const int8_t* pos, int32_t npad, const uint8_t* mask,
                          int32_t n, int32_t* index, int32_t* cost, uint8_t* acts, void* stream) try {
  if (!s) return pw_fail(PW_EINVAL, "pw_search_table_query: null search");
  if (n < 1) return pw_fail(PW_EINVAL, "pw_search_table_query: n must be >= 1");
  if (!pos) return pw_fail(PW_EINVAL, "pw_search_table_query: null pos");
  if (int rc = pw_check_npad("pw_search_table_query: ", npad)) return rc;
  if (npad < s->N) return pw_fail(PW_EINVAL, "pw_search_table_query: npad is smaller than the puzzle's number of movables");
  if (!s->solved) return pw_fail(PW_EINVAL, "pw_search_table_query: no table (call pw_search_solve after the search is exhausted)");
  PwDeviceGuard guard(s->eng->set->device);
  const PwPuzzleHeader& h = s->eng->set->headers[s->puzzle];
  TableQueryArgs a;
  a.table = s->d_table;
  a.states = s->d_states;
  a.slot_index = s->d_slot_index;
  a.cost = s->d_cost;
  a.acts = s->d_acts;
  a.mask = s->table_slots - 1u;
  a.puzzle = s->puzzle;
  a.n_mov = s->N;
  a.nw = s->NW;
  a.gs = s->gs;
  a.bx = s->use_keys ? s->key_bx : 0;
  a.by = s->use_keys ? s->key_by : 0;
  a.W = h.W;
  a.H = h.H;
  a.puzzle_id = puzzle_id;
  a.pos = pos;
  a.item_mask = mask;
  a.npad = npad;
  a.n = n;
  a.out_index = index;
  a.out_cost = cost;
  a.out_acts = acts;
  const dim3 grid(static_cast<unsigned>((static_cast<int64_t>(n) + 255) / 256)), block(256);
  if (s->use_keys) hipLaunchKernelGGL(pw_table_query_kernel<true>, grid, block, 0, static_cast<hipStream_t>(stream), a);
  else hipLaunchKernelGGL(pw_table_query_kernel<false>, grid, block, 0, static_cast<hipStream_t>(stream), a);
  return check_launch("pw_search_table_query");
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

}  // extern "C"

// pw_push_draw.inc -- the draws from cost-to-go tables over pushes, written once (DESIGN.md K20 and K26).
// Part of the single translation unit pw_kernels.hip, included there after pw_push_table.inc and before its two users,
// pw_push_table_sample.inc (K20: the one table of a PwPushSearch) and pw_push_batch_sample.inc (K26: the pooled tables of a
// PwPushSolveBatch).  Uses the stream constants and the state helpers of pw_table_sample.inc and mix64.
//
//   sample       one thread per environment draws a state uniformly from a band of costs and writes it as a reset would;
//   plans        one thread per item walks best / the optimal rows and succ from a state down to cost 0;
//   emit         one thread per (item, step) writes one flat demonstration row: the push, the cost to go and the state the push
//                is made from, read off the store or the keys -- no flood and no step function.
// The kernels are written against a TABLE VIEW: base pointers and sizes of one table.  The one table of a search is the batch's
// case with one item at offset 0.  Two things are specialised by kBatch, as in K14: which table answers for environment i
// (push_view_of_env) and how a stored state becomes 16 words (push_view_state).  The cost indices are built by the two users: they
// order the buckets by different rules.
// Every loop is bounded by the items, a state's rows, plan_cap or the start's cost.  No kernel waits on another workgroup, there
// is no device assert, and every store is a plain or vector store.

// Where the tables of a handle live.  Members of the other form are NULL / 0.
struct PushDrawSrc {
  const int32_t* cost;   // [states]: K20 the table's, K26 the pool's (so with the per-state and per-row arrays below)
  const int32_t* best;
  const int64_t* srow;   // K20: [states + 1] absolute rows; K26: rows within the item
  const int32_t* succ;   // [rows]
  const uint16_t* from;  // [rows]: x | y << 8 (K20 stores them as int8 pairs)
  const uint8_t* action;
  const uint8_t* flags;
  const int32_t* states_by_cost;  // the cost index, or NULL: none
  const uint32_t* cost_start;     // K20: [max_cost + 3]; K26: ragged over the items, item i at cs_off[i]
  // K26: one table per stored item
  const int32_t* item_of_puzzle;  // [num_puzzles], -1: no stored table
  const int32_t* summary;         // [items][6]
  const int64_t* state_off;       // [items]
  const int64_t* row_off;
  const int64_t* ix_off;          // [items], or NULL: no index
  const int64_t* cs_off;
  const unsigned long long* key;  // [states]: the packed canonical state
  int32_t num_puzzles;
  // K20: the one table
  const int8_t* pos;  // the store: [states][snpad][2] the states as reached
  int64_t states;
  int32_t snpad, n_mov, puzzle, max_cost;
};

struct PushTableView {
  const int32_t* cost;  // per state
  const int32_t* best;
  const int64_t* srow;  // state s owns the rows row_base + [srow[s], srow[s + 1])
  int64_t row_base;     // into succ / from / action / flags of the source
  int64_t state_base;   // into key of the source (K26)
  int64_t states;
  int32_t max_cost;
  const uint32_t* cs;            // its cost_start: max_cost + 3 entries, or NULL: no index
  const int32_t* states_by_cost;
};

// the table that answers for environment i; false: another table's environment, or no stored table for its puzzle here
template <bool kBatch>
__device__ __forceinline__ bool push_view_of_env(const PushDrawSrc& s, const int32_t* puzzle_id, int64_t i, PushTableView& v) {
  if (kBatch) {
    const int32_t pid = puzzle_id[i];
    if (pid < 0 || pid >= s.num_puzzles) return false;
    const int32_t item = s.item_of_puzzle[pid];
    if (item < 0) return false;
    v.state_base = s.state_off[item];
    v.row_base = s.row_off[item];
    if (v.state_base < 0 || v.row_base < 0) return false;
    v.cost = s.cost + v.state_base;
    v.best = s.best + v.state_base;
    v.srow = s.srow + v.state_base;
    v.states = s.summary[static_cast<int64_t>(item) * 6];
    v.max_cost = s.summary[static_cast<int64_t>(item) * 6 + 4];
    const int64_t ix = s.ix_off ? s.ix_off[item] : -1;
    v.cs = ix >= 0 ? s.cost_start + s.cs_off[item] : nullptr;
    v.states_by_cost = ix >= 0 ? s.states_by_cost + ix : nullptr;
    return true;
  }
  if (puzzle_id && puzzle_id[i] != s.puzzle) return false;
  v.cost = s.cost;
  v.best = s.best;
  v.srow = s.srow;
  v.row_base = v.state_base = 0;
  v.states = s.states;
  v.max_cost = s.max_cost;
  v.cs = s.cost_start;
  v.states_by_cost = s.states_by_cost;
  return true;
}

// stored state -> the engine's layout: the key (K26) or the store's int8 pairs (K20)
template <bool kBatch>
__device__ __forceinline__ void push_view_state(const PushDrawSrc& s, const PushTableView& v, int64_t state, uint32_t (&w)[16]) {
  if (kBatch)
    table_key_state(s.key[v.state_base + state], w);
  else
    table_store_state(reinterpret_cast<const uint32_t*>(s.pos + state * s.snpad * 2), s.snpad / 2, s.n_mov, w);
}

// the bucket of a state: its cost, the dead ends after the largest finite cost
__device__ __forceinline__ uint32_t push_table_bucket(int32_t cost, int32_t max_cost) {
  return cost >= 0 && cost <= max_cost ? static_cast<uint32_t>(cost) : static_cast<uint32_t>(max_cost + 1);
}

// ---- sample: one start state per environment, drawn from a band of costs of its own table ---------------------------------------
struct PushSampleArgs {
  PushDrawSrc src;
  const int32_t* puzzle_id;  // [n]; K20: or NULL
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

template <bool kBatch>
__global__ __launch_bounds__(256) void pw_push_sample_kernel(PushSampleArgs a) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= a.n) return;
  if (a.item_mask && a.item_mask[i] == 0) return;
  PushTableView v;
  if (!push_view_of_env<kBatch>(a.src, a.puzzle_id, i, v)) return;  // another table's environment: untouched
  if (!v.cs) return;  // (a stored table is indexed: never)
  const int32_t mc = v.max_cost;
  const int64_t S = v.states;
  const uint32_t finite = mc >= 0 ? v.cs[mc + 1] : 0u;  // states below the dead-end bucket
  if (finite == 0u) {  // nothing can be solved from any state of this table
    a.out_state[i] = -1;
    a.out_cost[i] = -1;
    return;
  }
  int32_t lo = a.lo_n ? a.lo_n[i] : a.lo, hi = a.hi_n ? a.hi_n[i] : a.hi;
  hi = max(hi, lo);
  lo = min(max(lo, 0), mc);
  hi = min(max(hi, 0), mc);
  const uint32_t first = v.cs[lo], end = v.cs[hi + 1];
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
  const int64_t state = v.states_by_cost[first + u];
  if (state < 0 || state >= S) {  // (never, for an index built by this library)
    a.out_state[i] = -1;
    a.out_cost[i] = -1;
    return;
  }
  uint32_t w[16];
  push_view_state<kBatch>(a.src, v, state, w);
  table_write_state(a.pos + i * a.npad * 2, a.npad, w);
  a.steps[i] = 0;
  if (a.term) a.term[i] = 0;
  if (a.trunc) a.trunc[i] = 0;
  a.out_state[i] = static_cast<int32_t>(state);
  a.out_cost[i] = v.cost[state];
}

// ---- plans: a fewest-pushes plan from every given state --------------------------------------------------------------------------
struct PushPlansArgs {
  PushDrawSrc src;
  const int32_t* index;      // [n] states within the table, as the query returns them
  const int32_t* puzzle_id;  // [n]; K20: or NULL
  const uint8_t* item_mask;  // [n] or NULL
  int32_t n, tie, plan_cap;
  uint64_t seed;
  int8_t* plan_from;         // [n][plan_cap][2]
  uint8_t* plan_action;      // [n][plan_cap]
  int32_t* plan_state;       // [n][plan_cap] or NULL
  int32_t* plan_len;         // [n]
};

template <bool kBatch>
__global__ __launch_bounds__(256) void pw_push_plans_kernel(PushPlansArgs a) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= a.n) return;
  if (a.item_mask && a.item_mask[i] == 0) return;
  const PushDrawSrc& t = a.src;
  PushTableView v;
  int64_t cur = a.index[i];
  if (!push_view_of_env<kBatch>(t, a.puzzle_id, i, v) || cur < 0 || cur >= v.states) {
    a.plan_len[i] = -1;
    return;
  }
  const int32_t c = v.cost[cur];
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
    const int64_t r0 = v.row_base + v.srow[cur], r1 = v.row_base + v.srow[cur + 1];
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
      const int32_t k = v.best[cur];
      if (k >= 0 && r0 + k < r1) r = r0 + k;
    }
    if (r < 0) break;  // (only at cost 0: never inside the loop)
    reinterpret_cast<uint16_t*>(a.plan_from)[base + step] = t.from[r];
    a.plan_action[base + step] = t.action[r];
    if (a.plan_state) a.plan_state[base + step] = static_cast<int32_t>(cur);
    step++;
    if (t.flags[r] & 1) break;  // a goal row ends the plan, whatever its successor is
    const int32_t nxt = t.succ[r];
    if (nxt < 0 || nxt >= v.states) break;  // (an optimal row is safe: never)
    cur = nxt;
  }
  a.plan_len[i] = step;
}

// ---- emit: every push of every plan becomes one flat demonstration row -----------------------------------------------------------
struct PushEmitArgs {
  PushDrawSrc src;
  const int32_t* puzzle_id;  // [n]; K20: or NULL
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
template <bool kBatch>
__global__ __launch_bounds__(256) void pw_push_emit_kernel(PushEmitArgs a) {
  const int64_t g = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  const int64_t i = g / a.plan_cap;
  const int32_t step = static_cast<int32_t>(g - i * a.plan_cap);
  if (i >= a.n) return;
  if (a.item_mask && a.item_mask[i] == 0) return;
  PushTableView v;
  if (!push_view_of_env<kBatch>(a.src, a.puzzle_id, i, v)) return;  // another table's item
  const int32_t len = min(a.plan_len[i], a.plan_cap);
  if (step >= len) return;  // (len <= 0: no plan)
  const int64_t at = i * a.plan_cap + step, row = a.offset[i] + step;
  const int64_t state = a.plan_state[at];
  if (row < 0 || row >= a.rows_cap || state < 0 || state >= v.states) {  // (a state outside the table: not a plan of this table)
    atomicAdd(a.dropped, 1u);
    return;
  }
  uint32_t w[16];
  if (step == 0 && a.pos) {
    const uint32_t* live = reinterpret_cast<const uint32_t*>(a.pos + i * a.npad * 2);
#pragma unroll
    for (int k = 0; k < 16; k++) w[k] = 2 * k < a.npad ? live[k] : 0u;
  } else {
    push_view_state<kBatch>(a.src, v, state, w);
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
  table_write_state(a.row_pos + row * a.npad * 2, a.npad, w);
  a.row_item[row] = static_cast<int32_t>(i);
  a.row_t[row] = step;
  a.row_state[row] = static_cast<int32_t>(state);
  reinterpret_cast<int16_t*>(a.row_from)[row] = reinterpret_cast<const int16_t*>(a.plan_from)[at];
  a.row_action[row] = a.plan_action[at];
  a.row_cost[row] = len - step;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
// The argument checks that the two handles share, in the order both entry points make them.  need_puzzle_id: the batch refuses
// a NULL puzzle_id where the one table means "all mine".
static int push_plans_checks(const std::string& f, int32_t n, const int32_t* index, const int32_t* puzzle_id, bool need_puzzle_id,
                             int32_t tie, const int8_t* plan_from, const uint8_t* plan_action, int32_t plan_cap,
                             const int32_t* plan_len) {
  if (n < 1) return pw_fail(PW_EINVAL, f + ": n must be >= 1");
  if (!index) return pw_fail(PW_EINVAL, f + ": null index");
  if (need_puzzle_id && !puzzle_id) return pw_fail(PW_EINVAL, f + ": null puzzle_id");
  if (!plan_from || !plan_action || !plan_len) return pw_fail(PW_EINVAL, f + ": null plan_from / plan_action / plan_len");
  if (plan_cap < 1) return pw_fail(PW_EINVAL, f + ": plan_cap must be >= 1");
  if (tie != 0 && tie != 1) return pw_fail(PW_EINVAL, f + ": tie must be 0 (lowest) or 1 (uniform)");
  return PW_OK;
}

static int push_emit_checks(const std::string& f, const PushEmitArgs& a, bool need_puzzle_id) {
  if (a.n < 1) return pw_fail(PW_EINVAL, f + ": n must be >= 1");
  if (need_puzzle_id && !a.puzzle_id) return pw_fail(PW_EINVAL, f + ": null puzzle_id");
  if (int rc = pw_check_npad(f + ": ", a.npad)) return rc;
  if (!a.plan_from || !a.plan_action || !a.plan_state || !a.plan_len)
    return pw_fail(PW_EINVAL, f + ": null plan_from / plan_action / plan_state / plan_len");
  if (a.plan_cap < 1) return pw_fail(PW_EINVAL, f + ": plan_cap must be >= 1");
  if (!a.offset) return pw_fail(PW_EINVAL, f + ": null offset");
  if (a.rows_cap < 0) return pw_fail(PW_EINVAL, f + ": rows_cap must be >= 0");
  if (a.rows_cap > 0 && (!a.row_item || !a.row_t || !a.row_state || !a.row_from || !a.row_action || !a.row_cost || !a.row_pos))
    return pw_fail(PW_EINVAL, f + ": null row output");  // (rows_cap 0: every row is dropped, the arrays are never written)
  if (!a.dropped) return pw_fail(PW_EINVAL, f + ": null dropped");
  if ((static_cast<int64_t>(a.n) * a.plan_cap + 255) / 256 > 0x7fffffffll)
    return pw_fail(PW_EINVAL, f + ": n * plan_cap is beyond one launch (split the items)");
  return PW_OK;
}

// one thread per environment / item (sample, plans: threads = n) or per (item, step) (emit: threads = n * plan_cap)
template <class Args>
static int push_draw_launch(void (*kernel)(Args), int64_t threads, const Args& a, void* stream, const std::string& f) {
  const dim3 grid(static_cast<unsigned>((threads + 255) / 256)), block(256);
  hipLaunchKernelGGL(kernel, grid, block, 0, static_cast<hipStream_t>(stream), a);
  return check_launch(f.c_str());
}

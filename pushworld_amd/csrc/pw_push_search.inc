// pw_push_search.inc -- K16: breadth-first search over pushes with its closed set on the device.
// Part of the single translation unit pw_kernels.hip (included there after pw_walk.inc: the two floods of a pass run through
// pw_walk_kernel by way of walk_launch, the scans are rocPRIM's).
//
// A node is a canonical state (the packed positions with the agent's slot replaced by canon(s), include/pushworld_amd.h); the
// store keeps the state as reached and its canon, the closed set is a table of fingerprint << 32 | (store index + 1) in HBM,
// linear probing, and a fingerprint match is always confirmed against the canonical state in the store (or, inside a pass,
// against the other candidate's packed state).  One pass over up to `chunk` parents of the newest layer:
//
//   counts     the push moves per parent and the region sizes are in the store (the flood over the successors of the layer
//              before counted them: a parent's region is not flooded a second time); a scan turns the counts into row
//              offsets.  The host reads the row count T -- the pass's only wait.
//   pushes     pw_walk_kernel over the parents (read straight from the store): the T rows (parent, from, action, walk, goal,
//              successor).
//   regions    pw_walk_kernel over the T successors: canon, region size (-1 for one outside its grid), push moves.
//   candidate  packs the canonical state of every row, its first slot and its fingerprint.
//   claim      probes the table: an equal published state ends the candidate; an empty slot takes a tentative entry that
//              carries the candidate id; an equal tentative entry is lowered to the candidate id when that is lower
//              (atomicMin), and the id it replaces is marked lost.  The lowest row with a canonical state owns it.
//   flags, scan, publish, finish
//              owner flags -> ranks in row order (rocPRIM) -> store rows, links and the entries' final form; the lowest goal
//              row ends the store under stop_at_goal.
//
// Every loop is bounded by the rows of the pass, the slots of the table or the length of a chain of links; a probe gives up
// after table_slots steps and raises the overflow flag.  No kernel waits on another workgroup.

#define PW_PS_TENT 0x80000000u
#define PW_PS_NOGOAL 0xFFFFFFFFFFFFFFFFull

// d_info words
#define PW_PS_I_STATES 0    // states in the store
#define PW_PS_I_GOALROW 1   // lowest goal row of the pass that met one (PW_PS_NOGOAL: none yet)
#define PW_PS_I_OVERFLOW 2  // the store (or the table) is full
#define PW_PS_I_GOAL 3      // store index of the goal row's successor (PW_PS_NOGOAL: none)
#define PW_PS_I_ROWS 4      // push rows of the regions launch just made
#define PW_PS_I_REGION 5    // largest walk region of an expanded state
#define PW_PS_I_WORDS 8

struct PwPushSearch {
  PwEngine* eng;
  int32_t puzzle;
  int N, NW, npad, fp_bits;
  int64_t max_states;
  uint64_t table_slots;  // power of two, >= 2 * (max_states + 1)
  int32_t chunk;         // parents per pass
  // the store
  int8_t* d_pos;      // [max_states][npad][2] the state as reached
  int8_t* d_canon;    // [max_states][2]
  int32_t* d_parent;  // [max_states]
  int8_t* d_from;     // [max_states][2]
  uint8_t* d_action;  // [max_states]
  int32_t* d_walk;    // [max_states]
  uint8_t* d_goal;    // [max_states]
  int32_t* d_rsize;   // [max_states] positions of the state's walk region
  int32_t* d_npush;   // [max_states] push moves available in it
  unsigned long long* d_table;
  // the parents of a pass
  int32_t* d_f_size;    // [1] region size of the start state (pw_push_search_begin)
  int64_t* d_f_offset;  // [chunk + 1]
  void* d_f_scan;
  size_t f_scan_bytes;
  // the rows of a pass (grown on demand)
  int64_t row_cap;
  int32_t* d_ids;  // [max(chunk, row_cap)] the puzzle's index
  int32_t* d_row_item;
  int8_t* d_row_from;
  uint8_t* d_row_action;
  int32_t* d_row_walk;
  uint8_t* d_row_goal;
  int8_t* d_row_next;    // [row_cap][npad][2]
  int32_t* d_s_size;     // [row_cap] region_size of the successors
  int8_t* d_s_canon;     // [row_cap][2]
  int64_t* d_s_offset;   // [row_cap + 1] push moves of the successors (the flood's counts, not scanned)
  uint32_t* d_cand_state;  // [row_cap][NW]
  uint32_t* d_cand_hash;   // [row_cap] first slot
  uint32_t* d_cand_fp;     // [row_cap]
  uint32_t* d_cand_slot;   // [row_cap] the slot a candidate holds (valid where d_cand_won)
  uint8_t* d_cand_won;     // [row_cap] written by the candidate itself
  uint8_t* d_cand_lost;    // [row_cap] written by the lower id that took the state over
  uint32_t* d_flag;        // [row_cap + 1] owner flags
  uint32_t* d_rank;        // [row_cap + 1] their exclusive scan
  void* d_r_scan;
  size_t r_scan_bytes;
  uint32_t* d_counter;  // the floods' item counter (they run in stream order, walk_launch zeroes it before each)
  unsigned long long* d_info;
  int64_t layer_begin, layer_end, depth, goal_index, largest;
  int32_t stop_at_goal;
  bool begun, overflow, ended;
  // the cost-to-go table of pw_push_search_solve and the query's workspace (pw_push_table.inc)
  bool t_solved;
  int64_t t_states, t_rows, t_info[5];
  int64_t* d_t_row_off;  // [t_states + 1]
  int32_t* d_t_cost;     // [t_states]
  int32_t* d_t_best;     // [t_states]
  int32_t* d_t_succ;     // [t_rows]
  int8_t* d_t_from;      // [t_rows][2]
  uint8_t* d_t_action;   // [t_rows]
  uint8_t* d_t_flags;    // [t_rows]
  int32_t q_cap;         // items the query's workspace holds
  bool q_maps;           // ... with their walk maps
  uint8_t* d_q_mem;      // one allocation: ids, effective mask, region sizes, canon, push counts, maps
  // the cost index over the table (pw_push_table_sample.inc); discarded with the table
  bool t_index_valid;
  int32_t* d_t_states_by_cost;  // [t_states]
  uint32_t* d_t_cost_start;     // [t_info[4] + 3]
};

static void push_table_discard(PwPushSearch* s);  // (pw_push_table.inc)

struct PushSearchArgs {
  int32_t nw, npad, fp_bits, stop;
  uint32_t mask;  // table_slots - 1
  uint64_t slots;
  int64_t max_states, first;
  int32_t rows;     // T
  int32_t parents;  // P
  const int32_t* plist;  // store index of parent rank i (the best-first search's pop list), or NULL: first + i
  int8_t* pos;
  int8_t* canon;
  int32_t* parent;
  int8_t* from;
  uint8_t* action;
  int32_t* walk;
  uint8_t* goal;
  int32_t* rsize;
  int32_t* npush;
  unsigned long long* table;
  const int32_t* f_size;
  int64_t* f_offset;
  const int32_t* row_item;
  const int8_t* row_from;
  const uint8_t* row_action;
  const int32_t* row_walk;
  const uint8_t* row_goal;
  const int8_t* row_next;
  const int32_t* s_size;
  const int8_t* s_canon;
  const int64_t* s_offset;
  uint32_t* cand_state;
  uint32_t* cand_hash;
  uint32_t* cand_fp;
  uint32_t* cand_slot;
  uint8_t* cand_won;
  uint8_t* cand_lost;
  uint32_t* flag;
  uint32_t* rank;
  unsigned long long* info;
};

// 64 bits of hash of a packed canonical state, word by word: the low word chooses the first slot, the high word is the
// fingerprint
#define PW_PS_HASH_SEED 0x9E3779B97F4A7C15ull
__device__ __forceinline__ unsigned long long push_search_hash_word(unsigned long long h, uint32_t w) {
  h = (h ^ w) * 0xBF58476D1CE4E5B9ull;
  return h ^ (h >> 29);
}
__device__ __forceinline__ unsigned long long push_search_hash_end(unsigned long long h) {
  h ^= h >> 30;
  h *= 0xBF58476D1CE4E5B9ull;
  h ^= h >> 27;
  h *= 0x94D049BB133111EBull;
  return h ^ (h >> 31);
}

__device__ __forceinline__ uint32_t push_search_fp(unsigned long long h, int bits) {
  const uint32_t f = static_cast<uint32_t>(h >> 32);
  return bits >= 32 ? f : (f & ((1u << bits) - 1u));
}

// word k of the canonical state of store row `idx`: the positions as reached, the agent's pair replaced by canon
__device__ __forceinline__ uint32_t push_search_store_word(const PushSearchArgs& a, int64_t idx, int k) {
  uint32_t w = reinterpret_cast<const uint32_t*>(a.pos + idx * a.npad * 2)[k];
  if (k == 0) w = (w & 0xFFFF0000u) | reinterpret_cast<const uint16_t*>(a.canon)[idx];
  return w;
}

// ---- the start state: published as state 0 (the table is empty: its first slot is free) -------------------------------
__global__ void pw_push_search_root_kernel(PushSearchArgs a, int32_t is_goal) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  unsigned long long h = PW_PS_HASH_SEED;
  for (int k = 0; k < a.nw; k++) h = push_search_hash_word(h, push_search_store_word(a, 0, k));
  h = push_search_hash_end(h);
  a.table[static_cast<uint32_t>(h) & a.mask] = (static_cast<unsigned long long>(push_search_fp(h, a.fp_bits)) << 32) | 1ull;
  a.parent[0] = -1;
  reinterpret_cast<int16_t*>(a.from)[0] = 0;
  a.action[0] = 0xFF;
  a.walk[0] = 0;
  a.goal[0] = is_goal ? 1 : 0;
  a.rsize[0] = a.f_size[0];  // (pw_push_search_begin's flood of the start state)
  a.npush[0] = static_cast<int32_t>(a.f_offset[0]);
}

// ---- the parents of a pass: their push counts out of the store (the scan's input), then the row count for the host and
// the largest region ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pw_push_search_counts_kernel(PushSearchArgs a) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i < a.parents) a.f_offset[i] = a.npush[a.first + i];
  if (i == 0) a.f_offset[a.parents] = 0;  // the scan's last input: f_offset[parents] becomes the total
}

__global__ __launch_bounds__(256) void pw_push_search_stat_kernel(PushSearchArgs a) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  int v = i < a.parents ? a.rsize[a.first + i] : 0;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = max(v, __shfl_xor(v, o, PW_WAVE));
  if ((threadIdx.x & 63) == 0 && v > 0) atomicMax(&a.info[PW_PS_I_REGION], static_cast<unsigned long long>(v));
  if (i == 0) a.info[PW_PS_I_ROWS] = static_cast<unsigned long long>(a.f_offset[a.parents]);
}

// ---- (a) candidate: the packed canonical state of every row, its first slot and fingerprint ---------------------------
__global__ __launch_bounds__(256) void pw_push_search_candidate_kernel(PushSearchArgs a) {
  const int64_t r = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (r >= a.rows) return;
  a.cand_won[r] = 0;
  a.cand_lost[r] = 0;
  if (a.s_size[r] <= 0) return;  // a successor outside its grid is no candidate
  const uint32_t* src = reinterpret_cast<const uint32_t*>(a.row_next + r * a.npad * 2);
  uint32_t* dst = a.cand_state + r * a.nw;
  unsigned long long h = PW_PS_HASH_SEED;
  for (int k = 0; k < a.nw; k++) {
    uint32_t w = src[k];
    if (k == 0) w = (w & 0xFFFF0000u) | reinterpret_cast<const uint16_t*>(a.s_canon)[r];
    dst[k] = w;
    h = push_search_hash_word(h, w);
  }
  h = push_search_hash_end(h);
  a.cand_hash[r] = static_cast<uint32_t>(h) & a.mask;
  a.cand_fp[r] = push_search_fp(h, a.fp_bits);
}

// ---- (b) claim -------------------------------------------------------------------------------------------------------
// Entries: fingerprint << 32 | (store index + 1) published, fingerprint << 32 | PW_PS_TENT | row tentative.  Among equal
// fingerprints a published entry is smaller than every tentative one and a tentative one is smaller the lower its row, so
// atomicMin lets the lowest row of a canonical state keep the slot.  An entry only ever changes from empty to tentative and
// from a row to a lower row with the SAME canonical state, so a comparison made against the row read stays true.
__global__ __launch_bounds__(256) void pw_push_search_claim_kernel(PushSearchArgs a) {
  const int64_t c = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (c >= a.rows || a.s_size[c] <= 0) return;
  const uint32_t* my = a.cand_state + c * a.nw;
  const uint32_t fp = a.cand_fp[c];
  const unsigned long long claim = (static_cast<unsigned long long>(fp) << 32) | PW_PS_TENT | static_cast<uint32_t>(c);
  uint32_t slot = a.cand_hash[c];
  for (uint64_t step = 0; step < a.slots; step++, slot = (slot + 1u) & a.mask) {
    // a table that one pass has filled (a layer far beyond max_states): once a candidate has raised the flag the others stop
    // probing -- the search is over either way
    if ((step & 255u) == 255u && __hip_atomic_load(&a.info[PW_PS_I_OVERFLOW], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0ull)
      return;
    unsigned long long v = __hip_atomic_load(&a.table[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (v == 0ull) {
      v = atomicCAS(&a.table[slot], 0ull, claim);
      if (v == 0ull) {
        a.cand_slot[c] = slot;
        a.cand_won[c] = 1;
        return;
      }
    }
    if (static_cast<uint32_t>(v >> 32) != fp) continue;
    const uint32_t low = static_cast<uint32_t>(v);
    const bool tentative = (low & PW_PS_TENT) != 0u;
    bool eq = true;
    if (tentative) {
      const uint32_t* other = a.cand_state + static_cast<int64_t>(low & ~PW_PS_TENT) * a.nw;
      for (int k = 0; k < a.nw; k++) eq = eq && my[k] == other[k];
    } else {
      const int64_t idx = static_cast<int64_t>(low) - 1;
      for (int k = 0; k < a.nw; k++) eq = eq && my[k] == push_search_store_word(a, idx, k);
    }
    if (!eq) continue;
    if (tentative && v > claim) {  // (a lower row already in place: lost without touching the entry)
      const unsigned long long old = atomicMin(&a.table[slot], claim);
      if (old > claim) {
        a.cand_lost[static_cast<uint32_t>(old) & ~PW_PS_TENT] = 1;
        a.cand_slot[c] = slot;
        a.cand_won[c] = 1;
      }
    }
    return;
  }
  a.info[PW_PS_I_OVERFLOW] = 1ull;  // every slot probed: more canonical states than the table was sized for
}

// ---- (c) flags -> scan -> publish -> finish --------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pw_push_search_flag_kernel(PushSearchArgs a) {
  const int64_t r = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  const bool in = r < a.rows;
  if (in) a.flag[r] = (a.cand_won[r] != 0 && a.cand_lost[r] == 0) ? 1u : 0u;
  if (r == 0) a.flag[a.rows] = 0u;  // the scan's last input: rank[rows] becomes the number of owners
  const unsigned long long goals = __ballot(in && a.stop && a.row_goal[r] != 0);
  if (goals != 0ull && (threadIdx.x & 63) == __ffsll(goals) - 1)  // rows ascend with the lanes: the first lane holds the lowest
    atomicMin(&a.info[PW_PS_I_GOALROW], static_cast<unsigned long long>(r));
}

__global__ __launch_bounds__(256) void pw_push_search_publish_kernel(PushSearchArgs a) {
  const int64_t r = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (r >= a.rows) return;
  const unsigned long long g = a.info[PW_PS_I_GOALROW];
  const bool own = a.flag[r] != 0u;
  // rows after the goal row are not published; the goal row's successor always is (it is new: an equal canonical state
  // reached earlier would itself have been a goal)
  if (static_cast<unsigned long long>(r) > g || (!own && static_cast<unsigned long long>(r) != g)) return;
  const int64_t idx = static_cast<int64_t>(a.info[PW_PS_I_STATES]) + a.rank[r];
  if (idx >= a.max_states) return;  // store full: the finish kernel raises the flag
  const uint32_t* src = reinterpret_cast<const uint32_t*>(a.row_next + r * a.npad * 2);
  uint32_t* dst = reinterpret_cast<uint32_t*>(a.pos + idx * a.npad * 2);
  for (int k = 0; k < a.npad / 2; k++) dst[k] = src[k];
  reinterpret_cast<int16_t*>(a.canon)[idx] = reinterpret_cast<const int16_t*>(a.s_canon)[r];
  a.parent[idx] = a.plist ? a.plist[a.row_item[r]] : static_cast<int32_t>(a.first + a.row_item[r]);
  reinterpret_cast<int16_t*>(a.from)[idx] = reinterpret_cast<const int16_t*>(a.row_from)[r];
  a.action[idx] = a.row_action[r];
  a.walk[idx] = a.row_walk[r];
  a.goal[idx] = a.row_goal[r];
  a.rsize[idx] = a.s_size[r];
  a.npush[idx] = static_cast<int32_t>(a.s_offset[r]);
  // the entry becomes (fingerprint, index + 1): the low word; the fingerprint stays
  if (own) reinterpret_cast<uint32_t*>(a.table + a.cand_slot[r])[0] = static_cast<uint32_t>(idx) + 1u;
}

__global__ void pw_push_search_finish_kernel(PushSearchArgs a) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const unsigned long long g = a.info[PW_PS_I_GOALROW];
  unsigned long long total = a.info[PW_PS_I_STATES] + (g != PW_PS_NOGOAL ? a.rank[g] + 1u : a.rank[a.rows]);
  if (total > static_cast<unsigned long long>(a.max_states)) {
    a.info[PW_PS_I_OVERFLOW] = 1ull;
    total = static_cast<unsigned long long>(a.max_states);
  } else if (g != PW_PS_NOGOAL) {
    a.info[PW_PS_I_GOAL] = total - 1ull;
  }
  a.info[PW_PS_I_STATES] = total;
}

// ---- (d) the plan: the chain of links, and the states the pushes of the chain started from ------------------------------
__global__ void pw_push_search_chain_kernel(const int32_t* parent, int64_t index, int32_t cap, int32_t* chain, int32_t* len) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  int n = 0;
  int64_t i = index;
  while (i > 0 && n < cap) {  // (cap: the layers of the search, a chain has one state per layer)
    chain[n++] = static_cast<int32_t>(i);
    i = parent[i];
  }
  *len = i > 0 ? -1 : n;
}

__global__ __launch_bounds__(256) void pw_push_search_gather_kernel(PushSearchArgs a, const int32_t* chain, int32_t len,
                                                                     int8_t* pos, int8_t* from, uint8_t* action, int32_t* walk) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= len) return;
  const int64_t k = chain[j], par = a.parent[k];
  const uint32_t* src = reinterpret_cast<const uint32_t*>(a.pos + par * a.npad * 2);
  uint32_t* dst = reinterpret_cast<uint32_t*>(pos + static_cast<int64_t>(j) * a.npad * 2);
  for (int w = 0; w < a.npad / 2; w++) dst[w] = src[w];
  reinterpret_cast<int16_t*>(from)[j] = reinterpret_cast<const int16_t*>(a.from)[k];
  action[j] = a.action[k];
  walk[j] = a.walk[k];
}

static void push_search_free_rows(PwPushSearch* s) {
  void* bufs[] = {s->d_ids, s->d_row_item, s->d_row_from, s->d_row_action, s->d_row_walk, s->d_row_goal, s->d_row_next,
                  s->d_s_size, s->d_s_canon, s->d_s_offset, s->d_cand_state, s->d_cand_hash, s->d_cand_fp, s->d_cand_slot,
                  s->d_cand_won, s->d_cand_lost, s->d_flag, s->d_rank, s->d_r_scan};
  for (void* b : bufs)
    if (b) (void)hipFree(b);
  s->d_ids = s->d_row_item = s->d_row_walk = s->d_s_size = nullptr;
  s->d_row_from = s->d_row_next = s->d_s_canon = nullptr;
  s->d_row_action = s->d_row_goal = s->d_cand_won = s->d_cand_lost = nullptr;
  s->d_s_offset = nullptr;
  s->d_cand_state = s->d_cand_hash = s->d_cand_fp = s->d_cand_slot = s->d_flag = s->d_rank = nullptr;
  s->d_r_scan = nullptr;
  s->row_cap = 0;
}

// the row buffers for `rows` rows of a pass (the caller has waited for the stream: nothing in flight reads the old ones)
static int push_search_reserve_rows(PwPushSearch* s, int64_t rows, hipStream_t st, const char* what) {
  if (rows <= s->row_cap) return PW_OK;
  push_search_free_rows(s);
  const int64_t cap = std::max<int64_t>(rows + rows / 2, 4096);
  size_t scan_bytes = 0;
  PwHipChain c(rocprim::exclusive_scan(nullptr, scan_bytes, s->d_flag, s->d_rank, 0u, static_cast<size_t>(cap) + 1,
                                       rocprim::plus<uint32_t>(), st));
  scan_bytes = std::max<size_t>(pw_pad256(scan_bytes), 256);
  const size_t n = static_cast<size_t>(cap), ids = static_cast<size_t>(std::max<int64_t>(cap, s->chunk));
  c.alloc(&s->d_ids, ids * 4);
  c.alloc(&s->d_row_item, n * 4);
  c.alloc(&s->d_row_from, n * 2);
  c.alloc(&s->d_row_action, n);
  c.alloc(&s->d_row_walk, n * 4);
  c.alloc(&s->d_row_goal, n);
  c.alloc(&s->d_row_next, n * s->npad * 2);
  c.alloc(&s->d_s_size, n * 4);
  c.alloc(&s->d_s_canon, n * 2);
  c.alloc(&s->d_s_offset, (n + 1) * 8);
  c.alloc(&s->d_cand_state, n * s->NW * 4);
  c.alloc(&s->d_cand_hash, n * 4);
  c.alloc(&s->d_cand_fp, n * 4);
  c.alloc(&s->d_cand_slot, n * 4);
  c.alloc(&s->d_cand_won, n);
  c.alloc(&s->d_cand_lost, n);
  c.alloc(&s->d_flag, (n + 1) * 4);
  c.alloc(&s->d_rank, (n + 1) * 4);
  c.alloc(&s->d_r_scan, scan_bytes);
  c.then([&] { return hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(s->d_ids), s->puzzle, ids, st); });
  if (!c.ok()) {
    push_search_free_rows(s);
    return pw_hip_fail(what, c.err);
  }
  s->r_scan_bytes = scan_bytes;
  s->row_cap = cap;
  return PW_OK;
}

static PushSearchArgs push_search_args(PwPushSearch* s) {
  PushSearchArgs a{};
  a.nw = s->NW;
  a.npad = s->npad;
  a.fp_bits = s->fp_bits;
  a.stop = s->stop_at_goal;
  a.mask = static_cast<uint32_t>(s->table_slots - 1u);
  a.slots = s->table_slots;
  a.max_states = s->max_states;
  a.pos = s->d_pos;
  a.canon = s->d_canon;
  a.parent = s->d_parent;
  a.from = s->d_from;
  a.action = s->d_action;
  a.walk = s->d_walk;
  a.goal = s->d_goal;
  a.rsize = s->d_rsize;
  a.npush = s->d_npush;
  a.table = s->d_table;
  a.f_size = s->d_f_size;
  a.f_offset = s->d_f_offset;
  a.row_item = s->d_row_item;
  a.row_from = s->d_row_from;
  a.row_action = s->d_row_action;
  a.row_walk = s->d_row_walk;
  a.row_goal = s->d_row_goal;
  a.row_next = s->d_row_next;
  a.s_size = s->d_s_size;
  a.s_canon = s->d_s_canon;
  a.s_offset = s->d_s_offset;
  a.cand_state = s->d_cand_state;
  a.cand_hash = s->d_cand_hash;
  a.cand_fp = s->d_cand_fp;
  a.cand_slot = s->d_cand_slot;
  a.cand_won = s->d_cand_won;
  a.cand_lost = s->d_cand_lost;
  a.flag = s->d_flag;
  a.rank = s->d_rank;
  a.info = s->d_info;
  return a;
}

// the regions of `n` states at `pos` through pw_walk_kernel, with the search's own item counter
static void push_search_regions(PwPushSearch* s, const int8_t* pos, int32_t n, int32_t* size, int8_t* canon, int64_t* offset,
                                uint16_t* walk_map, const int32_t* ids, hipStream_t st) {
  WalkArgs w{};
  w.puzzle_id = ids;
  w.pos = pos;
  w.n = n;
  w.npad = s->npad;
  w.emit = 0;
  w.region_size = size;
  w.canon = canon;
  w.offset = offset;
  w.walk_map = walk_map;
  w.map_h = s->eng->set->max_h;
  w.map_w = s->eng->set->max_w;
  w.next_item = s->d_counter;
  walk_launch(s->eng, w, st);
}

// The front half of a pass over `a.parents` parents at `fpos` (contiguous rows; their scanned push counts in d_f_offset,
// a.rows = the total, the row buffers reserved): the two floods and the candidates.  What follows decides what a pass is: claim
// and publish (push_search_pass), or a read-only lookup (pw_push_table.inc).
static void push_search_front(PwPushSearch* s, const PushSearchArgs& a, const int8_t* fpos, hipStream_t st) {
  const int64_t T = a.rows;
  WalkArgs w{};
  w.puzzle_id = s->d_ids;
  w.pos = fpos;
  w.n = a.parents;
  w.npad = s->npad;
  w.emit = 1;
  w.offset = s->d_f_offset;
  w.cap = T;
  w.row_item = s->d_row_item;
  w.row_from = s->d_row_from;
  w.row_action = s->d_row_action;
  w.row_walk = s->d_row_walk;
  w.row_goal = s->d_row_goal;
  w.row_next_pos = s->d_row_next;
  w.next_item = s->d_counter;
  walk_launch(s->eng, w, st);
  push_search_regions(s, s->d_row_next, a.rows, s->d_s_size, s->d_s_canon, s->d_s_offset, nullptr, s->d_ids, st);
  hipLaunchKernelGGL(pw_push_search_candidate_kernel, dim3(static_cast<unsigned>((T + 255) / 256)), dim3(256), 0, st, a);
}

// One pass: the front half, then claim, flags, scan, publish, finish.  Shared by the breadth-first search (a range of the
// store) and the best-first search (pw_push_planner.inc: a gathered pop list, a.plist).
static hipError_t push_search_pass(PwPushSearch* s, const PushSearchArgs& a, const int8_t* fpos, hipStream_t st) {
  const int64_t T = a.rows;
  push_search_front(s, a, fpos, st);
  const dim3 grid(static_cast<unsigned>((T + 255) / 256)), block(256);
  hipLaunchKernelGGL(pw_push_search_claim_kernel, grid, block, 0, st, a);
  hipLaunchKernelGGL(pw_push_search_flag_kernel, grid, block, 0, st, a);
  size_t tmp = s->r_scan_bytes;
  const hipError_t err = rocprim::exclusive_scan(s->d_r_scan, tmp, s->d_flag, s->d_rank, 0u, static_cast<size_t>(T) + 1,
                                                 rocprim::plus<uint32_t>(), st);
  if (err != hipSuccess) return err;
  hipLaunchKernelGGL(pw_push_search_publish_kernel, grid, block, 0, st, a);
  hipLaunchKernelGGL(pw_push_search_finish_kernel, dim3(1), dim3(64), 0, st, a);
  return hipSuccess;
}

static int push_search_create(PwEngine* e, int32_t puzzle, int64_t max_states, int64_t parents, PwPushSearch** out);
static int push_search_plan(PwPushSearch* s, int64_t index, int64_t chain_cap, uint8_t* actions, int32_t cap, int32_t* pushes,
                            void* stream);

extern "C" {

void pw_push_search_destroy(PwPushSearch* s) {
  if (!s) return;
  void* bufs[] = {s->d_pos, s->d_canon, s->d_parent, s->d_from, s->d_action, s->d_walk, s->d_goal, s->d_rsize, s->d_npush,
                  s->d_table, s->d_f_size, s->d_f_offset, s->d_f_scan, s->d_counter, s->d_info};
  for (void* b : bufs)
    if (b) (void)hipFree(b);
  push_search_free_rows(s);
  push_table_discard(s);
  if (s->d_q_mem) (void)hipFree(s->d_q_mem);
  delete s;
}

int pw_push_search_create(PwEngine* e, int32_t puzzle, int64_t max_states, PwPushSearch** out) try {
  if (!e) return pw_fail(PW_EINVAL, "pw_push_search_create: null engine");
  if (!out) return pw_fail(PW_EINVAL, "pw_push_search_create: null out");
  if (max_states < 1 || max_states >= (1ll << 31)) return pw_fail(PW_EINVAL, "pw_push_search_create: max_states must be in 1 .. 2^31 - 1");
  if (puzzle < 0 || puzzle >= e->set->count) return pw_fail(PW_EINVAL, "pw_push_search_create: puzzle index out of range");
  return push_search_create(e, puzzle, max_states, 0, out);
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

}  // extern "C"

// (the arguments are checked; parents > 0: that many parents per pass whatever PW_OPT_SEARCH_CHUNK says -- the best-first
// search's K)
static int push_search_create(PwEngine* e, int32_t puzzle, int64_t max_states, int64_t parents, PwPushSearch** out) {
  PwPushSearch* s = new (std::nothrow) PwPushSearch();
  if (!s) return pw_fail(PW_ENOMEM, "pw_push_search_create: out of memory");
  std::memset(static_cast<void*>(s), 0, sizeof(*s));
  const PwPuzzleHeader& h = e->set->headers[puzzle];
  s->eng = e;
  s->puzzle = puzzle;
  s->N = h.N;
  s->NW = (h.N + 1) / 2;
  s->npad = e->np;
  s->fp_bits = e->push_search_fp_bits > 0 ? e->push_search_fp_bits : 32;  // PW_OPT_PUSH_SEARCH_FP_BITS
  s->max_states = max_states;
  const int64_t chunk = e->search_chunk > 0 ? e->search_chunk : (1 << 16);  // PW_OPT_SEARCH_CHUNK
  s->chunk = static_cast<int32_t>(parents > 0 ? parents : std::min<int64_t>(std::min<int64_t>(chunk, 1 << 24), max_states));
  const uint64_t slots = std::max<uint64_t>(1024, pw_table_slots(static_cast<uint64_t>(max_states) + 1ull));  // load factor below one half
  s->table_slots = slots;
  PwDeviceGuard guard(e->set->device);
  PwHipChain c(guard.status());
  size_t scan_bytes = 0;
  c.then([&] {
    return rocprim::exclusive_scan(nullptr, scan_bytes, s->d_f_offset, s->d_f_offset, static_cast<int64_t>(0),
                                   static_cast<size_t>(s->chunk) + 1, rocprim::plus<int64_t>(), static_cast<hipStream_t>(nullptr));
  });
  s->f_scan_bytes = std::max<size_t>(pw_pad256(scan_bytes), 256);
  const size_t n = static_cast<size_t>(max_states);
  c.alloc(&s->d_pos, n * s->npad * 2);
  c.alloc(&s->d_canon, n * 2);
  c.alloc(&s->d_parent, n * 4);
  c.alloc(&s->d_from, n * 2);
  c.alloc(&s->d_action, n);
  c.alloc(&s->d_walk, n * 4);
  c.alloc(&s->d_goal, n);
  c.alloc(&s->d_rsize, n * 4);
  c.alloc(&s->d_npush, n * 4);
  c.alloc(&s->d_table, static_cast<size_t>(slots) * 8);
  c.alloc(&s->d_f_size, 256);
  c.alloc(&s->d_f_offset, (static_cast<size_t>(s->chunk) + 1) * 8);
  c.alloc(&s->d_f_scan, s->f_scan_bytes);
  c.alloc(&s->d_counter, 64);
  c.alloc(&s->d_info, PW_PS_I_WORDS * sizeof(unsigned long long));
  if (!c.ok()) {
    pw_push_search_destroy(s);
    return pw_hip_fail("pw_push_search_create", c.err);
  }
  *out = s;
  return PW_OK;
}

extern "C" {

int pw_push_search_begin(PwPushSearch* s, const int8_t* start, int32_t stop_at_goal, void* stream) try {
  if (!s) return pw_fail(PW_EINVAL, "pw_push_search_begin: null search");
  const PwPuzzleHeader& h = s->eng->set->headers[s->puzzle];
  alignas(8) int8_t packed[PW_MAX_OBJECTS][2];
  std::memset(packed, 0, sizeof(packed));
  bool goal = true;
  for (int j = 0; j < s->N; j++) {
    const int x = start ? start[2 * j] : h.init[j][0], y = start ? start[2 * j + 1] : h.init[j][1];
    if (x < 0 || y < 0 || x + h.objtab[j].w > h.W || y + h.objtab[j].h > h.H)
      return pw_fail(PW_EINVAL, "pw_push_search_begin: start has a movable outside its grid");
    packed[j][0] = static_cast<int8_t>(x);
    packed[j][1] = static_cast<int8_t>(y);
    if (j >= 1 && j <= h.G && (x != h.goal[j - 1][0] || y != h.goal[j - 1][1])) goal = false;
  }
  PwDeviceGuard guard(s->eng->set->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  s->begun = false;
  push_table_discard(s);
  if (int rc = push_search_reserve_rows(s, 1, st, "pw_push_search_begin")) return rc;  // (the smallest: it grows with the passes)
  const unsigned long long info[PW_PS_I_WORDS] = {1ull, PW_PS_NOGOAL, 0ull, PW_PS_NOGOAL, 0ull, 0ull, 0ull, 0ull};
  hipError_t err = hipMemsetAsync(s->d_table, 0, static_cast<size_t>(s->table_slots) * 8, st);
  if (err == hipSuccess) err = hipMemcpyAsync(s->d_pos, packed, static_cast<size_t>(s->npad) * 2, hipMemcpyHostToDevice, st);
  if (err == hipSuccess) err = hipMemcpyAsync(s->d_info, info, sizeof(info), hipMemcpyHostToDevice, st);
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string("pw_push_search_begin: ") + hipGetErrorString(err));
  PushSearchArgs a = push_search_args(s);
  push_search_regions(s, s->d_pos, 1, s->d_f_size, s->d_canon, s->d_f_offset, nullptr, s->d_ids, st);
  hipLaunchKernelGGL(pw_push_search_root_kernel, dim3(1), dim3(64), 0, st, a, goal ? 1 : 0);
  if (int rc = check_launch("pw_push_search_begin")) return rc;
  err = hipStreamSynchronize(st);  // the sources are stack variables
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string("pw_push_search_begin: ") + hipGetErrorString(err));
  s->layer_begin = 0;
  s->layer_end = 1;
  s->depth = 0;
  s->largest = 0;
  s->stop_at_goal = stop_at_goal ? 1 : 0;
  s->begun = true;
  s->overflow = false;
  s->ended = goal && stop_at_goal;  // a start that is a goal state: the search is over before its first layer
  s->goal_index = s->ended ? 0 : -1;
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_push_search_expand(PwPushSearch* s, int64_t info_out[6], void* stream) try {
  if (!s) return pw_fail(PW_EINVAL, "pw_push_search_expand: null search");
  if (!info_out) return pw_fail(PW_EINVAL, "pw_push_search_expand: null info");
  if (!s->begun) return pw_fail(PW_EINVAL, "pw_push_search_expand: pw_push_search_begin has not been called");
  if (s->overflow) return pw_fail(PW_ELIMIT, "pw_push_search_expand: the state store is full (max_states)");
  if (s->ended) return pw_fail(PW_EINVAL, "pw_push_search_expand: the search has ended at its goal");
  PwDeviceGuard guard(s->eng->set->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t nlayer = s->layer_end - s->layer_begin;
  unsigned long long info[PW_PS_I_WORDS] = {0};
  int64_t layer_rows = 0;
  bool stop = false;  // a pass of this layer met the goal, or filled the store
  hipError_t err = hipSuccess;
  for (int64_t off = 0; off < nlayer; off += s->chunk) {
    PushSearchArgs a = push_search_args(s);
    a.first = s->layer_begin + off;
    a.parents = static_cast<int32_t>(std::min<int64_t>(s->chunk, nlayer - off));
    const int8_t* fpos = s->d_pos + a.first * s->npad * 2;
    const dim3 pgrid(static_cast<unsigned>((a.parents + 255) / 256));
    hipLaunchKernelGGL(pw_push_search_counts_kernel, pgrid, dim3(256), 0, st, a);
    size_t tmp = s->f_scan_bytes;
    err = rocprim::exclusive_scan(s->d_f_scan, tmp, s->d_f_offset, s->d_f_offset, static_cast<int64_t>(0),
                                  static_cast<size_t>(a.parents) + 1, rocprim::plus<int64_t>(), st);
    if (err != hipSuccess) break;
    hipLaunchKernelGGL(pw_push_search_stat_kernel, pgrid, dim3(256), 0, st, a);
    // the pass's one wait: its row count (with it, what the pass before left: the goal, the overflow flag)
    err = hipMemcpyAsync(info, s->d_info, sizeof(info), hipMemcpyDeviceToHost, st);
    if (err == hipSuccess) err = hipStreamSynchronize(st);
    if (err != hipSuccess) break;
    const int64_t T = static_cast<int64_t>(info[PW_PS_I_ROWS]);
    layer_rows += T;
    if (info[PW_PS_I_OVERFLOW] != 0ull) break;
    if (info[PW_PS_I_GOAL] != PW_PS_NOGOAL) stop = true;  // the rest of the layer is counted, not expanded
    if (stop || T == 0) continue;
    if (T >= (1ll << 31) - 1) {
      s->begun = false;
      return pw_fail(PW_ELIMIT, "pw_push_search_expand: 2^31 push rows in one pass (lower PW_OPT_SEARCH_CHUNK)");
    }
    if (int rc = push_search_reserve_rows(s, T, st, "pw_push_search_expand")) {
      s->begun = false;
      return rc;
    }
    a = push_search_args(s);  // (the row buffers may have moved)
    a.first = s->layer_begin + off;
    a.parents = static_cast<int32_t>(std::min<int64_t>(s->chunk, nlayer - off));
    a.rows = static_cast<int32_t>(T);
    err = push_search_pass(s, a, fpos, st);
    if (err != hipSuccess) break;
  }
  if (err == hipSuccess) err = hipGetLastError();
  // the layer's read: what its last pass left
  if (err == hipSuccess) err = hipMemcpyAsync(info, s->d_info, sizeof(info), hipMemcpyDeviceToHost, st);
  if (err == hipSuccess) err = hipStreamSynchronize(st);
  if (err != hipSuccess) {
    s->begun = false;
    return pw_fail(PW_EDEVICE, std::string("pw_push_search_expand: ") + hipGetErrorString(err));
  }
  const int64_t total = static_cast<int64_t>(info[PW_PS_I_STATES]);
  s->layer_begin = s->layer_end;
  s->layer_end = total;
  s->depth += 1;
  s->overflow = info[PW_PS_I_OVERFLOW] != 0ull;
  if (info[PW_PS_I_GOAL] != PW_PS_NOGOAL) {
    s->goal_index = static_cast<int64_t>(info[PW_PS_I_GOAL]);
    s->ended = true;
  }
  s->largest = static_cast<int64_t>(info[PW_PS_I_REGION]);
  info_out[0] = s->depth;
  info_out[1] = s->layer_end - s->layer_begin;
  info_out[2] = total;
  info_out[3] = s->goal_index;
  info_out[4] = layer_rows;
  info_out[5] = s->largest;
  if (s->overflow) return pw_fail(PW_ELIMIT, "pw_push_search_expand: the state store is full (max_states): the last layer is incomplete");
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_push_search_read_states(PwPushSearch* s, int64_t first, int64_t count, int8_t* pos, int8_t* canon, void* stream) try {
  if (!s) return pw_fail(PW_EINVAL, "pw_push_search_read_states: null search");
  if (!s->begun) return pw_fail(PW_EINVAL, "pw_push_search_read_states: pw_push_search_begin has not been called");
  if (first < 0 || count < 0 || first + count > s->layer_end)
    return pw_fail(PW_EINVAL, "pw_push_search_read_states: state range out of bounds");
  PwDeviceGuard guard(s->eng->set->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t err = hipSuccess;
  const size_t n = static_cast<size_t>(count), row = static_cast<size_t>(s->npad) * 2;
  if (n && pos) err = hipMemcpyAsync(pos, s->d_pos + first * row, n * row, hipMemcpyDeviceToDevice, st);
  if (err == hipSuccess && n && canon) err = hipMemcpyAsync(canon, s->d_canon + first * 2, n * 2, hipMemcpyDeviceToDevice, st);
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string("pw_push_search_read_states: ") + hipGetErrorString(err));
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_push_search_read_links(PwPushSearch* s, int64_t first, int64_t count, int32_t* parent, int8_t* from, uint8_t* action,
                              int32_t* walk, uint8_t* goal, void* stream) try {
  if (!s) return pw_fail(PW_EINVAL, "pw_push_search_read_links: null search");
  if (!s->begun) return pw_fail(PW_EINVAL, "pw_push_search_read_links: pw_push_search_begin has not been called");
  if (first < 0 || count < 0 || first + count > s->layer_end)
    return pw_fail(PW_EINVAL, "pw_push_search_read_links: state range out of bounds");
  PwDeviceGuard guard(s->eng->set->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t err = hipSuccess;
  const size_t n = static_cast<size_t>(count);
  auto copy = [&](void* dst, const void* src, size_t bytes) {
    if (err == hipSuccess && n && dst) err = hipMemcpyAsync(dst, src, n * bytes, hipMemcpyDeviceToDevice, st);
  };
  copy(parent, s->d_parent + first, 4);
  copy(from, s->d_from + first * 2, 2);
  copy(action, s->d_action + first, 1);
  copy(walk, s->d_walk + first, 4);
  copy(goal, s->d_goal + first, 1);
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string("pw_push_search_read_links: ") + hipGetErrorString(err));
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_push_search_plan(PwPushSearch* s, int64_t index, uint8_t* actions, int32_t cap, int32_t* pushes, void* stream) try {
  if (!s) return pw_fail(PW_EINVAL, "pw_push_search_plan: null search");
  if (!actions && cap > 0) return pw_fail(PW_EINVAL, "pw_push_search_plan: null actions");
  if (cap < 0) return pw_fail(PW_EINVAL, "pw_push_search_plan: cap must be >= 0");
  if (!s->begun) return pw_fail(PW_EINVAL, "pw_push_search_plan: pw_push_search_begin has not been called");
  if (index < 0 || index >= s->layer_end) return pw_fail(PW_EINVAL, "pw_push_search_plan: state index out of bounds");
  return push_search_plan(s, index, s->depth + 1, actions, cap, pushes, stream);  // (a chain has one state per layer)
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

}  // extern "C"

// (the arguments are checked; chain_cap bounds the chain of links: the layers of a breadth-first search, the states of a
// best-first one)
static int push_search_plan(PwPushSearch* s, int64_t index, int64_t chain_cap64, uint8_t* actions, int32_t cap, int32_t* pushes,
                            void* stream) {
  PwDeviceGuard guard(s->eng->set->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int32_t chain_cap = static_cast<int32_t>(std::min<int64_t>(chain_cap64, (1ll << 31) - 2));
  const int map_h = s->eng->set->max_h, map_w = s->eng->set->max_w;
  const size_t cells = static_cast<size_t>(map_h) * map_w, row = static_cast<size_t>(s->npad) * 2;
  // two allocations for the plan's device buffers: chain + length, then, sized by the chain found: ids, sizes, offsets,
  // positions, links, maps
  struct Release {
    void* p = nullptr;
    ~Release() {
      if (p) (void)hipFree(p);
    }
  } chain_mem, mem;
  const size_t L0 = static_cast<size_t>(chain_cap);
  hipError_t err = hipMalloc(&chain_mem.p, (L0 + 1) * 4);
  if (err != hipSuccess) return pw_hip_fail("pw_push_search_plan", err);
  int32_t* d_chain = static_cast<int32_t*>(chain_mem.p);
  int32_t* d_len = d_chain + L0;
  hipLaunchKernelGGL(pw_push_search_chain_kernel, dim3(1), dim3(64), 0, st, s->d_parent, index, chain_cap, d_chain, d_len);
  int32_t len = 0;
  err = hipMemcpyAsync(&len, d_len, 4, hipMemcpyDeviceToHost, st);
  if (err == hipSuccess) err = hipStreamSynchronize(st);
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string("pw_push_search_plan: ") + hipGetErrorString(err));
  if (len < 0) return pw_fail(PW_EDEVICE, "pw_push_search_plan: the chain of links is longer than the search is deep (an internal error)");
  if (pushes) *pushes = len;
  if (len == 0) return 0;
  const size_t L = static_cast<size_t>(len);
  const size_t o_ids = 0, o_size = o_ids + pw_pad256(L * 4), o_off = o_size + pw_pad256(L * 4), o_pos = o_off + pw_pad256((L + 1) * 8),
               o_from = o_pos + pw_pad256(L * row), o_act = o_from + pw_pad256(L * 2), o_walk = o_act + pw_pad256(L),
               o_map = o_walk + pw_pad256(L * 4), bytes = o_map + pw_pad256(L * cells * 2);
  err = hipMalloc(&mem.p, bytes);
  if (err != hipSuccess) return pw_hip_fail("pw_push_search_plan", err);
  uint8_t* base = static_cast<uint8_t*>(mem.p);
  int32_t* d_ids = reinterpret_cast<int32_t*>(base + o_ids);
  int8_t* d_gpos = reinterpret_cast<int8_t*>(base + o_pos);
  int8_t* d_gfrom = reinterpret_cast<int8_t*>(base + o_from);
  uint8_t* d_gact = base + o_act;
  int32_t* d_gwalk = reinterpret_cast<int32_t*>(base + o_walk);
  uint16_t* d_map = reinterpret_cast<uint16_t*>(base + o_map);
  err = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_ids), s->puzzle, L, st);
  if (err == hipSuccess) err = hipMemsetAsync(d_map, 0xff, L * cells * 2, st);
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string("pw_push_search_plan: ") + hipGetErrorString(err));
  PushSearchArgs a = push_search_args(s);
  hipLaunchKernelGGL(pw_push_search_gather_kernel, dim3(static_cast<unsigned>((len + 255) / 256)), dim3(256), 0, st, a, d_chain, len,
                     d_gpos, d_gfrom, d_gact, d_gwalk);
  push_search_regions(s, d_gpos, len, reinterpret_cast<int32_t*>(base + o_size), nullptr, reinterpret_cast<int64_t*>(base + o_off),
                      d_map, d_ids, st);
  if (int rc = check_launch("pw_push_search_plan")) return rc;
  std::vector<uint16_t> maps(L * cells);
  std::vector<int8_t> from(L * 2);
  std::vector<uint8_t> act(L);
  std::vector<int32_t> walk(L);
  err = hipMemcpyAsync(maps.data(), d_map, L * cells * 2, hipMemcpyDeviceToHost, st);
  if (err == hipSuccess) err = hipMemcpyAsync(from.data(), d_gfrom, L * 2, hipMemcpyDeviceToHost, st);
  if (err == hipSuccess) err = hipMemcpyAsync(act.data(), d_gact, L, hipMemcpyDeviceToHost, st);
  if (err == hipSuccess) err = hipMemcpyAsync(walk.data(), d_gwalk, L * 4, hipMemcpyDeviceToHost, st);
  if (err == hipSuccess) err = hipStreamSynchronize(st);
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string("pw_push_search_plan: ") + hipGetErrorString(err));
  int64_t total = static_cast<int64_t>(len);
  for (size_t j = 0; j < L; j++) total += walk[j];
  if (total > (1ll << 31) - 1) return pw_fail(PW_ELIMIT, "pw_push_search_plan: plan longer than 2^31 - 1 actions");
  if (total > cap) return static_cast<int>(total);  // caller retries with a larger buffer
  // chain[0] is state `index`: the plan is written from its end
  static const int kDx[4] = {-1, 1, 0, 0}, kDy[4] = {0, 0, -1, 1};
  int64_t at = total;
  for (size_t j = 0; j < L; j++) {
    actions[--at] = act[j];
    const uint16_t* m = maps.data() + j * cells;
    int x = from[2 * j], y = from[2 * j + 1];
    for (int32_t k = 0; k < walk[j]; k++) {  // from the push's starting position back along the parent actions
      const bool inside = x >= 0 && y >= 0 && x < map_w && y < map_h;
      const uint16_t e = inside ? m[static_cast<size_t>(y) * map_w + x] : 0xFFFFu;
      if (e == 0xFFFFu || (e & 0xFFFu) != static_cast<uint32_t>(walk[j] - k))
        return pw_fail(PW_EDEVICE, "pw_push_search_plan: a link's walk does not follow its walk map (an internal error)");
      const int d = e >> 12;
      actions[--at] = static_cast<uint8_t>(d);
      x -= kDx[d];
      y -= kDy[d];
    }
  }
  return static_cast<int>(total);
}

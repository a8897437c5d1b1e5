// pw_search.inc -- breadth-first frontier services for the planner (SURVEY 8-f3).
// Included at the end of pw_kernels.hip (uses its LanePuzzle helpers; one translation unit).
//
// The reference planner expands one node at a time and keeps its closed set in a
// std::unordered_set<State> (cpp/include/search/best_first_search.h:72-93).  Here a whole BFS
// layer is expanded per call and the closed set is an open-addressing table in HBM:
//
//   store    states[i]   uint16 (x | y << 8) per movable, NW = ceil(N / 2) 32-bit words per state
//            parent[i], action[i]                         (state 0 = start, parent -1)
//   table    uint64 slots: low word 0 empty | i + 1 published state i | 0x80000000 | c tentative claim of
//            candidate c during a pass; high word = a 32-bit fingerprint of the state (a second hash of its words):
//            a probe reads ONE 8-byte slot and goes on to the (random) read of the stored state only when the
//            fingerprints agree -- the full compare stays, so the closed set is exact
//
// One pass over <= chunk parents of the current layer = five launches:
//   expand   GS lanes per parent (lane = movable, as pw_step_group_kernel): the 4 successors;
//            those that moved are written to the candidate scratch with their start slot
//   claim    thread per candidate: linear probing; equal published state -> duplicate; empty slot
//            -> 64-bit CAS of (fingerprint, tentative claim); equal tentative state -> 64-bit atomicMin (same
//            fingerprint, so the LOWEST candidate id = parent order, then action order, owns a state discovered
//            several times)
//   count / scan / publish   owners are numbered by an exclusive scan in candidate order and
//            appended to the store; their slot becomes a published entry.  count leaves the owner flags of its 256
//            candidates as four ballots; publish reads those instead of probing the table again
// Round 5 (VERDICT r4 #3: 1.1 KB of random 64-byte sectors per parent, claim 57 % / count 20 % / publish 12 % of it):
//   * LOST FLAGS: who owns a state that several candidates of a pass discover is settled where the claims meet -- a claim that
//     takes a slot over from a higher candidate id marks that candidate in cand_lost (a 4-byte array indexed by candidate id:
//     sequential for its readers, L2-sized), one that finds a lower id in place gives up at once.  count / novelty / publish
//     read cand_slot and cand_lost only: the second random read of every new state's slot is gone.
//   * BUCKETS: the first probe slot is rounded down to a 64-byte line of 8 slots, which a candidate reads whole (four 16-byte
//     loads, one sector) and scans in registers: the probe chain of linear probing -- every step of it a random access of its
//     own -- collapses into the line (a bucket is full for one candidate in thousands at load <= 0.5).
//   * EXACT KEYS (states that pack into 63 bits: bx + by bits per movable, e.g. `Pull Dont Push`; the start state must not
//     overlap a wall, which keeps every movable inside the grid for good): a PUBLISHED entry is the packed state itself, so a
//     visited state -- 3 of 4 candidates of a breadth-first search -- is recognised from the line alone, without the random
//     read of "the other state's words" the fingerprinted entries need.  Tentative entries stay (bit 63 | candidate id).
//   What the claim kernel is bound by is the RATE of random 64-byte accesses (~50 G/s on this chip, profiles/r04_launch_floor
//   chain probe), not their bytes: per probing candidate 1 line + 0.25 CAS (+ 0.75 reads of another state without exact keys)
//   instead of ~1.3 lines + 0.25 CAS + 0.75 reads.  MEASURED (both 40 M-state searches of tools/bench_search.py, 2 x FETCH_SIZE +
//   WRITE_SIZE, profiles/r05_search_big_* against r04_search_big_*): 1.14 -> 0.91 KB of HBM traffic per parent, all of it the
//   count kernel's (241 -> 33 bytes: the lost flags); the claim kernel's ~0.62 KB did not move with the buckets, and exact keys
//   move the same bytes as the fingerprinted entries (the reads they save hit the caches: the duplicates of a breadth-first
//   search are the states of the last two layers) and are 6 % slower (the key arithmetic), so they are an option, not the
//   default.  Neither makes the search faster -- 2.9e9 parents/s either way, and the same with a table an eighth the size: the
//   claim kernel waits 86 % of its time on its dependent chain of 3 .. 5 accesses per candidate at the hardware's 8 wavefronts
//   per SIMD (profiles/r05_atomic_probe.txt: the chip's random-read and CAS rates are not reached), bound by neither bytes nor
//   DRAM locality.  (A 16-byte {key, epoch | candidate} slot that needs no
//   write at publication was tried first: two atomics per new state and two atomic loads per probe -- 1.37x the bytes, no faster.)
// The numbering therefore equals the one a sequential FIFO breadth-first search (actions in the
// order L, R, U, D) assigns: results are deterministic and comparable entry by entry with a host
// BFS over the oracle (tests/test_gpu_search.py).


// ====================================================================================================
// Novelty tables (cpp/src/heuristics/novelty.cc:20-77, SURVEY 8-f3)
//
// The reference keeps unordered_sets of visited positions per object and of visited position pairs
// per object pair and evaluates states ONE AT A TIME: novelty 1 if a moved object is at a new
// position, 2 if a (moved object, other object) position pair is new, else 3; all atoms of the moved
// objects are inserted whatever the result.  The batched form evaluates a whole array of states with
// the result of feeding them to the reference IN INDEX ORDER: every atom has a uint32 entry holding
// the id of the first state that produced it (0xFFFFFFFF = never); a batch first atomicMin's the
// ids of all its atoms (mark), then a state's atom is new exactly when its entry equals the state's
// own id (resolve).  Ids grow monotonically across calls, so older batches always win.
//   single  [N][D]                 D = width * height positions, index y * width + x
//   pair    [N (N - 1) / 2][D][D]  pair (i < j) -> entry p_i * D + p_j
// ====================================================================================================
struct NoveltyTables {
  uint32_t* single;
  uint32_t* pair;
  int N, W, H, D;
};

struct PwNovelty {
  int device;
  NoveltyTables t;
  size_t single_bytes, pair_bytes;
  int32_t* d_bad;  // device flag: a position outside the domain was seen
  uint32_t next_id;
};

__device__ __forceinline__ int64_t novelty_pair_base(const NoveltyTables& t, int lo, int hi) {
  const int pid = lo * t.N - (lo * (lo + 1)) / 2 + (hi - lo - 1);
  return static_cast<int64_t>(pid) * t.D * t.D;
}

// One group of 32 lanes = one state (lane j = object j, pj = its position index or -1 beyond N).
// kMark: record the state's atoms under `id`.  !kMark: returns the novelty (same value on every lane
// of the group).  Must be called by all 64 lanes of the wave; `active` is group-uniform.
template <bool kMark>
__device__ __forceinline__ int novelty_group(const NoveltyTables& t, int lj, int gbase, unsigned long long gmask,
                                             bool active, int pj, uint32_t moved, uint32_t id) {
  bool new1 = false, new2 = false;
  for (int i = 0; i < t.N; i++) {
    const int pi = __shfl(pj, gbase + i, PW_WAVE);
    if (!active || !((moved >> i) & 1u) || lj >= t.N) continue;
    uint32_t* entry;
    if (lj == i) {
      entry = t.single + static_cast<int64_t>(i) * t.D + pi;
    } else {
      const bool lower = lj < i;
      entry = t.pair + novelty_pair_base(t, lower ? lj : i, lower ? i : lj) +
              static_cast<int64_t>(lower ? pj : pi) * t.D + (lower ? pi : pj);
    }
    if (kMark) {
      atomicMin(entry, id);
    } else {
      const bool mine = *entry == id;
      new1 = new1 || (mine && lj == i);
      new2 = new2 || (mine && lj != i);
    }
  }
  if (kMark) return 0;
  const bool any1 = (__ballot(new1) & gmask) != 0ull, any2 = (__ballot(new2) & gmask) != 0ull;
  return any1 ? 1 : (any2 ? 2 : 3);
}

struct NoveltyEvalArgs {
  NoveltyTables t;
  const int32_t* states;  // [count][N] Position2D
  const uint32_t* moved;  // [count]
  uint8_t* out;           // [count]
  int32_t* bad;           // set to 1 when a position lies outside the width x height domain
  uint32_t id_base;
  int32_t count;
};

template <bool kMark>
__global__ __launch_bounds__(256) void pw_novelty_eval_kernel(NoveltyEvalArgs a) {
  const int lane = threadIdx.x & (PW_WAVE - 1);
  const int lj = threadIdx.x & 31;
  const int gbase = lane & ~31;
  const unsigned long long gmask = 0xFFFFFFFFull << gbase;
  const int64_t s = static_cast<int64_t>(blockIdx.x) * 8 + threadIdx.x / 32;
  const bool live = s < a.count;
  int pj = -1;
  bool ok = true;
  if (live && lj < a.t.N) {
    const int32_t v = a.states[s * a.t.N + lj];
    const int x = v / PW_POSITION_LIMIT, y = v % PW_POSITION_LIMIT;
    ok = v >= 0 && x < a.t.W && y < a.t.H;
    pj = ok ? y * a.t.W + x : 0;
  }
  const bool good = (__ballot(!ok) & gmask) == 0ull;
  if (live && !good && lj == 0) *a.bad = 1;
  const uint32_t moved = live ? a.moved[s] : 0u;
  const int nov = novelty_group<kMark>(a.t, lj, gbase, gmask, live && good, pj, moved, a.id_base + static_cast<uint32_t>(s));
  if (!kMark && live && lj == 0) a.out[s] = static_cast<uint8_t>(nov);
}

extern "C" {

void pw_novelty_destroy(PwNovelty* n) {
  if (!n) return;
  if (n->t.single) (void)hipFree(n->t.single);
  if (n->t.pair) (void)hipFree(n->t.pair);
  if (n->d_bad) (void)hipFree(n->d_bad);
  delete n;
}

static int novelty_alloc(int device, int state_size, int width, int height, PwNovelty** out) {
  if (state_size < 1 || state_size > PW_MAX_OBJECTS || width < 1 || width > PW_MAX_DIM || height < 1 || height > PW_MAX_DIM)
    return pw_fail(PW_EINVAL, "novelty tables: state_size in 1..32, width/height in 1..64");
  PwNovelty* n = new (std::nothrow) PwNovelty();
  if (!n) return pw_fail(PW_ENOMEM, "out of memory");
  std::memset(static_cast<void*>(n), 0, sizeof(*n));
  n->device = device;
  n->t.N = state_size;
  n->t.W = width;
  n->t.H = height;
  n->t.D = width * height;
  const size_t d = static_cast<size_t>(n->t.D);
  n->single_bytes = static_cast<size_t>(state_size) * d * 4;
  n->pair_bytes = static_cast<size_t>(state_size) * (state_size - 1) / 2 * d * d * 4;
  PwDeviceGuard guard(device);
  hipError_t err = guard.status();
  if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&n->t.single), n->single_bytes);
  if (err == hipSuccess && n->pair_bytes) err = hipMalloc(reinterpret_cast<void**>(&n->t.pair), n->pair_bytes);
  if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&n->d_bad), 4);
  if (err != hipSuccess) {
    pw_novelty_destroy(n);
    return pw_hip_fail("novelty tables", err);
  }
  *out = n;
  return PW_OK;
}

int pw_novelty_reset(PwNovelty* n, void* stream) try {
  if (!n) return pw_fail(PW_EINVAL, "null argument");
  PwDeviceGuard guard(n->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t err = hipMemsetAsync(n->t.single, 0xFF, n->single_bytes, st);
  if (err == hipSuccess && n->pair_bytes) err = hipMemsetAsync(n->t.pair, 0xFF, n->pair_bytes, st);
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string("pw_novelty_reset: ") + hipGetErrorString(err));
  n->next_id = 0;
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_novelty_create(int device, int state_size, int width, int height, PwNovelty** out) try {
  if (!out) return pw_fail(PW_EINVAL, "null argument");
  if (int rc = novelty_alloc(device, state_size, width, height, out)) return rc;
  if (int rc = pw_novelty_reset(*out, nullptr)) {
    pw_novelty_destroy(*out);
    *out = nullptr;
    return rc;
  }
  PwDeviceGuard guard(device);
  (void)hipStreamSynchronize(nullptr);
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_novelty_eval(PwNovelty* n, const int32_t* states, const uint32_t* moved, uint8_t* novelty, int32_t count,
                    void* stream) try {
  if (!n || !states || !moved || !novelty) return pw_fail(PW_EINVAL, "null argument");
  if (count <= 0) return PW_OK;
  if (static_cast<uint64_t>(n->next_id) + static_cast<uint64_t>(count) >= 0xFFFFFFFFull)
    return pw_fail(PW_ELIMIT, "novelty tables: 2^32 state ids used up, call pw_novelty_reset");
  PwDeviceGuard guard(n->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t err = hipMemsetAsync(n->d_bad, 0, 4, st);
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string("pw_novelty_eval: ") + hipGetErrorString(err));
  NoveltyEvalArgs a{n->t, states, moved, novelty, n->d_bad, n->next_id, count};
  const unsigned blocks = static_cast<unsigned>((count + 7) / 8);
  hipLaunchKernelGGL(pw_novelty_eval_kernel<true>, dim3(blocks), dim3(256), 0, st, a);
  hipLaunchKernelGGL(pw_novelty_eval_kernel<false>, dim3(blocks), dim3(256), 0, st, a);
  n->next_id += static_cast<uint32_t>(count);
  int32_t bad = 0;
  err = hipMemcpyAsync(&bad, n->d_bad, 4, hipMemcpyDeviceToHost, st);
  if (err == hipSuccess) err = hipStreamSynchronize(st);
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string("pw_novelty_eval: ") + hipGetErrorString(err));
  if (bad) return pw_fail(PW_EINVAL, "pw_novelty_eval: a position lies outside the width x height domain (that state was skipped)");
  return check_launch("pw_novelty_eval");
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

}  // extern "C"

// ====================================================================================================
// Breadth-first search
// ====================================================================================================
#define PW_S_NONE 0xFFFFFFFFu
#define PW_S_TENT 0x80000000u

struct PwSearch {
  PwEngine* eng;
  int32_t puzzle;
  int N, G, NW, gs;
  int64_t max_states;
  uint32_t table_slots;  // power of two
  int32_t chunk;         // parents per pass
  uint32_t* d_states;
  int32_t* d_parent;
  uint8_t* d_action;
  unsigned long long* d_table;  // [table_slots] fingerprint << 32 | entry
  unsigned long long* d_owner;  // [4 * chunk / 64] owner flags of the candidates, one ballot per wavefront
  uint32_t* d_cand_lost;   // [4 * chunk] epoch of the pass in which a lower candidate id took this candidate's state over
  uint32_t epoch;          // pass counter (1 ..): what "this pass" is in d_cand_lost
  int key_bx, key_by;      // exact keys: bits per x / y (0: fingerprinted entries)
  bool use_keys;           // this search runs on them (pw_search_begin: the start state overlaps no wall)
  uint32_t* d_cand_state;  // [4 * chunk][NW]
  uint32_t* d_cand_hash;   // [4 * chunk] first probe slot | PW_S_NONE (did not move)
  uint32_t* d_cand_slot;   // [4 * chunk] slot the candidate ended at | PW_S_NONE (already visited)
  uint8_t* d_cand_goal;    // [4 * chunk]
  uint32_t* d_block_off;   // [4 * chunk / 256 + 1]
  unsigned long long* d_info;  // [0] states in the store, [1] lowest goal state index, [2] overflow flag
  uint8_t* d_plan;
  int32_t plan_cap;
  int64_t layer_begin, layer_end, depth, goal_index;
  bool begun, overflow;
  // width-limited search (IW(k)): novelty of every new state, states above the width are kept in the
  // closed set but not expanded
  int32_t width;           // 0 = plain breadth-first search
  PwNovelty* nov;
  uint8_t* d_pruned;       // [max_states]
  uint32_t* d_cand_moved;  // [4 * chunk] moved-object mask (pushworld_puzzle.cc:446-457)
  uint8_t* d_cand_nov;     // [4 * chunk]
  // exact cost-to-go table (pw_search_solve, csrc/pw_solution.inc): one row per state of the exhausted store
  bool exhausted;          // the last pw_search_expand found no new state
  bool solved;             // the table below is valid
  int64_t table_states;    // rows
  int32_t* d_succ;         // [table_states][4] store index of the successor under L, R, U, D (the state itself: nothing moves)
  uint16_t* d_cost;        // [table_states] length of a shortest way to a goal state, 0xFFFF = none (dead end)
  uint8_t* d_acts;         // [table_states] bits 0..3 optimal actions, bits 4..7 safe actions
  uint32_t* d_slot_index;  // [table_slots] exact keys only: store index of the state published in each slot
  uint32_t* d_solve_counts;  // pw_search_solve's device words (states settled per sweep, then the totals)
  float solve_ms[3];       // device milliseconds of the last pw_search_solve: successor pass, sweeps, action bits
  int64_t solve_passes, solve_lane_passes;  // its successor passes, and how many of them ran one lane per parent
  // cost index of the table (pw_search_table_index, csrc/pw_table_sample.inc)
  int64_t table_max_cost;  // largest finite cost of the table
  bool index_valid;
  int32_t* d_rows_by_cost;  // [table_states] the rows grouped by cost, the dead ends last
  uint32_t* d_cost_start;   // [table_max_cost + 3]
};

static void search_index_discard(PwSearch* s) {
  if (s->d_rows_by_cost) (void)hipFree(s->d_rows_by_cost);
  if (s->d_cost_start) (void)hipFree(s->d_cost_start);
  s->d_rows_by_cost = nullptr;
  s->d_cost_start = nullptr;
  s->index_valid = false;
}

// the cost-to-go table goes with the search it was computed from (pw_search_begin, pw_search_destroy)
static void search_table_discard(PwSearch* s) {
  search_index_discard(s);
  void* bufs[] = {s->d_succ, s->d_cost, s->d_acts, s->d_slot_index, s->d_solve_counts};
  for (void* b : bufs)
    if (b) (void)hipFree(b);
  s->d_succ = nullptr;
  s->d_cost = nullptr;
  s->d_acts = nullptr;
  s->d_slot_index = nullptr;
  s->d_solve_counts = nullptr;
  s->solved = false;
  s->table_states = 0;
}

struct SearchArgs {
  const PwPuzzleHeader* hdrs;
  const uint8_t* blob;
  int32_t puzzle;
  int32_t nw;
  uint32_t* states;
  int32_t* parent;
  uint8_t* action;
  unsigned long long* table;
  unsigned long long* owner;
  uint32_t* cand_lost;
  uint32_t epoch;
  int32_t key_bx, key_by;  // 0: fingerprint table
  uint32_t mask;
  uint32_t* cand_state;
  uint32_t* cand_hash;
  uint32_t* cand_slot;
  uint8_t* cand_goal;
  uint32_t* block_off;
  unsigned long long* info;
  int64_t first;       // store index of the first parent of this pass
  int32_t nparents;
  int32_t ncand;       // 4 * nparents
  int64_t max_states;
  uint8_t* pruned;     // NULL for plain breadth-first search
  uint32_t* cand_moved;
  uint8_t* cand_nov;
  int32_t width;
  uint32_t id_base;    // novelty id of candidate 0 of this pass
  NoveltyTables nt;
  const uint64_t* ovl;      // overlap tables (PwOvlDir), or NULL
  const PwOvlDir* ovl_dir;
  const PwPushDir* push_dir;  // push tables (pw_search_expand_lane_kernel), or NULL
  // best-first rounds (pw_planner.inc; all NULL for breadth-first search):
  const int32_t* plist;            // [nparents] store index of the parent of each pop rank (-1: none), instead of first + rank
  const uint8_t* pperm;            // [nparents] action group of each rank: action at position p = bits 2p..2p+1; candidate
                                   // slot of action a = 4 rank + its position
  const unsigned long long* halt;  // every kernel returns at once while *halt != 0
  uint8_t* state_nov;              // [max_states] novelty of each published state
};

// position-dependent 32-bit hash of a state: per-movable mix, summed over the GS lanes of a group
// (lanes beyond N hold 0), final avalanche.  Host copy: the start state is inserted by pw_search_begin.
__host__ __device__ __forceinline__ uint32_t search_lane_term(uint32_t xy, uint32_t lj) {
  uint32_t t = (xy | (lj << 16)) * 0x85EBCA6Bu;
  t ^= t >> 13;
  return t * 0xC2B2AE35u;
}
__host__ __device__ __forceinline__ uint32_t search_final(uint32_t t) {
  t ^= t >> 16;
  t *= 0x7FEB352Du;
  t ^= t >> 15;
  t *= 0x846CA68Bu;
  return t ^ (t >> 16);
}

// fingerprint of a packed state (nw 32-bit words): independent of the slot hash, computed where the words are at hand
// (claim kernel; host copy for the start state)
__host__ __device__ __forceinline__ uint32_t search_fingerprint(const uint32_t* w, int nw) {
  uint32_t f = 0x9E3779B9u;
  for (int k = 0; k < nw; k++) {
    f = (f ^ w[k]) * 0x01000193u;
    f = (f << 13) | (f >> 19);
    f *= 0x5BD1E995u;
  }
  f ^= f >> 15;
  return f * 0x2C1B3C6Du;
}

// exact key of a packed state: (x | y << bx) of movable j at bit j * (bx + by); N * (bx + by) <= 63 (bit 63 marks a tentative
// entry) and never 0 (the agent stands inside the border ring: x >= 1)
#define PW_S_TENT64 0x8000000000000000ull
__host__ __device__ __forceinline__ unsigned long long search_key(const uint32_t* w, int n, int bx, int by) {
  unsigned long long key = 0ull;
  for (int j = 0; j < n; j++) {
    const uint32_t xy = (w[j >> 1] >> (16 * (j & 1))) & 0xffffu;
    key |= static_cast<unsigned long long>((xy & 0xffu) | ((xy >> 8) << bx)) << (j * (bx + by));
  }
  return key;
}

// ---- expand: the 4 successors of every parent of the pass -----------------------------------------
// kTwo: two movables per lane (slots lj and GS + lj), as pw_expand4_kernel: puzzles with 9 .. 16 movables in 8-lane groups
template <int GS, bool kTab = false, bool kTwo = false>
__global__ __launch_bounds__(256) void pw_search_expand_kernel(SearchArgs a) {
  constexpr int kGroups = 256 / GS;
  const int lane = threadIdx.x & (PW_WAVE - 1);
  const int lj = threadIdx.x & (GS - 1);
  const int gbase = lane & ~(GS - 1);
  const unsigned long long gmask = ((1ull << (GS - 1) << 1) - 1ull) << gbase;
  if (a.halt && *a.halt) return;
  const int g = blockIdx.x * kGroups + static_cast<int>(threadIdx.x) / GS;
  bool live = g < a.nparents;
  const int gg = live ? g : 0;
  int64_t pidx = a.first + gg;
  if (a.plist) {  // best-first round: the popped parent of rank gg
    const int32_t v = a.plist[gg];
    live = live && v >= 0;
    pidx = v >= 0 ? v : 0;
  }
  if (a.pruned && a.pruned[pidx]) live = false;  // above the novelty width: closed, not expanded
  uint32_t slot_of = 0xE4u;  // 2-bit candidate slot of each action (identity: L R U D)
  if (a.pperm) {
    const uint32_t perm = a.pperm[gg];
    slot_of = 0u;
    for (int p = 0; p < 4; p++) slot_of |= static_cast<uint32_t>(p) << (2 * ((perm >> (2 * p)) & 3u));
  }

  LanePuzzleT<const uint64_t*, kTab ? 2 : 0> p;
  const PwPuzzleHeader* h = a.hdrs + a.puzzle;
  p.h = h;
  {
    const uint8_t* b = a.blob + h->base;
    p.wall = reinterpret_cast<const uint64_t*>(b + h->off_wall);
    p.awall = reinterpret_cast<const uint64_t*>(b + h->off_awall);
    p.shapes = reinterpret_cast<const uint64_t*>(b + h->off_shapes);
  }
  lane_tables(p, a.ovl, a.ovl_dir, a.puzzle);
  p.H = h->H;
  p.N = h->N;
  p.G = h->G;
  const int N = p.N;
  const uint16_t* srow = reinterpret_cast<const uint16_t*>(a.states + pidx * a.nw);
  const uint64_t* smalls = reinterpret_cast<const uint64_t*>(a.blob + h->base + h->off_small);
  const int xy = (lj < N) ? static_cast<int>(srow[lj]) : 0;
  const uint32_t ot = (lj < N) ? reinterpret_cast<const uint32_t*>(h->objtab)[lj] : 0u;
  const uint64_t small = (lj < N) ? smalls[lj] : 0ull;
  const bool is_goal_lane = lj >= 1 && lj <= p.G;
  const int gxy = is_goal_lane ? static_cast<int>(reinterpret_cast<const uint16_t*>(h->goal)[lj - 1]) : -1;
  const LaneSlot s0 = lane_slot(xy, ot, small);
  const int lj1 = lj + GS;  // second slot (kTwo)
  const bool has1 = kTwo && lj1 < N;
  const int xy1 = has1 ? static_cast<int>(srow[lj1]) : 0;
  const uint32_t ot1 = has1 ? reinterpret_cast<const uint32_t*>(h->objtab)[lj1] : 0u;
  const uint64_t small1 = has1 ? smalls[lj1] : 0ull;
  const bool is_goal_lane1 = kTwo && lj1 <= p.G;
  const int gxy1 = is_goal_lane1 ? static_cast<int>(reinterpret_cast<const uint16_t*>(h->goal)[lj1 - 1]) : -1;
  const LaneSlot s1 = lane_slot(xy1, ot1, small1);

  const uint32_t agent_blocked = group_agent_blocked4<GS>(p, xy, ot, small, lj, gbase, gmask, live);
  // the agent's sweep, once for the four actions (agent_pushes4)
  const LaneObj ag = lane_obj(static_cast<uint32_t>(__shfl(static_cast<int>(ot), gbase, PW_WAVE)), __shfl(xy, gbase, PW_WAVE));
  const uint64_t asmall = __shfl(static_cast<unsigned long long>(small), gbase, PW_WAVE);
  const uint32_t hit4_0 = agent_pushes4(p, ag, asmall, s0, lj, live && lj >= 1 && lj < N);
  const uint32_t hit4_1 = kTwo ? agent_pushes4(p, ag, asmall, s1, lj1, live && has1) : 0u;
  // The way back: a parent that was reached by the agent moving ALONE (bit 2 of its action byte) has, under the opposite
  // action with again nothing but the agent moving, exactly its own parent as the successor -- a visited state by
  // construction.  That candidate is dropped here (like one that did not move): a quarter of the closed-set probes, the
  // search's dominant traffic, for most parents.
  const uint32_t came = a.action[pidx];
#pragma unroll 1
  for (int act = 0; act < 4; act++) {
    const int dx = act == 0 ? -1 : (act == 1 ? 1 : 0);
    const int dy = act == 2 ? -1 : (act == 3 ? 1 : 0);
    const uint32_t pushed = group_push_closure_swept<GS, kTwo>(p, s0, s1, hit4_0, hit4_1, lj, gbase, gmask, live,
                                                               ((agent_blocked >> act) & 1u) != 0u, act, dx, dy);
    const bool way_back = (came & 0x84u) == 4u && (came & 3u) == static_cast<uint32_t>(act ^ 1) && pushed == 1u;  // (the root: 0xFF)
    const bool moved = pushed != 0u && !way_back;
    int nxy = xy, nxy1 = xy1;
    if (moved && ((pushed >> lj) & 1u)) {
      const int x = static_cast<int8_t>(xy & 0xff) + dx, y = static_cast<int8_t>((xy >> 8) & 0xff) + dy;
      nxy = (x & 0xff) | ((y & 0xff) << 8);
    }
    if (kTwo && moved && ((pushed >> lj1) & 1u)) {
      const int x = static_cast<int8_t>(xy1 & 0xff) + dx, y = static_cast<int8_t>((xy1 >> 8) & 0xff) + dy;
      nxy1 = (x & 0xff) | ((y & 0xff) << 8);
    }
    int after = __popcll(__ballot(is_goal_lane && nxy == gxy) & gmask);
    if (kTwo && __ballot(is_goal_lane1) != 0ull) after += __popcll(__ballot(is_goal_lane1 && nxy1 == gxy1) & gmask);
    // the hash sums one term per SLOT (2 GS of them with kTwo: the same value the 2 GS-lane kernel and the host compute)
    uint32_t t = search_lane_term(static_cast<uint32_t>(nxy), static_cast<uint32_t>(lj));
    if (kTwo) t += search_lane_term(static_cast<uint32_t>(nxy1), static_cast<uint32_t>(lj1));
#pragma unroll
    for (int o = GS / 2; o > 0; o >>= 1) t += static_cast<uint32_t>(__shfl_xor(static_cast<int>(t), o, GS));
    t = search_final(t);
    const int hi = __shfl_down(nxy, 1, PW_WAVE);
    const int64_t c = static_cast<int64_t>(g) * 4 + ((slot_of >> (2 * act)) & 3u);
    if (g < a.nparents && lj == 0) {
      a.cand_hash[c] = moved ? (t & a.mask) : PW_S_NONE;
      a.cand_goal[c] = static_cast<uint8_t>(((moved && after == p.G) ? 1 : 0) | (pushed == 1u ? 2 : 0));  // bit 1: the agent alone
      if (a.cand_moved) a.cand_moved[c] = moved ? pushed : 0u;
    }
    if (moved && !(lj & 1) && lj < 2 * a.nw)
      a.cand_state[c * a.nw + (lj >> 1)] = static_cast<uint32_t>(nxy) | (static_cast<uint32_t>(hi) << 16);
    if (kTwo) {
      const int hi1 = __shfl_down(nxy1, 1, PW_WAVE);
      if (moved && !(lj & 1) && lj1 < 2 * a.nw)
        a.cand_state[c * a.nw + (lj1 >> 1)] = static_cast<uint32_t>(nxy1) | (static_cast<uint32_t>(hi1) << 16);
    }
  }
}

// ---- expand, one LANE per parent (puzzles with push tables; passes of >= 131 072 parents) ----------------------------
// The formulation of pw_expand4_lane_kernel (csrc/pw_expand_kernels.inc: push tables, one work list over the four actions,
// parents in and candidates out through LDS) on the search's packed states: a state is already the (x, y) byte pairs the
// push tests take, a successor is the parent's words with the moved halves displaced.  Same candidate records as
// pw_search_expand_kernel (hash over `slots` = 8 / 16 / 32 slots: hash_pad = the terms of the empty slots N .. slots - 1), except
// that the words of candidates that did not move are written too (the parent's; nobody reads them).
// per_pass: actions staged at a time (runs of per_pass * nw words leave together, width words per store).
template <int NP>
__global__ __launch_bounds__(64) void pw_search_expand_lane_kernel(SearchArgs a, uint32_t hash_pad, int per_pass, int width) {
  extern __shared__ int s_rows[];  // [64][per_pass nw + 2] candidates (first the parents, [64][nw | 1]), then [64][NP / 2 + 1] positions
  const PwPuzzleHeader* h = a.hdrs + a.puzzle;
  const int N = h->N, G = h->G, nw = a.nw;
  const PwPushDir dir = a.push_dir[a.puzzle];
  const uint32_t* pair = reinterpret_cast<const uint32_t*>(a.ovl + dir.pair_off);
  const uint32_t* wtab = reinterpret_cast<const uint32_t*>(a.ovl + dir.wall_off);
  const int lane = threadIdx.x;
  const int64_t first = static_cast<int64_t>(blockIdx.x) * 64;
  const int nlive = static_cast<int>(min(static_cast<int64_t>(64), a.nparents - first));
  const bool live = lane < nlive;
  const int run = per_pass * nw, in_stride = nw | 1, out_stride = run | 1, out_len = 4 * nw;
  uint32_t* s_words = reinterpret_cast<uint32_t*>(s_rows);
  uint32_t* s_xy = s_words + 64 * (run + 2) + lane * (NP / 2 + 1);
  const uint32_t magic_nw = 0xFFFFFFFFu / static_cast<uint32_t>(nw) + 1u;
  const uint32_t magic_run = 0xFFFFFFFFu / static_cast<uint32_t>(run) + 1u;
  {
    const uint32_t* src = a.states + (a.first + first) * nw;
    const int total = nlive * nw;
    uint32_t tmp[NP / 2];
#pragma unroll
    for (int k = 0; k < NP / 2; k++) {
      const int e = lane + 64 * k;
      tmp[k] = (k < nw && e < total) ? src[e] : 0u;
    }
#pragma unroll
    for (int k = 0; k < NP / 2; k++) {
      const int e = lane + 64 * k;
      if (k < nw && e < total) {
        const int st = pw_small_div(e, nw, magic_nw);
        s_words[st * in_stride + (e - st * nw)] = tmp[k];
      }
    }
  }
  __syncthreads();
  uint32_t XY[NP / 2], GW[NP / 2], GSEL[NP / 2];
#pragma unroll
  for (int k = 0; k < NP / 2; k++) {
    XY[k] = (k < nw && live) ? s_words[lane * in_stride + k] : 0u;
    s_xy[k] = XY[k];
    const int j0 = 2 * k, j1 = 2 * k + 1;  // goal k is the target of movable k + 1
    const uint32_t g0 = (j0 >= 1 && j0 <= G) ? reinterpret_cast<const uint16_t*>(h->goal)[j0 - 1] : 0u;
    const uint32_t g1 = (j1 <= G) ? reinterpret_cast<const uint16_t*>(h->goal)[j1 - 1] : 0u;
    GW[k] = g0 | (g1 << 16);
    GSEL[k] = ((j0 >= 1 && j0 <= G) ? 0xffffu : 0u) | ((j1 <= G) ? 0xffff0000u : 0u);
  }
  __syncthreads();  // every lane has its words: the buffer is free for the candidates
  // above the novelty width: closed, not expanded
  const bool expand = live && !(a.pruned && a.pruned[a.first + first + lane]);
  PwActMasks<NP> pushed;
  uint32_t stopped;
  lane_push_sets<NP>(h, pair, wtab, dir.R2, dir.RW, dir.Hs, dir.WW, N, XY, s_xy, expand, pushed, stopped);

  uint32_t hash4[4], moved4[4], goal4 = 0;
  const uint32_t came = live ? a.action[a.first + first + lane] : 0u;  // (the way back: see pw_search_expand_kernel)
  const int total = nlive * run;
#pragma unroll
  for (int act = 0; act < 4; act++) {
    const int dx = act == 0 ? -1 : (act == 1 ? 1 : 0);
    const int dy = act == 2 ? -1 : (act == 3 ? 1 : 0);
    const uint32_t m = ((stopped >> act) & 1u) ? 0u : pushed.get(act);
    const bool moved = m != 0u;
    const uint32_t addx = static_cast<uint32_t>(dx & 0xff) * 0x00010001u, addy = static_cast<uint32_t>((dy & 0xff) << 8) * 0x00010001u;
    const int slot = act & (per_pass - 1);
    if (act && slot == 0) __syncthreads();  // the previous pass's rows have left
    uint32_t* row = s_words + lane * out_stride + slot * nw;
    uint32_t t = hash_pad;
    bool on_goals = true;
#pragma unroll
    for (int k = 0; k < NP / 2; k++) {
      if (k < nw) {
        const uint32_t b = (m >> (2 * k)) & 3u;
        const uint32_t sel = ((b & 1u) ? 0xffffu : 0u) | ((b & 2u) ? 0xffff0000u : 0u);
        const uint32_t w = XY[k];
        // byte-wise x += dx, y += dy in the moved halves (no carry between bytes)
        const uint32_t nwv = (((w & 0x00ff00ffu) + (addx & sel)) & 0x00ff00ffu) | (((w & 0xff00ff00u) + (addy & sel)) & 0xff00ff00u);
        row[k] = nwv;
        on_goals = on_goals && (((nwv ^ GW[k]) & GSEL[k]) == 0u);
        // (slots 2 k and 2 k + 1; a slot beyond N holds 0 and is part of hash_pad ... unless it is inside the last word)
        t += search_lane_term(nwv & 0xffffu, static_cast<uint32_t>(2 * k));
        if (2 * k + 1 < N) t += search_lane_term(nwv >> 16, static_cast<uint32_t>(2 * k + 1));
      }
    }
    const bool way_back = (came & 0x84u) == 4u && (came & 3u) == static_cast<uint32_t>(act ^ 1) && m == 1u;
    hash4[act] = (moved && !way_back) ? (search_final(t) & a.mask) : PW_S_NONE;
    moved4[act] = way_back ? 0u : m;
    if (moved && on_goals) goal4 |= 1u << (8 * act);
    if (m == 1u) goal4 |= 2u << (8 * act);  // bit 1: the agent alone
    if (slot != per_pass - 1) continue;
    __syncthreads();
    uint32_t* dst = a.cand_state + first * out_len + (act - slot) * nw;
    if (width == 4) {
      for (int e = 4 * lane; e < total; e += 256) {
        const int st = pw_small_div(e, run, magic_run);
        const int j = e - st * run;
        const uint32_t* src = s_words + st * out_stride + j;
        *reinterpret_cast<uint4*>(dst + st * out_len + j) = make_uint4(src[0], src[1], src[2], src[3]);
      }
    } else if (width == 2) {
      for (int e = 2 * lane; e < total; e += 128) {
        const int st = pw_small_div(e, run, magic_run);
        const int j = e - st * run;
        const uint32_t* src = s_words + st * out_stride + j;
        *reinterpret_cast<uint2*>(dst + st * out_len + j) = make_uint2(src[0], src[1]);
      }
    } else {
      for (int e = lane; e < total; e += 64) {
        const int st = pw_small_div(e, run, magic_run);
        const int j = e - st * run;
        dst[st * out_len + j] = s_words[st * out_stride + j];
      }
    }
  }
  if (live) {  // (the candidate arrays come from hipMalloc and a block starts at a multiple of 256 candidates: aligned)
    reinterpret_cast<uint4*>(a.cand_hash)[first + lane] = make_uint4(hash4[0], hash4[1], hash4[2], hash4[3]);
    reinterpret_cast<uint32_t*>(a.cand_goal)[first + lane] = goal4;
    if (a.pruned) reinterpret_cast<uint4*>(a.cand_moved)[first + lane] = make_uint4(moved4[0], moved4[1], moved4[2], moved4[3]);
  }
}

// ---- claim: visited-set lookup + tentative insertion ------------------------------------------------
// cand_slot[c] on return: PW_S_NONE = not the owner of a new state (did not move, visited, or a lower candidate id of this pass
// holds the state); else the slot, and the candidate owns the state unless cand_lost[c] == epoch (a lower id came later).
// Entries, kKey false: fingerprint << 32 | (index + 1 published | PW_S_TENT | candidate tentative); kKey true: the packed state
// itself published | PW_S_TENT64 | candidate tentative.  A tentative entry is smaller the lower its candidate id and a
// published one smaller than any of them: atomicMin lets the first discovery in (parent, action) order own the state.
template <bool kKey>
__global__ __launch_bounds__(256) void pw_search_claim_kernel(SearchArgs a, int n) {
  if (a.halt && *a.halt) return;
  const int64_t c = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  // Rediscoveries inside the workgroup first (its 256 candidates are the successors of 64 consecutive parents -- siblings and
  // cousins, which is where most states found twice in a pass are found): the lowest candidate id per hash in a small LDS table;
  // a candidate that finds a lower id there with the SAME state is done -- lost -- without touching the closed set.  What
  // bounds this kernel is the rate of memory-side atomics (profiles/r05_atomic_probe.txt: 18 G/s; the kernel ran at 14 G/s with
  // ~2.4 per parent, of which only the first CAS of a new state, 1.16 per parent, is needed): a rediscovery that arrives while
  // the first claim is still in flight costs a lost CAS and often an atomicMin.
  __shared__ uint32_t s_first[512];
  for (int i = threadIdx.x; i < 512; i += 256) s_first[i] = 0xFFFFFFFFu;
  __syncthreads();
  const bool in_range = c < a.ncand;
  const uint32_t h = in_range ? a.cand_hash[c] : PW_S_NONE;
  const uint32_t ls = (h ^ (h >> 9) ^ (h >> 18)) & 511u;
  if (h != PW_S_NONE) atomicMin(&s_first[ls], threadIdx.x);
  __syncthreads();
  if (!in_range) return;
  if (h == PW_S_NONE) {
    a.cand_slot[c] = PW_S_NONE;
    return;
  }
  const uint32_t* my = a.cand_state + c * a.nw;
  {
    const uint32_t first = s_first[ls];
    if (first < threadIdx.x) {
      const int64_t cf = c - threadIdx.x + first;
      bool same = a.cand_hash[cf] == h;
      const uint32_t* other = a.cand_state + cf * a.nw;
      for (int k = 0; k < a.nw; k++) same = same && my[k] == other[k];
      if (same) {
        a.cand_slot[c] = PW_S_NONE;
        return;
      }
    }
  }
  const uint32_t fp = kKey ? 0u : search_fingerprint(my, a.nw);
  const unsigned long long key = kKey ? search_key(my, n, a.key_bx, a.key_by) : 0ull;
  const unsigned long long claim = kKey ? (PW_S_TENT64 | static_cast<unsigned long long>(c))
                                        : ((static_cast<unsigned long long>(fp) << 32) | PW_S_TENT | static_cast<uint32_t>(c));
  uint32_t bucket = h & ~7u;
  for (;;) {
    // the whole 64-byte line in registers.  (Plain loads: what another XCD inserted during this launch may be missing from the
    // view -- entries only ever appear -- and the CAS below, which is not, has the last word on an empty slot.)
    unsigned long long e[8];
    {
      const uint4* line = reinterpret_cast<const uint4*>(a.table + bucket);
      const uint4 v0 = line[0], v1 = line[1], v2 = line[2], v3 = line[3];
      e[0] = v0.x | (static_cast<unsigned long long>(v0.y) << 32), e[1] = v0.z | (static_cast<unsigned long long>(v0.w) << 32);
      e[2] = v1.x | (static_cast<unsigned long long>(v1.y) << 32), e[3] = v1.z | (static_cast<unsigned long long>(v1.w) << 32);
      e[4] = v2.x | (static_cast<unsigned long long>(v2.y) << 32), e[5] = v2.z | (static_cast<unsigned long long>(v2.w) << 32);
      e[6] = v3.x | (static_cast<unsigned long long>(v3.y) << 32), e[7] = v3.z | (static_cast<unsigned long long>(v3.w) << 32);
    }
#pragma unroll
    for (int i = 0; i < 8; i++) {
      unsigned long long v = e[i];
      const uint32_t slot = bucket + static_cast<uint32_t>(i);
      if (v == 0ull) {
        v = atomicCAS(&a.table[slot], 0ull, claim);
        if (v == 0ull) {
          a.cand_slot[c] = slot;
          return;
        }
      }
      bool tentative, maybe;
      if (kKey) {
        if (v == key) {  // visited in an earlier layer / pass: recognised from the entry alone
          a.cand_slot[c] = PW_S_NONE;
          return;
        }
        tentative = (v & PW_S_TENT64) != 0ull;
        maybe = tentative;
      } else {
        tentative = (static_cast<uint32_t>(v) & PW_S_TENT) != 0u;
        maybe = static_cast<uint32_t>(v >> 32) == fp;
      }
      if (maybe) {  // only now the (random) read of the other state
        const uint32_t id = kKey ? static_cast<uint32_t>(v) : (static_cast<uint32_t>(v) & ~PW_S_TENT);
        const uint32_t* other = tentative ? a.cand_state + static_cast<int64_t>(id) * a.nw
                                          : a.states + static_cast<int64_t>(static_cast<uint32_t>(v) - 1u) * a.nw;
        bool eq = true;
        for (int k = 0; k < a.nw; k++) eq = eq && my[k] == other[k];
        if (eq) {
          uint32_t mine_slot = PW_S_NONE;  // visited, or a lower id of this pass holds it
          if (tentative && v > claim) {  // (a lower id already in place: lost without touching the entry)
            const unsigned long long old = atomicMin(&a.table[slot], claim);
            if (old > claim) {
              a.cand_lost[kKey ? static_cast<uint32_t>(old) : (static_cast<uint32_t>(old) & ~PW_S_TENT)] = a.epoch;
              mine_slot = slot;
            }
          }
          a.cand_slot[c] = mine_slot;
          return;
        }
      }
    }
    bucket = (bucket + 8u) & a.mask;
  }
}

__device__ __forceinline__ bool search_owner(const SearchArgs& a, int64_t c) {
  if (c >= a.ncand) return false;
  return a.cand_slot[c] != PW_S_NONE && a.cand_lost[c] != a.epoch;
}

// ---- novelty of the owners (width-limited search): 32 lanes per candidate, ids in candidate order ------
template <bool kMark>
__global__ __launch_bounds__(256) void pw_search_novelty_kernel(SearchArgs a) {
  if (a.halt && *a.halt) return;
  const int lane = threadIdx.x & (PW_WAVE - 1);
  const int lj = threadIdx.x & 31;
  const int gbase = lane & ~31;
  const unsigned long long gmask = 0xFFFFFFFFull << gbase;
  const int64_t c = static_cast<int64_t>(blockIdx.x) * 8 + threadIdx.x / 32;
  const bool active = search_owner(a, c);
  int pj = 0;
  if (active && lj < a.nt.N) {
    const uint32_t xy = reinterpret_cast<const uint16_t*>(a.cand_state + c * a.nw)[lj];
    pj = static_cast<int>(xy >> 8) * a.nt.W + static_cast<int>(xy & 0xffu);
  }
  const uint32_t moved = active ? a.cand_moved[c] : 0u;
  const int nov = novelty_group<kMark>(a.nt, lj, gbase, gmask, active, pj, moved, a.id_base + static_cast<uint32_t>(c));
  if (!kMark && active && lj == 0) a.cand_nov[c] = static_cast<uint8_t>(nov);
}

// the start state enters the novelty tables with every object marked as moved (best_first_search.h:58-67)
__global__ __launch_bounds__(64) void pw_search_root_novelty_kernel(SearchArgs a) {
  const int lj = threadIdx.x & 31;
  const bool active = threadIdx.x < 32;
  int pj = 0;
  if (active && lj < a.nt.N) {
    const uint32_t xy = reinterpret_cast<const uint16_t*>(a.states)[lj];
    pj = static_cast<int>(xy >> 8) * a.nt.W + static_cast<int>(xy & 0xffu);
  }
  const uint32_t all = a.nt.N >= 32 ? 0xFFFFFFFFu : ((1u << a.nt.N) - 1u);
  novelty_group<true>(a.nt, lj, 0, 0xFFFFFFFFull, active, pj, all, 0u);
  if (threadIdx.x == 0 && a.pruned) a.pruned[0] = 0;
}

// ---- count: owners per block of 256 candidates -------------------------------------------------------
__global__ __launch_bounds__(256) void pw_search_count_kernel(SearchArgs a) {
  if (a.halt && *a.halt) return;
  __shared__ uint32_t wsum[4];
  const int64_t c = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  const unsigned long long m = __ballot(search_owner(a, c));
  if ((threadIdx.x & 63) == 0) {
    wsum[threadIdx.x >> 6] = static_cast<uint32_t>(__popcll(m));
    a.owner[static_cast<int64_t>(blockIdx.x) * 4 + (threadIdx.x >> 6)] = m;  // publish reads these, not the table
  }
  __syncthreads();
  if (threadIdx.x == 0) a.block_off[blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// ---- scan: block counts -> first store index of each block (single workgroup) ----------------------
__global__ __launch_bounds__(1024) void pw_search_scan_kernel(SearchArgs a, int32_t nblocks) {
  if (a.halt && *a.halt) return;
  __shared__ uint32_t part[1024];
  const int tid = threadIdx.x;
  const int per = (nblocks + 1023) / 1024;
  const int lo = min(tid * per, nblocks), hi = min(lo + per, nblocks);
  uint32_t s = 0;
  for (int i = lo; i < hi; i++) s += a.block_off[i];
  part[tid] = s;
  __syncthreads();
  for (int o = 1; o < 1024; o <<= 1) {  // Hillis-Steele inclusive scan of the 1024 partial sums
    const uint32_t v = tid >= o ? part[tid - o] : 0u;
    __syncthreads();
    part[tid] += v;
    __syncthreads();
  }
  const unsigned long long base = a.info[0];
  uint32_t run = static_cast<uint32_t>(base) + (tid ? part[tid - 1] : 0u);
  for (int i = lo; i < hi; i++) {
    const uint32_t n = a.block_off[i];
    a.block_off[i] = run;
    run += n;
  }
  if (tid == 1023) {
    const unsigned long long total = base + part[1023];
    if (total > static_cast<unsigned long long>(a.max_states)) {
      a.info[2] = 1ull;
      a.info[0] = static_cast<unsigned long long>(a.max_states);
    } else {
      a.info[0] = total;
    }
  }
}

// ---- publish: owners -> store, table entry becomes permanent ----------------------------------------
__global__ __launch_bounds__(256) void pw_search_publish_kernel(SearchArgs a, int n) {
  if (a.halt && *a.halt) return;
  __shared__ uint32_t wsum[4];
  const int64_t c = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long m = a.owner[static_cast<int64_t>(blockIdx.x) * 4 + w];  // the count kernel's ballots
  const bool own = ((m >> lane) & 1ull) != 0ull;
  if (lane == 0) wsum[w] = static_cast<uint32_t>(__popcll(m));
  __syncthreads();
  if (!own) return;
  uint32_t rank = static_cast<uint32_t>(__popcll(m & ((1ull << lane) - 1ull)));
  for (int k = 0; k < w; k++) rank += wsum[k];
  const int64_t idx = static_cast<int64_t>(a.block_off[blockIdx.x]) + rank;
  if (idx >= a.max_states) return;  // store full: the overflow flag is already set by the scan
  const uint32_t* src = a.cand_state + c * a.nw;
  uint32_t* dst = a.states + idx * a.nw;
  for (int k = 0; k < a.nw; k++) dst[k] = src[k];
  a.parent[idx] = a.plist ? a.plist[c >> 2] : static_cast<int32_t>(a.first + (c >> 2));
  const uint32_t cg = a.cand_goal[c];
  const uint32_t act = a.pperm ? (static_cast<uint32_t>(a.pperm[c >> 2]) >> (2 * (c & 3))) & 3u : static_cast<uint32_t>(c & 3);
  a.action[idx] = static_cast<uint8_t>(act | ((cg & 2u) << 1));  // bit 2: reached by the agent moving alone
  // the entry becomes (fingerprint, index + 1) -- the low word; the fingerprint stays -- or, with exact keys, the state itself
  if (a.key_bx == 0) reinterpret_cast<uint32_t*>(a.table + a.cand_slot[c])[0] = static_cast<uint32_t>(idx) + 1u;
  else a.table[a.cand_slot[c]] = search_key(src, n, a.key_bx, a.key_by);
  if (a.pruned) a.pruned[idx] = a.cand_nov[c] > a.width ? 1 : 0;
  if (a.state_nov) a.state_nov[idx] = a.cand_nov[c];
  if (cg & 1u) atomicMin(&a.info[1], static_cast<unsigned long long>(idx));
}

// ---- read-out ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pw_search_unpack_kernel(const uint32_t* states, int nw, int n, int64_t first,
                                                               int64_t count, int32_t* out) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= count * n) return;
  const int64_t s = i / n;
  const int j = static_cast<int>(i - s * n);
  const uint32_t xy = reinterpret_cast<const uint16_t*>(states + (first + s) * nw)[j];
  out[i] = static_cast<int32_t>(xy & 0xffu) * PW_POSITION_LIMIT + static_cast<int32_t>(xy >> 8);
}

// the action bytes as the API hands them out: 0 .. 3, 0xFF for the start state (bit 2 is the search's own: see publish)
__global__ __launch_bounds__(256) void pw_search_actions_kernel(const uint8_t* src, int64_t count, uint8_t* out) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i < count) out[i] = src[i] == 0xFFu ? 0xFFu : (src[i] & 3u);
}

__global__ void pw_search_plan_kernel(const int32_t* parent, const uint8_t* action, int64_t index, uint8_t* out,
                                      int32_t cap, int32_t* len) {
  int n = 0;
  int64_t i = index;
  while (i > 0) {
    if (n < cap) out[n] = action[i] & 3;
    n++;
    i = parent[i];
  }
  *len = n;  // actions from the goal back to the start
}

extern "C" {

void pw_search_destroy(PwSearch* s) {
  if (!s) return;
  void* bufs[] = {s->d_states, s->d_parent, s->d_action, s->d_table, s->d_owner, s->d_cand_state, s->d_cand_hash,
                  s->d_cand_slot, s->d_cand_goal, s->d_block_off, s->d_info, s->d_plan, s->d_pruned, s->d_cand_lost,
                  s->d_cand_moved, s->d_cand_nov};
  for (void* b : bufs)
    if (b) (void)hipFree(b);
  search_table_discard(s);
  pw_novelty_destroy(s->nov);
  delete s;
}

}  // extern "C"

// chunk > 0: parents per pass (the planner: its batch K); 0: PW_OPT_SEARCH_CHUNK or 2^20
static int search_create(PwEngine* e, int32_t puzzle, int64_t max_states, int32_t novelty_width, int64_t chunk_parents,
                         PwSearch** out) {
  if (!e || !out) return pw_fail(PW_EINVAL, "null argument");
  if (novelty_width < 0 || novelty_width > 2) return pw_fail(PW_EINVAL, "novelty_width must be 0 (off), 1 or 2");
  if (puzzle < 0 || puzzle >= e->set->count) return pw_fail(PW_EINVAL, "puzzle index out of range");
  if (max_states < 1 || max_states > (1ll << 30)) return pw_fail(PW_EINVAL, "max_states must be in 1 .. 2^30");
  PwSearch* s = new (std::nothrow) PwSearch();
  if (!s) return pw_fail(PW_ENOMEM, "out of memory");
  std::memset(static_cast<void*>(s), 0, sizeof(*s));
  const PwPuzzleHeader& h = e->set->headers[puzzle];
  s->eng = e;
  s->puzzle = puzzle;
  s->N = h.N;
  s->G = h.G;
  s->NW = (h.N + 1) / 2;
  s->gs = h.N <= 8 ? 8 : (h.N <= 16 ? 16 : 32);
  s->max_states = max_states;
  s->width = novelty_width;
  const int64_t chunk = e->search_chunk > 0 ? e->search_chunk : (1 << 20);  // PW_OPT_SEARCH_CHUNK (tests: many passes per layer)
  s->chunk = chunk_parents > 0 ? static_cast<int32_t>(chunk_parents)
                               : static_cast<int32_t>(std::min<int64_t>(chunk, std::max<int64_t>(max_states, 1)));
  const uint64_t slots = std::max<uint64_t>(1024, pw_table_slots(static_cast<uint64_t>(max_states) + 4ull * s->chunk));
  if (slots > (1ull << 31)) {
    delete s;
    return pw_fail(PW_ELIMIT, "visited table would exceed 2^31 slots");
  }
  s->table_slots = static_cast<uint32_t>(slots);
  s->plan_cap = 1 << 16;
  const int64_t ncand = 4ll * s->chunk;
  PwDeviceGuard guard(e->set->device);
  PwHipChain c(guard.status());
  c.alloc(&s->d_states, static_cast<size_t>(max_states) * s->NW * 4);
  c.alloc(&s->d_parent, static_cast<size_t>(max_states) * 4);
  c.alloc(&s->d_action, static_cast<size_t>(max_states));
  // exact keys (PW_OPT_SEARCH_KEYS 1) when the state packs into 63 bits (the start state decides in pw_search_begin whether they
  // are used: it must not overlap a wall)
  {
    int bx = 1, by = 1;
    while ((1 << bx) < h.W) bx++;
    while ((1 << by) < h.H) by++;
    const bool fits = h.N * (bx + by) <= 63 && e->search_keys == 1;
    s->key_bx = fits ? bx : 0;
    s->key_by = fits ? by : 0;
  }
  c.alloc(&s->d_table, static_cast<size_t>(slots) * 8);
  c.alloc(&s->d_cand_lost, static_cast<size_t>(ncand) * 4);
  c.alloc(&s->d_owner, static_cast<size_t>(ncand / 64 + 8) * 8);
  c.alloc(&s->d_cand_state, static_cast<size_t>(ncand) * s->NW * 4);
  c.alloc(&s->d_cand_hash, static_cast<size_t>(ncand) * 4);
  c.alloc(&s->d_cand_slot, static_cast<size_t>(ncand) * 4);
  c.alloc(&s->d_cand_goal, static_cast<size_t>(ncand));
  c.alloc(&s->d_block_off, static_cast<size_t>(ncand / 256 + 2) * 4);
  c.alloc(&s->d_info, 4 * sizeof(unsigned long long));
  c.alloc(&s->d_plan, static_cast<size_t>(s->plan_cap) + 16);
  if (novelty_width > 0) {
    c.alloc(&s->d_pruned, static_cast<size_t>(max_states));
    c.alloc(&s->d_cand_moved, static_cast<size_t>(ncand) * 4);
    c.alloc(&s->d_cand_nov, static_cast<size_t>(ncand));
  }
  if (!c.ok()) {
    pw_search_destroy(s);
    return pw_hip_fail("pw_search_create", c.err);
  }
  if (novelty_width > 0) {
    if (int rc = novelty_alloc(e->set->device, h.N, h.W, h.H, &s->nov)) {
      pw_search_destroy(s);
      return rc;
    }
  }
  *out = s;
  return PW_OK;
}

extern "C" int pw_search_create(PwEngine* e, int32_t puzzle, int64_t max_states, int32_t novelty_width, PwSearch** out) try {
  return search_create(e, puzzle, max_states, novelty_width, 0, out);
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}


static constexpr int64_t kSearchLaneParents = 131072;  // passes from this many parents on run one lane per parent

static SearchArgs search_args(PwSearch* s) {
  SearchArgs a;
  a.hdrs = s->eng->set->d_headers;
  a.blob = s->eng->set->d_blob;
  a.ovl = s->eng->d_ovl;
  a.ovl_dir = s->eng->d_ovl_dir;
  a.push_dir = s->eng->d_push_dir;
  a.puzzle = s->puzzle;
  a.nw = s->NW;
  a.states = s->d_states;
  a.parent = s->d_parent;
  a.action = s->d_action;
  a.table = s->d_table;
  a.owner = s->d_owner;
  a.cand_lost = s->d_cand_lost;
  a.epoch = s->epoch;
  a.key_bx = s->use_keys ? s->key_bx : 0;
  a.key_by = s->use_keys ? s->key_by : 0;
  a.mask = s->table_slots - 1u;
  a.cand_state = s->d_cand_state;
  a.cand_hash = s->d_cand_hash;
  a.cand_slot = s->d_cand_slot;
  a.cand_goal = s->d_cand_goal;
  a.block_off = s->d_block_off;
  a.info = s->d_info;
  a.first = 0;
  a.nparents = 0;
  a.ncand = 0;
  a.max_states = s->max_states;
  a.pruned = s->width > 0 ? s->d_pruned : nullptr;
  a.cand_moved = s->d_cand_moved;
  a.cand_nov = s->d_cand_nov;
  a.width = s->width;
  a.id_base = 0;
  if (s->nov) a.nt = s->nov->t;
  else std::memset(&a.nt, 0, sizeof(a.nt));
  a.plist = nullptr;
  a.pperm = nullptr;
  a.halt = nullptr;
  a.state_nov = nullptr;
  return a;
}

// lane_ok false keeps the lane-group expand kernels (the planner's parent lists and action groups are theirs only).
// The expand launch of a pass (the cost-to-go table's successor pass, csrc/pw_solution.inc, runs it too).  Returns true when
// it was the one-lane-per-parent kernel.
static bool search_launch_expand(PwSearch* s, SearchArgs& a, hipStream_t st, bool lane_ok) {
  const bool tab = !s->eng->ovl_has.empty() && s->eng->ovl_has[static_cast<size_t>(s->puzzle)];  // overlap tables
  // One lane per parent (pw_search_expand_lane_kernel) for passes that fill the chip by themselves: puzzles with push
  // tables; PW_OPT_STEP_KERNEL lane forces it, PW_OPT_STEP_LANE_BATCH moves the threshold.
  const bool push_tab = !s->eng->push_has.empty() && s->eng->push_has[static_cast<size_t>(s->puzzle)];
  const int64_t lane_from = s->eng->step_lane_batch == 0 ? kSearchLaneParents : s->eng->step_lane_batch;
  if (lane_ok && push_tab && s->N <= 32 && (s->eng->step_kernel == 2 || (s->eng->step_kernel == 0 && a.nparents >= lane_from))) {
    uint32_t hash_pad = 0;  // the hash sums one term per slot of the lane-group kernels (8 or 16), empty ones included
    for (int j = s->N; j < s->gs; j++) hash_pad += search_lane_term(0u, static_cast<uint32_t>(j));
    const int nw = s->NW;
    // runs of per_pass * nw words, 16-byte stores when that is a multiple of 4 (nw: 1 .. 8)
    const int per_pass = nw % 4 == 0 ? 1 : (nw % 2 == 0 ? 2 : 4);
    const int width = 4;
    const int np_lane = s->N <= 4 ? 4 : (s->N <= 8 ? 8 : (s->N <= 16 ? 16 : 32));  // positions in LDS: NP / 2 + 1 words per state
    const size_t lds = static_cast<size_t>(64) * (per_pass * nw + 2 + np_lane / 2 + 1) * sizeof(int);
    const dim3 grid(static_cast<unsigned>((a.nparents + 63) / 64)), wave(64);
    if (s->N <= 4) hipLaunchKernelGGL(pw_search_expand_lane_kernel<4>, grid, wave, lds, st, a, hash_pad, per_pass, width);
    else if (s->N <= 8) hipLaunchKernelGGL(pw_search_expand_lane_kernel<8>, grid, wave, lds, st, a, hash_pad, per_pass, width);
    else if (s->N <= 16) hipLaunchKernelGGL(pw_search_expand_lane_kernel<16>, grid, wave, lds, st, a, hash_pad, per_pass, width);
    else hipLaunchKernelGGL(pw_search_expand_lane_kernel<32>, grid, wave, lds, st, a, hash_pad, per_pass, width);
    return true;
  } else if (s->gs == 8) {
    if (tab) hipLaunchKernelGGL((pw_search_expand_kernel<8, true>), dim3((a.nparents + 31) / 32), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((pw_search_expand_kernel<8, false>), dim3((a.nparents + 31) / 32), dim3(256), 0, st, a);
  } else if (s->gs == 16 && !s->eng->step_wide_groups) {  // 9 .. 16 movables: 8-lane groups, two movables per lane
    if (tab) hipLaunchKernelGGL((pw_search_expand_kernel<8, true, true>), dim3((a.nparents + 31) / 32), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((pw_search_expand_kernel<8, false, true>), dim3((a.nparents + 31) / 32), dim3(256), 0, st, a);
  } else if (s->gs == 16) {
    if (tab) hipLaunchKernelGGL((pw_search_expand_kernel<16, true>), dim3((a.nparents + 15) / 16), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((pw_search_expand_kernel<16, false>), dim3((a.nparents + 15) / 16), dim3(256), 0, st, a);
  } else {
    if (tab) hipLaunchKernelGGL((pw_search_expand_kernel<32, true>), dim3((a.nparents + 7) / 8), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((pw_search_expand_kernel<32, false>), dim3((a.nparents + 7) / 8), dim3(256), 0, st, a);
  }
  return false;
}

// One pass over a.nparents parents: expand, claim, (novelty), count, scan, publish.
static void search_pass(PwSearch* s, SearchArgs& a, hipStream_t st, bool lane_ok) {
  const unsigned cblocks = static_cast<unsigned>((a.ncand + 255) / 256);
  (void)search_launch_expand(s, a, st, lane_ok);
  if (a.key_bx) hipLaunchKernelGGL(pw_search_claim_kernel<true>, dim3(cblocks), dim3(256), 0, st, a, s->N);
  else hipLaunchKernelGGL(pw_search_claim_kernel<false>, dim3(cblocks), dim3(256), 0, st, a, s->N);
  if (s->nov) {  // width-limited search, or the planner's N+RGD mode
    a.id_base = s->nov->next_id;
    s->nov->next_id += static_cast<uint32_t>(a.ncand);
    const unsigned nblocks = static_cast<unsigned>((a.ncand + 7) / 8);
    hipLaunchKernelGGL(pw_search_novelty_kernel<true>, dim3(nblocks), dim3(256), 0, st, a);
    hipLaunchKernelGGL(pw_search_novelty_kernel<false>, dim3(nblocks), dim3(256), 0, st, a);
  }
  hipLaunchKernelGGL(pw_search_count_kernel, dim3(cblocks), dim3(256), 0, st, a);
  hipLaunchKernelGGL(pw_search_scan_kernel, dim3(1), dim3(1024), 0, st, a, static_cast<int32_t>(cblocks));
  hipLaunchKernelGGL(pw_search_publish_kernel, dim3(cblocks), dim3(256), 0, st, a, s->N);
}

extern "C" {

int pw_search_begin(PwSearch* s, const int32_t* start, void* stream) try {
  if (!s) return pw_fail(PW_EINVAL, "null search");
  PwDeviceGuard guard(s->eng->set->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  search_table_discard(s);  // a cost-to-go table belongs to the search it was computed from
  s->exhausted = false;
  const PwPuzzleHeader& h = s->eng->set->headers[s->puzzle];
  alignas(8) uint16_t packed[PW_MAX_OBJECTS + 2] = {0};
  bool goal = true;
  for (int j = 0; j < s->N; j++) {
    int x, y;
    if (start) {
      x = start[j] / PW_POSITION_LIMIT;
      y = start[j] % PW_POSITION_LIMIT;
      if (start[j] < 0 || x >= h.W || y >= h.H) return pw_fail(PW_EINVAL, "start state outside the puzzle");
    } else {
      x = h.init[j][0];
      y = h.init[j][1];
    }
    packed[j] = static_cast<uint16_t>((x & 0xff) | ((y & 0xff) << 8));
    if (j >= 1 && j <= s->G && (x != h.goal[j - 1][0] || y != h.goal[j - 1][1])) goal = false;
  }
  uint32_t t = 0;
  for (int lj = 0; lj < s->gs; lj++) t += search_lane_term(lj < s->N ? packed[lj] : 0u, static_cast<uint32_t>(lj));
  const uint32_t root_slot = search_final(t) & (s->table_slots - 1u);
  // Exact keys need every coordinate in 0 .. 2^bits - 1 for the whole search: a movable that overlaps no wall can never enter
  // one (puzzle.py:522-564), the border ring is all wall, so a start state without overlaps stays inside the grid for good.
  s->use_keys = s->key_bx != 0;
  if (s->use_keys) {
    const uint8_t* blob = s->eng->set->blob.data() + h.base;
    const uint64_t* wall = reinterpret_cast<const uint64_t*>(blob + h.off_wall);
    const uint64_t* awall = reinterpret_cast<const uint64_t*>(blob + h.off_awall);
    const uint64_t* shapes = reinterpret_cast<const uint64_t*>(blob + h.off_shapes);
    for (int j = 0; j < s->N && s->use_keys; j++) {
      const int x = packed[j] & 0xff, y = packed[j] >> 8;
      if (x + h.objtab[j].w > h.W || y + h.objtab[j].h > h.H) s->use_keys = false;
      for (int r = 0; r < h.objtab[j].h && s->use_keys; r++)
        if ((shapes[h.objtab[j].row_off + r] << x) & (j == 0 ? awall : wall)[y + r]) s->use_keys = false;
    }
  }
  // published state 0: under its fingerprint, or as its key; in the first free slot of its 64-byte line (= the first)
  const unsigned long long root_entry =
      s->use_keys ? search_key(reinterpret_cast<const uint32_t*>(packed), s->N, s->key_bx, s->key_by)
                  : ((static_cast<unsigned long long>(search_fingerprint(reinterpret_cast<const uint32_t*>(packed), s->NW)) << 32) | 1ull);
  const unsigned long long info[4] = {1ull, ~0ull, 0ull, 0ull};
  const int32_t root_parent = -1;
  const uint8_t root_action = 0xFF;
  hipError_t err = hipMemsetAsync(s->d_table, 0, static_cast<size_t>(s->table_slots) * 8, st);
  if (err == hipSuccess) err = hipMemcpyAsync(s->d_table + (root_slot & ~7u), &root_entry, 8, hipMemcpyHostToDevice, st);
  if (err == hipSuccess) err = hipMemsetAsync(s->d_cand_lost, 0, static_cast<size_t>(4ll * s->chunk) * 4, st);
  s->epoch = 0;
  if (err == hipSuccess) err = hipMemcpyAsync(s->d_states, packed, static_cast<size_t>(s->NW) * 4, hipMemcpyHostToDevice, st);
  if (err == hipSuccess) err = hipMemcpyAsync(s->d_parent, &root_parent, 4, hipMemcpyHostToDevice, st);
  if (err == hipSuccess) err = hipMemcpyAsync(s->d_action, &root_action, 1, hipMemcpyHostToDevice, st);
  if (err == hipSuccess) err = hipMemcpyAsync(s->d_info, info, sizeof(info), hipMemcpyHostToDevice, st);
  if (err == hipSuccess) err = hipStreamSynchronize(st);  // the sources are stack variables
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string("pw_search_begin: ") + hipGetErrorString(err));
  if (s->width > 0) {
    if (int rc = pw_novelty_reset(s->nov, stream)) return rc;
    hipLaunchKernelGGL(pw_search_root_novelty_kernel, dim3(1), dim3(64), 0, st, search_args(s));
    if (int rc = check_launch("pw_search_begin")) return rc;
    s->nov->next_id = 1;
  }
  s->layer_begin = 0;
  s->layer_end = 1;
  s->depth = 0;
  s->goal_index = goal ? 0 : -1;
  s->begun = true;
  s->overflow = false;
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_search_expand(PwSearch* s, int64_t info_out[4], void* stream) try {
  if (!s || !info_out) return pw_fail(PW_EINVAL, "null argument");
  if (!s->begun) return pw_fail(PW_EINVAL, "pw_search_begin has not been called");
  if (s->overflow) return pw_fail(PW_ELIMIT, "the state store is full (max_states)");
  PwDeviceGuard guard(s->eng->set->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t nlayer = s->layer_end - s->layer_begin;
  // Novelty ids are checked for the WHOLE layer before anything is launched: failing between two passes would
  // leave the passes already published in the table with layer_begin / layer_end / depth not advanced.
  if (s->width > 0 && static_cast<uint64_t>(s->nov->next_id) + 4ull * static_cast<uint64_t>(nlayer) >= 0xFFFFFFFFull)
    return pw_fail(PW_ELIMIT, "novelty ids exhausted (2^32 candidates): the layer was not expanded");
  SearchArgs a = search_args(s);
  for (int64_t off = 0; off < nlayer; off += s->chunk) {
    a.first = s->layer_begin + off;
    a.nparents = static_cast<int32_t>(std::min<int64_t>(s->chunk, nlayer - off));
    a.ncand = 4 * a.nparents;
    a.epoch = ++s->epoch;  // (2^32 passes: a search of 2^30 states in passes of one parent each would not get there)
    search_pass(s, a, st, true);
  }
  if (int rc = check_launch("pw_search_expand")) return rc;
  unsigned long long info[4] = {0, 0, 0, 0};
  hipError_t err = hipMemcpyAsync(info, s->d_info, sizeof(info), hipMemcpyDeviceToHost, st);
  if (err == hipSuccess) err = hipStreamSynchronize(st);
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string("pw_search_expand: ") + hipGetErrorString(err));
  const int64_t total = static_cast<int64_t>(info[0]);
  s->layer_begin = s->layer_end;
  s->layer_end = total;
  s->depth += 1;
  if (s->goal_index < 0 && info[1] != ~0ull) s->goal_index = static_cast<int64_t>(info[1]);
  s->overflow = info[2] != 0ull;
  s->exhausted = !s->overflow && s->layer_end == s->layer_begin;
  info_out[0] = s->depth;
  info_out[1] = s->layer_end - s->layer_begin;
  info_out[2] = total;
  info_out[3] = s->goal_index;
  if (s->overflow) return pw_fail(PW_ELIMIT, "the state store is full (max_states): the last layer is incomplete");
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_search_read_states(PwSearch* s, int64_t first, int64_t count, int32_t* dst, void* stream) try {
  if (!s || !dst) return pw_fail(PW_EINVAL, "null argument");
  PwDeviceGuard guard(s->eng->set->device);
  if (first < 0 || count < 0 || first + count > s->layer_end) return pw_fail(PW_EINVAL, "state range out of bounds");
  if (count == 0) return PW_OK;
  const int64_t n = count * s->N;
  hipLaunchKernelGGL(pw_search_unpack_kernel, dim3(static_cast<unsigned>((n + 255) / 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), s->d_states, s->NW, s->N, first, count, dst);
  return check_launch("pw_search_read_states");
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_search_read_links(PwSearch* s, int64_t first, int64_t count, int32_t* parent, uint8_t* action, void* stream) try {
  if (!s) return pw_fail(PW_EINVAL, "null argument");
  PwDeviceGuard guard(s->eng->set->device);
  if (first < 0 || count < 0 || first + count > s->layer_end) return pw_fail(PW_EINVAL, "state range out of bounds");
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t err = hipSuccess;
  if (count && parent) err = hipMemcpyAsync(parent, s->d_parent + first, static_cast<size_t>(count) * 4, hipMemcpyDeviceToDevice, st);
  if (err == hipSuccess && count && action) {
    hipLaunchKernelGGL(pw_search_actions_kernel, dim3(static_cast<unsigned>((count + 255) / 256)), dim3(256), 0, st, s->d_action + first,
                       count, action);
    err = hipGetLastError();
  }
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string("pw_search_read_links: ") + hipGetErrorString(err));
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_search_read_flags(PwSearch* s, int64_t first, int64_t count, uint8_t* pruned, void* stream) try {
  if (!s || !pruned) return pw_fail(PW_EINVAL, "null argument");
  PwDeviceGuard guard(s->eng->set->device);
  if (first < 0 || count < 0 || first + count > s->layer_end) return pw_fail(PW_EINVAL, "state range out of bounds");
  if (count == 0) return PW_OK;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const hipError_t err = s->width > 0
                             ? hipMemcpyAsync(pruned, s->d_pruned + first, static_cast<size_t>(count), hipMemcpyDeviceToDevice, st)
                             : hipMemsetAsync(pruned, 0, static_cast<size_t>(count), st);
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string("pw_search_read_flags: ") + hipGetErrorString(err));
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_search_plan(PwSearch* s, int64_t index, uint8_t* actions, int32_t cap, void* stream) try {
  if (!s || (!actions && cap > 0)) return pw_fail(PW_EINVAL, "null argument");
  PwDeviceGuard guard(s->eng->set->device);
  if (index < 0 || index >= s->layer_end) return pw_fail(PW_EINVAL, "state index out of bounds");
  hipStream_t st = static_cast<hipStream_t>(stream);
  int32_t* d_len = reinterpret_cast<int32_t*>(s->d_plan + ((s->plan_cap + 3) & ~3));
  hipLaunchKernelGGL(pw_search_plan_kernel, dim3(1), dim3(1), 0, st, s->d_parent, s->d_action, index, s->d_plan,
                     s->plan_cap, d_len);
  int32_t len = 0;
  hipError_t err = hipMemcpyAsync(&len, d_len, 4, hipMemcpyDeviceToHost, st);
  if (err == hipSuccess) err = hipStreamSynchronize(st);
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string("pw_search_plan: ") + hipGetErrorString(err));
  if (len > s->plan_cap) return pw_fail(PW_ELIMIT, "plan longer than 65536 actions");
  if (len > cap) return len;  // caller retries with a larger buffer
  std::vector<uint8_t> rev(static_cast<size_t>(len));
  if (len) {
    err = hipMemcpy(rev.data(), s->d_plan, static_cast<size_t>(len), hipMemcpyDeviceToHost);
    if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string("pw_search_plan: ") + hipGetErrorString(err));
  }
  for (int i = 0; i < len; i++) actions[i] = rev[static_cast<size_t>(len - 1 - i)];
  return len;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

}  // extern "C"

// ------------------------------------------------------------------------------------
// K5b batched search of SMALL puzzles (SURVEY 8-f3 x 8-f4: the solvability filter of generate.py:262-297 over a whole
// generated set).  pw_search_* explores ONE puzzle with a launch per pass and a host readback per layer: right for state
// spaces of millions, hopeless for the thousands of Level-0 puzzles a generator emits, whose searches end after a few
// hundred to a few thousand states (59 states: 0.9 ms of launch overhead, slower than a host FIFO).  Here ONE launch
// searches them all: persistent workgroups take puzzles off a device counter, and the whole breadth-first loop -- expand
// the layer, test the goal, insert into the closed set, next layer -- runs inside the kernel.
//   * a state is ONE 64-bit word: 4 + 4 bits per movable (grids up to 16 x 16 with their border, up to 8 movables:
//     every Level-0 recipe); the word itself is the key of the closed set, so the set is exact without a second store;
//   * the closed set starts as a 4 096-slot table in LDS (most puzzles never leave it) and moves to tables of 2^16, 2^20,
//     2^22 ... slots in the workgroup's HBM slab when a layer could outgrow it (rehash from the state store; the check is
//     made BEFORE a layer is expanded -- total + 4 * layer states fit at half load -- so no insert ever fails);
//   * the state store (discovery order: layer d is a contiguous index range) lives in the slab; one lane per parent runs
//     the table-only step (lane_step: the overlap tables, csrc/pw_step_kernels.inc) for the four actions.
// Verdicts: 1 solved (plan_len = depth of the first goal state = length of a shortest plan), 0 unsolvable (space
// exhausted), 2 unknown (more than max_states states), 3 not searched (puzzle beyond 16 x 16 / 8 movables, or without
// overlap tables).  Same answers as the layer-synchronous pw_search_* with novelty width 0 (tests/test_gpu_search.py).
// ------------------------------------------------------------------------------------
#define PW_BS_LDS_SLOTS 4096u

struct BatchSearchArgs {
  const PwPuzzleHeader* hdrs;
  const uint8_t* blob;
  const uint64_t* ovl;
  const PwOvlDir* ovl_dir;
  const int32_t* puzzles;  // [n] set indices, or NULL = 0 .. n - 1
  int32_t n;
  int32_t num_puzzles;
  uint32_t max_states;
  uint8_t* slab;           // gridDim.x slabs of slab_bytes: state store (max_states words), then the HBM tables
  uint64_t slab_bytes;
  uint32_t level_slots[6]; // slots of table level 1 .. (0 = no such level); level 0 is the LDS table
  uint64_t level_off[6];   // byte offsets of those tables in the slab
  uint8_t* verdict;
  int32_t* plan_len;
  int32_t* num_states;     // optional: states in the closed set when the search ended
  uint32_t* next;          // work counter
  uint8_t* plans;          // optional [n][plan_cap]: the actions of a shortest plan
  int32_t plan_cap;
  uint64_t link_off;       // with plans: byte offset of the (parent << 2 | action) word of every stored state in the slab
};

__global__ __launch_bounds__(256) void pw_search_batch_kernel(BatchSearchArgs a) {
  __shared__ unsigned long long s_tab[PW_BS_LDS_SLOTS];
  __shared__ uint32_t s_total, s_found, s_overflow, s_goal_idx;
  __shared__ int32_t s_item;
  const int tid = threadIdx.x;
  unsigned long long* store = reinterpret_cast<unsigned long long*>(a.slab + static_cast<uint64_t>(blockIdx.x) * a.slab_bytes);
  uint32_t* link = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(store) + a.link_off);  // (only with a.plans)
  for (;;) {
    const int item = pw_bs_next_item(a.next, &s_item);
    if (item >= a.n) return;
    const int pid = pw_clamp_pid(a.puzzles ? a.puzzles[item] : item, a.num_puzzles);
    const PwPuzzleHeader* h = a.hdrs + pid;
    const int G = h->G;
    if (!pw_bs_fits(h, a.ovl_dir, pid)) {  // not this kernel's puzzle: the caller searches it alone
      if (tid == 0) {
        a.verdict[item] = 3;
        a.plan_len[item] = -1;
        if (a.num_states) a.num_states[item] = 0;
      }
      continue;
    }
    LanePuzzleT<const uint64_t*, 2> p;
    uint32_t OT[8];
    pw_bs_puzzle(a.hdrs, a.blob, a.ovl, a.ovl_dir, pid, p, OT);

    PwBatchSet<false> set;
    set.start(s_tab, nullptr, PW_BS_LDS_SLOTS);
    uint32_t P0[4];
    pw_bs_load_init(h, P0);
    const uint64_t k0 = pw_bs_pack(P0);
    int at_goal = 0;
#pragma unroll
    for (int j = 1; j < 8; j++)
      if (j <= G) at_goal += reinterpret_cast<const uint16_t*>(h->init)[j] == reinterpret_cast<const uint16_t*>(h->goal)[j - 1];
    if (tid == 0) {
      s_total = 1u;
      s_found = 0xFFFFFFFFu;
      s_goal_idx = 0xFFFFFFFFu;
      s_overflow = 0u;
      store[0] = k0;
    }
    __syncthreads();
    if (tid == 0) set.put(k0, 0u);
    int verdict = -1, plan_len = -1;
    if (at_goal == G) {  // the start state is a goal state (vacuously without goals): the empty plan
      verdict = 1;
      plan_len = 0;
    }
    uint32_t begin = 0u, end = 1u, depth = 0u;
    while (verdict < 0) {
      __syncthreads();
      // (workgroup-uniform: `end` was read from s_total between two barriers; re-reading s_total here would race with the
      //  atomicAdd of a wavefront that is already expanding)
      const uint32_t total = end, L = end - begin;
      // everything this layer can add must fit at half load
      if (set.grow(min(static_cast<uint64_t>(total) + 4ull * L, static_cast<uint64_t>(a.max_states)), a.level_slots, a.level_off,
                   reinterpret_cast<uint8_t*>(store), store, total))
        __syncthreads();  // (uniform) the rehash is complete
      for (uint32_t i = begin + tid; i < end; i += 256u) {
        uint32_t PP[4];
        pw_bs_unpack(store[i], PP);
#pragma unroll 1
        for (int act = 0; act < 4; act++) {
          LaneEnv<8> s;
          pw_bs_fresh_env(PP, s);
          if (!lane_step<8>(p, h, OT, s, act, 0u, -1)) continue;  // nothing moved: the parent itself
          // a goal state decides the search whether or not the store still has room for it (one seen in an earlier layer would
          // have ended the search there, so this is a new one)
          if (s.term == 1) atomicMin(&s_found, depth + 1u);
          uint32_t idx;
          if (!set.claim(pw_bs_pack(s.P), store, a.max_states, &s_total, &s_overflow, idx)) continue;
          if (a.plans) {
            link[idx] = (i << 2) | static_cast<uint32_t>(act);
            if (s.term == 1) atomicMin(&s_goal_idx, idx);
          }
        }
      }
      __threadfence();
      __syncthreads();
      // (with plans asked for, a layer that overflowed the store is UNKNOWN whether or not a goal state happened to get a slot
      //  before the store filled up: which candidates did is thread order, the verdict must not be)
      if (s_found != 0xFFFFFFFFu && (!a.plans || (s_goal_idx != 0xFFFFFFFFu && !s_overflow))) {
        verdict = 1;
        plan_len = static_cast<int>(s_found);
      } else if (s_overflow || s_found != 0xFFFFFFFFu) {  // (a goal state that found no room in the store has no links to walk)
        verdict = 2;
      } else {
        begin = end;
        end = s_total;
        depth++;
        if (begin == end) verdict = 0;  // the reachable space is exhausted without a goal state
      }
    }
    if (tid == 0) {
      a.verdict[item] = static_cast<uint8_t>(verdict);
      a.plan_len[item] = plan_len;
      if (a.num_states) a.num_states[item] = static_cast<int32_t>(min(s_total, a.max_states));
      if (a.plans && verdict == 1 && plan_len > 0 && plan_len <= a.plan_cap) {  // walk the links back from the goal state
        uint8_t* out = a.plans + static_cast<int64_t>(item) * a.plan_cap;
        uint32_t at = s_goal_idx;
        for (int k = plan_len - 1; k >= 0; k--) {
          const uint32_t l = link[at];
          out[k] = static_cast<uint8_t>(l & 3u);
          at = l >> 2;
        }
      }
    }
  }
}

extern "C" int pw_search_batch(PwEngine* e, const int32_t* puzzles, int32_t n, int64_t max_states_each, int32_t novelty_width,
                               uint8_t* verdict, int32_t* plan_len, int32_t* num_states, uint8_t* plans, int32_t plan_cap,
                               void* stream) try {
  if (!e) return pw_fail(PW_EINVAL, "null engine");
  if (novelty_width != 0) return pw_fail(PW_EINVAL, "pw_search_batch: novelty_width must be 0 (breadth-first search; IW(k) is pw_search_create's)");
  if (max_states_each < 1 || max_states_each > (1ll << 28)) return pw_fail(PW_EINVAL, "max_states_each must be in 1 .. 2^28");
  if (n <= 0) return PW_OK;
  if (!verdict || !plan_len) return pw_fail(PW_EINVAL, "null argument");
  if (!e->d_ovl || !e->d_ovl_dir) return pw_fail(PW_EINVAL, "pw_search_batch needs the engine's overlap tables (PW_OPT_STEP_TABLES)");
  if (plans && plan_cap < 1) return pw_fail(PW_EINVAL, "pw_search_batch: plan_cap must be >= 1 with a plan buffer");
  PwDeviceGuard guard(e->set->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  BatchSearchArgs a;
  a.hdrs = e->set->d_headers;
  a.blob = e->set->d_blob;
  a.ovl = e->d_ovl;
  a.ovl_dir = e->d_ovl_dir;
  a.puzzles = puzzles;
  a.n = n;
  a.num_puzzles = e->set->count;
  a.max_states = static_cast<uint32_t>(max_states_each);
  // slab of one workgroup: the state store, then tables of 2^16, 2^20, 2^22, 2^24 ... slots up to >= 2 * max_states
  uint64_t off = pw_pad256(static_cast<uint64_t>(max_states_each) * 8);
  a.plans = plans;
  a.plan_cap = plan_cap;
  a.link_off = off;
  if (plans) off += pw_pad256(static_cast<uint64_t>(max_states_each) * 4);
  a.slab_bytes = pw_bs_ladder(static_cast<uint64_t>(max_states_each), PW_BS_LDS_SLOTS, 8, off, a.level_slots, a.level_off);
  int64_t groups = 0;
  if (int rc = engine_search_slab(e, n, a.slab_bytes, st, "pw_search_batch", &groups, &a.slab, &a.next)) return rc;
  a.verdict = verdict;
  a.plan_len = plan_len;
  a.num_states = num_states;
  if (hipMemsetAsync(a.next, 0, 4, st) != hipSuccess) return pw_fail(PW_EDEVICE, "pw_search_batch: hipMemsetAsync failed");
  hipLaunchKernelGGL(pw_search_batch_kernel, dim3(static_cast<unsigned>(groups)), dim3(256), 0, st, a);
  return check_launch("pw_search_batch");
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

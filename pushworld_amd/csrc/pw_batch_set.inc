// pw_batch_set.inc -- what the batched searches of small puzzles share on the device, written once (DESIGN.md K5b, K13, K22).
// Part of the single translation unit pw_kernels.hip, included there after pw_step_kernels.inc (uses its table-only lane step)
// and before its users: pw_search.inc (K5b pw_search_batch_kernel), pw_solution_batch.inc (K13 pw_solve_batch_kernel and its
// query), pw_push_solution_batch.inc (K22 pw_push_solve_batch_kernel and its query), pw_guide.inc (K28) and, for the small
// helpers only, pw_push_plan_batch.inc (K24).  A puzzle of these kernels has at most 8 movables on a grid of at most 16 x 16,
// and a state is ONE 64-bit word.
//
//   state words   pack / unpack / hash, the bits of the first N movables, insert and find in an open-addressing table of words;
//   small helpers the next item off the work counter, the "fits these kernels" test, the puzzle as the lane step sees it, a
//                 pos row or the initial state as four words, the goal test on the word, a fresh LaneEnv for one trial step;
//   closed set    PwBatchSet: the workgroup's table that starts in the kernel's LDS arrays and climbs the 2^16 / 2^20 / ... ladder
//                 of its slab (start, grow before the layer, claim a successor);
//   slot table    the per-item table from key to row of a STORED item: clear and fill (a workgroup), probe (a thread);
//   K13 lookup    SolveBatchTables and pw_sb_lookup: (puzzle id, pos row) -> row of the puzzle's stored table.  What a row
//                 answers (pw_sb_row_cost, pw_sb_row_acts) is decoded in pw_solution_batch.inc, behind PW_SOLVE_INF, which
//                 pw_solution.inc defines later than this file.
// What stays at the call sites: the LDS arrays themselves (their sizes differ), the layer loop of K5b and K13 and K22's
// parents-then-rows loop with their barriers, how much a layer can add (`need`), the goal and verdict rules, the sweeps, the
// rows, the slab layouts, and every best-first store (pw_plan_batch.inc, the tagged slabs of pw_push_plan_batch.inc).
// Every function with a barrier says so: it is called by all 256 threads of the workgroup in uniform control flow.

#define PW_BS_EMPTY 0xFFFFFFFFFFFFFFFFull
#define PW_SB_NOROW 0xFFFFFFFFu

// ---- 1. state words ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t pw_bs_pack(const uint32_t (&P)[4]) {
  uint64_t k = 0;
#pragma unroll
  for (int w = 0; w < 4; w++) {
    const uint32_t v = P[w];
    const uint32_t r = (v & 0xfu) | ((v >> 4) & 0xf0u) | ((v >> 8) & 0xf00u) | ((v >> 12) & 0xf000u);
    k |= static_cast<uint64_t>(r) << (16 * w);
  }
  return k;
}
__device__ __forceinline__ void pw_bs_unpack(uint64_t k, uint32_t (&P)[4]) {
#pragma unroll
  for (int w = 0; w < 4; w++) {
    const uint32_t r = static_cast<uint32_t>(k >> (16 * w)) & 0xffffu;
    P[w] = (r & 0xfu) | ((r & 0xf0u) << 4) | ((r & 0xf00u) << 8) | ((r & 0xf000u) << 12);
  }
}
__device__ __forceinline__ uint32_t pw_bs_hash(uint64_t k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  return static_cast<uint32_t>(k ^ (k >> 33));
}

// the bits of a state word that belong to the first n movables (8 per movable)
__host__ __device__ __forceinline__ uint64_t pw_sb_keep(int n) { return n >= 8 ? ~0ull : ((1ull << (8 * n)) - 1ull); }

// true when `key` was not in the table (it is now, in `slot`); else `slot` holds it.  The table never fills beyond half (see
// PwBatchSet::grow)
__device__ __forceinline__ bool pw_bs_insert_slot(unsigned long long* tab, uint32_t mask, uint64_t key, uint32_t& slot) {
  slot = pw_bs_hash(key) & mask;
  for (;;) {
    const unsigned long long old = atomicCAS(tab + slot, PW_BS_EMPTY, static_cast<unsigned long long>(key));
    if (old == PW_BS_EMPTY) return true;
    if (old == key) return false;
    slot = (slot + 1u) & mask;
  }
}

// read only: the store index of `key`, PW_SB_NOROW when the table does not hold it (the table is at most half full)
__device__ __forceinline__ uint32_t pw_bs_find(const unsigned long long* tab, const uint32_t* tidx, uint32_t mask, uint64_t key) {
  uint32_t slot = pw_bs_hash(key) & mask;
  for (uint32_t walked = 0; walked <= mask; walked++) {
    const unsigned long long v = tab[slot];
    if (v == key) return tidx[slot];
    if (v == PW_BS_EMPTY) return PW_SB_NOROW;
    slot = (slot + 1u) & mask;
  }
  return PW_SB_NOROW;
}

// ---- 2. small helpers ----------------------------------------------------------------------------------------------------------
// The next item off the work counter, the same for every thread (two barriers: behind the first, the previous item's shared
// state is no longer read).  Called by the whole workgroup.
__device__ __forceinline__ int pw_bs_next_item(uint32_t* next, int32_t* s_item) {
  __syncthreads();
  if (threadIdx.x == 0) *s_item = static_cast<int32_t>(atomicAdd(next, 1u));
  __syncthreads();
  return *s_item;
}

// a puzzle of these kernels: 1 .. 8 movables, at most 16 x 16, overlap tables present (else the caller searches it alone)
__device__ __forceinline__ bool pw_bs_fits(const PwPuzzleHeader* h, const PwOvlDir* ovl_dir, int pid) {
  const int N = h->N, W = h->W, H = h->H;
  const uint4 dirw = *reinterpret_cast<const uint4*>(ovl_dir + pid);
  return !(N < 1 || N > 8 || W > 16 || H > 16 || dirw.x == 0u);
}

// the puzzle as the table-only lane step sees it
__device__ __forceinline__ void pw_bs_puzzle(const PwPuzzleHeader* hdrs, const uint8_t* blob, const uint64_t* ovl,
                                             const PwOvlDir* ovl_dir, int pid, LanePuzzleT<const uint64_t*, 2>& p,
                                             uint32_t (&OT)[8]) {
  StepArgs sa;
  sa.hdrs = hdrs;
  sa.blob = blob;
  sa.ovl = ovl;
  sa.ovl_dir = ovl_dir;
  lane_puzzle<8>(sa, pid, p, OT);
}

// a row of a pos / starts array ([npad][2] int8) as four words: zeros beyond npad movables
__device__ __forceinline__ void pw_bs_load_row(const int8_t* row, int npad, uint32_t (&P)[4]) {
  if (npad >= 8) {
    const uint4 v = *reinterpret_cast<const uint4*>(row);
    P[0] = v.x, P[1] = v.y, P[2] = v.z, P[3] = v.w;
  } else {
    const uint2 v = *reinterpret_cast<const uint2*>(row);
    P[0] = v.x, P[1] = v.y, P[2] = 0u, P[3] = 0u;
  }
}
// the puzzle's initial state (the 16-byte init row, whatever it holds beyond N)
__device__ __forceinline__ void pw_bs_load_init(const PwPuzzleHeader* h, uint32_t (&P)[4]) {
#pragma unroll
  for (int w = 0; w < 4; w++) P[w] = reinterpret_cast<const uint32_t*>(h->init)[w];
}

// goal test on the word, (key & gmask) == gkey: movable j = 1 .. G on goal j - 1 (every state without goals)
__device__ __forceinline__ void pw_bs_goal_word(const PwPuzzleHeader* h, uint64_t& gkey, uint64_t& gmask) {
  const int G = h->G;
  gkey = 0;
  gmask = 0;
#pragma unroll
  for (int j = 1; j < 8; j++)
    if (j <= G) {
      const uint32_t g = reinterpret_cast<const uint16_t*>(h->goal)[j - 1];
      gkey |= static_cast<uint64_t>((g & 0xfu) | ((g >> 4) & 0xf0u)) << (8 * j);
      gmask |= 0xffull << (8 * j);
    }
}

// a fresh environment at the state PP for one trial step
__device__ __forceinline__ void pw_bs_fresh_env(const uint32_t (&PP)[4], LaneEnv<8>& s) {
#pragma unroll
  for (int w = 0; w < 4; w++) s.P[w] = PP[w];
  s.steps = 0;
  s.term = 0;
  s.trunc = 0;
  s.reward = 0.0;
  s.dgoals = 0;
}

// ---- 3. the workgroup's closed set ---------------------------------------------------------------------------------------------
// Level 0 is a table in the kernel's LDS; levels 1 .. are tables of level_slots[k] slots at level_off[k] in the workgroup's
// slab (pw_bs_ladder: the top one holds 2 * max_states).  With kIdx every slot also holds the store index of its state (a
// uint32 array: next to the LDS table, behind the keys of a slab table), which pw_bs_find(tab, tidx, cap - 1, key) reads.
// The members are workgroup-uniform.
template <bool kIdx>
struct PwBatchSet {
  unsigned long long* tab;
  uint32_t* tidx;  // (kIdx)
  uint32_t cap;
  int level;

  // `key` is state `idx` of the store
  __device__ __forceinline__ void put(uint64_t key, uint32_t idx) {
    uint32_t sl;
    (void)pw_bs_insert_slot(tab, cap - 1u, key, sl);
    if (kIdx) tidx[sl] = idx;
  }

  // The empty set in the caller's LDS arrays (`lds_idx` NULL without kIdx).  Every thread clears its share: a barrier comes
  // before the first put.
  __device__ __forceinline__ void start(unsigned long long* lds_tab, uint32_t* lds_idx, uint32_t lds_slots) {
    tab = lds_tab;
    tidx = lds_idx;
    cap = lds_slots;
    level = 0;
    for (uint32_t i = threadIdx.x; i < lds_slots; i += 256u) lds_tab[i] = PW_BS_EMPTY;
  }

  // Growth BEFORE the inserts: `need` states (what is stored and everything the next inserts can add, capped at max_states) must
  // fit at half load, so no insert ever fails.  Climbs the ladder as far as that takes and rehashes store[0 .. count).  Called
  // by the whole workgroup with uniform arguments behind a barrier (nobody inserts).  True (for every thread) when the set grew:
  // it has been through one barrier, between clearing and rehashing, and the CALLER's next barrier ends the rehash -- no
  // claim before it.
  __device__ __forceinline__ bool grow(uint64_t need, const uint32_t (&level_slots)[6], const uint64_t (&level_off)[6],
                                       uint8_t* slab, const unsigned long long* store, uint32_t count) {
    bool grown = false;
    while (static_cast<uint64_t>(cap) < 2ull * need) {
      if (level >= 6 || level_slots[level] == 0u) break;  // (the top level holds 2 * max_states by construction)
      cap = level_slots[level];
      tab = reinterpret_cast<unsigned long long*>(slab + level_off[level]);
      if (kIdx) tidx = reinterpret_cast<uint32_t*>(tab + cap);
      level++;
      grown = true;
    }
    if (grown) {
      for (uint32_t i = threadIdx.x; i < cap; i += 256u) tab[i] = PW_BS_EMPTY;
      __threadfence();
      __syncthreads();
      for (uint32_t i = threadIdx.x; i < count; i += 256u) put(store[i], i);
    }
    return grown;
  }

  // A successor: true when `key` is new AND got place `idx` of the store.  Once the store is full (*s_overflow) nothing more
  // goes into the table: it has room for max_states + the inserts in flight.  The index of a slot is read only behind a barrier.
  __device__ __forceinline__ bool claim(uint64_t key, unsigned long long* store, uint32_t max_states, uint32_t* s_total,
                                        uint32_t* s_overflow, uint32_t& idx) {
    if (*reinterpret_cast<volatile uint32_t*>(s_overflow)) return false;
    uint32_t sl;
    if (!pw_bs_insert_slot(tab, cap - 1u, key, sl)) return false;
    idx = atomicAdd(s_total, 1u);
    if (idx >= max_states) {
      *s_overflow = 1u;
      return false;
    }
    store[idx] = key;
    if (kIdx) tidx[sl] = idx;
    return true;
  }
};

// ---- 4. the slot table of a stored item: key -> row ----------------------------------------------------------------------------
// slots[0 .. smask] from the `total` distinct keys of an item (smask + 1 >= 2 * total: never more than half full, so a walk
// ends at a free slot), in two steps, each called by the whole workgroup: clear, then -- behind whatever else the kernel stores
// for the item -- fill (one barrier, in front of the inserts).
__device__ __forceinline__ void pw_sb_slots_clear(uint32_t* slots, uint32_t smask) {
  for (uint32_t i = threadIdx.x; i <= smask; i += 256u) slots[i] = PW_SB_NOROW;
}
__device__ __forceinline__ void pw_sb_slots_fill(uint32_t* slots, uint32_t smask, const unsigned long long* keys, uint32_t total) {
  __threadfence();
  __syncthreads();  // the slots are empty: every row takes the first free one on its probe path
  for (uint32_t i = threadIdx.x; i < total; i += 256u) {
    uint32_t sl = pw_bs_hash(keys[i]) & smask;
    for (uint32_t walked = 0; walked <= smask; walked++) {
      if (atomicCAS(slots + sl, PW_SB_NOROW, i) == PW_SB_NOROW) break;
      sl = (sl + 1u) & smask;
    }
  }
}

// the row of `key` among the item's stored keys, -1: none (a hit is confirmed against the stored key)
__device__ __forceinline__ int64_t pw_sb_probe(const uint32_t* slots, uint32_t smask, const unsigned long long* keys, uint64_t key) {
  uint32_t sl = pw_bs_hash(key) & smask;
  for (uint32_t walked = 0; walked <= smask; walked++) {
    const uint32_t r = slots[sl];
    if (r == PW_SB_NOROW) return -1;
    if (keys[r] == key) return r;
    sl = (sl + 1u) & smask;
  }
  return -1;
}

// ---- 5. the K13 lookup ---------------------------------------------------------------------------------------------------------
// the stored tables of a PwSolveBatch as a query sees them (solve_batch_tables fills it)
struct SolveBatchTables {
  const PwPuzzleHeader* hdrs;
  int32_t num_puzzles;
  const int32_t* item_of_puzzle;  // [num_puzzles], -1: no stored table
  const int64_t* row_off;         // [items]
  const int64_t* slot_off;
  const uint8_t* slot_log2;
  const unsigned long long* pool_key;
  const uint16_t* pool_cost;
  const uint8_t* pool_acts;
  const uint32_t* pool_slots;
};

#define PW_SB_NOTABLE (-2)  // pw_sb_lookup: an id outside the set, or a puzzle without a stored table

// The row of the state `row` ([npad][2] int8) in puzzle pid's stored table, with `base` where that table's rows begin in the
// pools: -1 when the table does not hold the state, PW_SB_NOTABLE when there is no table to ask.  Only the first N movables
// count (a pos row may hold anything beyond them); every coordinate in 0 .. 15 and inside W x H, else the state is in no table.
__device__ __forceinline__ int64_t pw_sb_lookup(const SolveBatchTables& t, int32_t pid, const int8_t* row, int npad, int64_t& base) {
  base = 0;
  if (pid < 0 || pid >= t.num_puzzles) return PW_SB_NOTABLE;
  const int32_t item = t.item_of_puzzle[pid];
  if (item < 0) return PW_SB_NOTABLE;  // (another table's item)
  const PwPuzzleHeader* h = t.hdrs + pid;
  const int N = h->N, W = h->W, H = h->H;
  uint32_t P[4];
  pw_bs_load_row(row, npad, P);
  bool inside = N <= npad;
#pragma unroll
  for (int j = 0; j < 8; j++)
    if (j < N) {
      const uint32_t xy = (P[j >> 1] >> (16 * (j & 1))) & 0xffffu;
      const int x = static_cast<int8_t>(xy & 0xffu), y = static_cast<int8_t>(xy >> 8);
      inside = inside && x >= 0 && x < W && x < 16 && y >= 0 && y < H && y < 16;
    }
  // (the three per-item words are independent of each other: one level of the chain of dependent loads)
  base = t.row_off[item];
  if (!inside) return -1;
  const uint32_t* slots = t.pool_slots + t.slot_off[item];
  const uint32_t smask = (1u << t.slot_log2[item]) - 1u;
  return pw_sb_probe(slots, smask, t.pool_key + base, pw_bs_pack(P) & pw_sb_keep(N));
}

// pw_push_solution_batch.inc -- cost-to-go tables OVER PUSHES of MANY small puzzles in one launch (DESIGN.md K22).
// Included from pw_kernels.hip after pw_push_table.inc and pw_solution_batch.inc (uses pw_batch_set.inc's state words and
// pw_solution_batch.inc's PW_SB_* statuses and the table-only lane step).  The SEARCH kernel below keeps its own closed-set
// code, the text PwBatchSet was written from: built on the shared helpers it measured about 1 % slower and the cause was not
// found (profiles/batch_closed_set.txt).  The query kernel and the host half use pw_batch_set.inc and pw_bs_ladder.
//
// pw_push_search_solve (K18) gives ONE puzzle its table with a handle, a launch sequence per layer and a flood launch per
// query: at the sizes of the Level-0 pool it is bound by launches.  pw_push_solve_batch is K18 in the frame of K13: persistent
// workgroups of 256 take items off a device counter and do everything for an item inside the kernel --
//   1. the search over canonical states: a node is the 64-bit packed word (pw_bs_pack) with the agent at the canon of its walk
//      region and zeros beyond the puzzle's N.  Parents are taken 256 at a time in store order; every lane floods the region of
//      one parent on the packed word (lane_step<8> with the agent's byte replaced: the step K13 uses, so states with overlaps
//      are exact) into region boards of 16 rows x 16 bits in LDS; the push counts are scanned; then the lanes take the ROWS of
//      the 256 parents (a parent yields tens of rows): step, range check on the 16-bit fields BEFORE packing, flood of the
//      successor for its canon, insert into the closed set (LDS first, then the 2^16 / 2^20 ... ladder of the workgroup's slab,
//      grown before the rows of a chunk are taken).  The rows stay in the slab with the key of their successor;
//   2. rows: the keys of the rows become local state indices (read-only lookups; a miss is counted, status 6);
//   3. K18's sweeps over the rows, one barrier per sweep (K13's rotating flags), then best and the row bits;
//   4. atomic reservations in the caller-sized pools of states and rows, coalesced stores, a per-item lookup from key to state.
// State 0 is the start; the order of a state's rows is (y, x, action); state numbers inside a layer and the pool offsets may
// depend on the schedule.  pw_push_solve_batch_query answers a mixed batch of live states in ONE capturable launch.
//
// Every loop is bounded by the items, 256 cells x 4 actions, the slots, the states, the rows or 255 trace steps; no kernel waits
// on another workgroup; there is no device assert.

#define PW_PSB_LDS_SLOTS 2048u      // closed set in LDS: 1 024 states at half load
#define PW_PSB_ROWS_PER_STATE 32    // rows the slab holds per state of max_states_each
#define PW_PSB_NOBEST 0xFFFFu
#define PW_PSB_META_GOAL 0x01000000u
#define PW_PSB_META_OPTIMAL 0x02000000u
#define PW_PSB_META_SAFE 0x04000000u
#define PW_PSB_META_OUTSIDE 0x80000000u  // the successor leaves the grid (kept out of the flags that are stored)

// row y of board k of one lane: the boards of the 256 lanes are interleaved (consecutive lanes, consecutive 16-bit words)
#define PW_PSB_BS(b, k, y, lanes) (b)[((k) * 16 + (y)) * (lanes)]
#define PW_PSB_B(b, k, y) PW_PSB_BS(b, k, y, 256)

struct PushSolveBatchArgs {
  const PwPuzzleHeader* hdrs;
  const uint8_t* blob;
  const uint64_t* ovl;
  const PwOvlDir* ovl_dir;
  const int32_t* puzzles;  // [n] set indices, or NULL = 0 .. n - 1
  const int8_t* starts;    // [n][npad][2], or NULL = every puzzle's initial state
  int32_t npad;
  int32_t n;
  int32_t num_puzzles;
  uint32_t max_states, max_rows;
  uint8_t* slab;           // gridDim.x slabs of slab_bytes
  uint64_t slab_bytes;
  uint32_t level_slots[6]; // slots of table level 1 .. (0 = no such level); level 0 is the LDS table
  uint64_t level_off[6];   // level_slots keys (8 bytes), then level_slots store indices (4 bytes)
  uint64_t srow_off, cost_off, best_off, rkey_off, rmeta_off;
  uint32_t* next;          // work counter
  unsigned long long* counters;  // [0] states + 1 of every built table, [1] their rows, [2] lookup slots reserved, [3] missing successors
  uint8_t* status;
  int32_t* summary;        // [n][6]
  int64_t* state_off;      // [n]
  int64_t* row_off;        // [n]
  int64_t* slot_off;       // [n]
  uint8_t* slot_log2;      // [n]
  int32_t* item_of_puzzle; // [num_puzzles]
  int64_t states_cap, rows_cap, slots_cap;
  unsigned long long* pool_key;
  int64_t* pool_srow;
  int32_t* pool_cost;
  int32_t* pool_best;
  int32_t* pool_succ;
  uint16_t* pool_from;
  uint8_t* pool_action;
  uint8_t* pool_flags;
  uint32_t* pool_slots;
};

// every one of the first N movables lies inside its grid, read off the 16-bit (x, y) fields
__device__ __forceinline__ bool pw_psb_in_grid(const uint32_t (&P)[4], const uint32_t (&OT)[8], int N, int W, int H) {
  bool in = true;
#pragma unroll
  for (int j = 0; j < 8; j++)
    if (j < N) {
      const uint32_t f = (P[j >> 1] >> (16 * (j & 1))) & 0xffffu;
      const int x = static_cast<int8_t>(f & 0xffu), y = static_cast<int8_t>(f >> 8);
      const int w = static_cast<int>(OT[j] & 0xffu), hh = static_cast<int>((OT[j] >> 8) & 0xffu);
      in = in && x >= 0 && y >= 0 && x + w <= W && y + hh <= H;
    }
  return in;
}

// One step of the state PP with the agent placed at (x, y): 0 nothing moves, 1 a walk move (the agent and nothing else),
// 2 a push move (the agent and at least one other movable).  `s` holds the stepped state.
template <class P>
__device__ __forceinline__ int pw_psb_step(const P& p, const PwPuzzleHeader* h, const uint32_t (&OT)[8], const uint32_t (&PP)[4],
                                           int x, int y, int act, LaneEnv<8>& s) {
  s.P[0] = (PP[0] & 0xffff0000u) | static_cast<uint32_t>(x) | (static_cast<uint32_t>(y) << 8);
  s.P[1] = PP[1];
  s.P[2] = PP[2];
  s.P[3] = PP[3];
  s.steps = 0;
  s.term = 0;
  s.trunc = 0;
  s.reward = 0.0;
  s.dgoals = 0;
  if (!lane_step<8>(p, h, OT, s, act, 0u, -1)) return 0;
  const uint32_t others = ((s.P[0] ^ PP[0]) & 0xffff0000u) | (s.P[1] ^ PP[1]) | (s.P[2] ^ PP[2]) | (s.P[3] ^ PP[3]);
  return others ? 2 : 1;
}

// The walk region of the state PP from (x0, y0), a fixed point over a to-do board: board 0 visited, board 1 to do, and with
// kPush boards 2 .. 5 the positions that push by action 0 .. 3.  At most 256 cells, four steps each.  Returns canon as x | y << 4.
// kLanes: the lanes whose boards are interleaved at `b` (256 here, 64 in pw_push_plan_batch.inc).
template <bool kPush, int kLanes, class P>
__device__ __forceinline__ uint32_t pw_psb_region_lanes(const P& p, const PwPuzzleHeader* h, const uint32_t (&OT)[8],
                                                  const uint32_t (&PP)[4], int x0, int y0, uint16_t* b) {
  const int W = h->W, H = h->H, aw = static_cast<int>(OT[0] & 0xffu), ah = static_cast<int>((OT[0] >> 8) & 0xffu);
  for (int y = 0; y < 16; y++) {
    PW_PSB_BS(b, 0, y, kLanes) = 0;
    PW_PSB_BS(b, 1, y, kLanes) = 0;
    if (kPush) {
      PW_PSB_BS(b, 2, y, kLanes) = 0;
      PW_PSB_BS(b, 3, y, kLanes) = 0;
      PW_PSB_BS(b, 4, y, kLanes) = 0;
      PW_PSB_BS(b, 5, y, kLanes) = 0;
    }
  }
  PW_PSB_BS(b, 0, y0, kLanes) = static_cast<uint16_t>(1u << x0);
  PW_PSB_BS(b, 1, y0, kLanes) = static_cast<uint16_t>(1u << x0);
  for (int cell = 0; cell < 256; cell++) {
    int y = 0;
    uint32_t row = 0;
    for (; y < 16; y++) {
      row = PW_PSB_BS(b, 1, y, kLanes);
      if (row) break;
    }
    if (y >= 16) break;
    const int x = __ffs(row) - 1;
    PW_PSB_BS(b, 1, y, kLanes) = static_cast<uint16_t>(row & (row - 1u));
#pragma unroll 1
    for (int act = 0; act < 4; act++) {
      const int rx = x + (act == 0 ? -1 : (act == 1 ? 1 : 0)), ry = y + (act == 2 ? -1 : (act == 3 ? 1 : 0));
      // the agent would leave its grid (not in the region) or the cell is known already: a walk move there adds nothing, so
      // the flood for a canon alone does not ask for the step's verdict (the flood for the push boards needs it: a push?)
      const bool fresh = !(rx < 0 || ry < 0 || rx + aw > W || ry + ah > H || rx > 15 || ry > 15) && !((PW_PSB_BS(b, 0, ry, kLanes) >> rx) & 1u);
      if (!kPush && !fresh) continue;
      LaneEnv<8> s;
      const int kind = pw_psb_step(p, h, OT, PP, x, y, act, s);
      if (kind == 1) {
        if (!fresh) continue;
        const uint32_t seen = PW_PSB_BS(b, 0, ry, kLanes);
        PW_PSB_BS(b, 0, ry, kLanes) = static_cast<uint16_t>(seen | (1u << rx));
        PW_PSB_BS(b, 1, ry, kLanes) = static_cast<uint16_t>(PW_PSB_BS(b, 1, ry, kLanes) | (1u << rx));
      } else if (kPush && kind == 2) {
        PW_PSB_BS(b, 2 + act, y, kLanes) = static_cast<uint16_t>(PW_PSB_BS(b, 2 + act, y, kLanes) | (1u << x));
      }
    }
  }
  for (int y = 0; y < 16; y++) {
    const uint32_t row = PW_PSB_BS(b, 0, y, kLanes);
    if (row) return static_cast<uint32_t>(__ffs(row) - 1) | (static_cast<uint32_t>(y) << 4);
  }
  return static_cast<uint32_t>(x0) | (static_cast<uint32_t>(y0) << 4);  // (never: the start is visited)
}

template <bool kPush, class P>
__device__ __forceinline__ uint32_t pw_psb_region(const P& p, const PwPuzzleHeader* h, const uint32_t (&OT)[8],
                                                  const uint32_t (&PP)[4], int x0, int y0, uint16_t* b) {
  return pw_psb_region_lanes<kPush, 256>(p, h, OT, PP, x0, y0, b);
}

__global__ __launch_bounds__(256) void pw_push_solve_batch_kernel(PushSolveBatchArgs a) {
  __shared__ unsigned long long s_tab[PW_PSB_LDS_SLOTS];
  __shared__ uint32_t s_idx[PW_PSB_LDS_SLOTS];
  __shared__ uint16_t s_boards[6 * 16 * 256];
  __shared__ uint32_t s_incl[256], s_wsum[4];
  __shared__ uint32_t s_total, s_overflow, s_goals, s_dead, s_missing, s_flag[3], s_log2, s_canon0;
  __shared__ int32_t s_item;
  __shared__ long long s_st, s_row, s_slot;
  const int tid = threadIdx.x;
  uint16_t* const b = s_boards + tid;
  uint8_t* slab = a.slab + static_cast<uint64_t>(blockIdx.x) * a.slab_bytes;
  unsigned long long* store = reinterpret_cast<unsigned long long*>(slab);
  uint32_t* srow = reinterpret_cast<uint32_t*>(slab + a.srow_off);
  uint16_t* cost = reinterpret_cast<uint16_t*>(slab + a.cost_off);
  uint16_t* best = reinterpret_cast<uint16_t*>(slab + a.best_off);
  unsigned long long* rkey = reinterpret_cast<unsigned long long*>(slab + a.rkey_off);  // the successor's key, then its index
  uint32_t* rmeta = reinterpret_cast<uint32_t*>(slab + a.rmeta_off);                    // from x | y << 8 | action << 16 | bits << 24
  for (;;) {
    __syncthreads();  // (the previous item's shared state is no longer read)
    if (tid == 0) s_item = static_cast<int32_t>(atomicAdd(a.next, 1u));
    __syncthreads();
    const int item = s_item;
    if (item >= a.n) return;
    const int pid = pw_clamp_pid(a.puzzles ? a.puzzles[item] : item, a.num_puzzles);
    const PwPuzzleHeader* h = a.hdrs + pid;
    const int N = h->N, G = h->G, W = h->W, H = h->H;
    const uint4 dirw = *reinterpret_cast<const uint4*>(a.ovl_dir + pid);
    int status = -1;
    if (N < 1 || N > 8 || W > 16 || H > 16 || dirw.x == 0u) status = PW_SB_NOT_SEARCHED;
    uint32_t total = 0, rows_done = 0;
    int32_t max_cost = -1;
    if (status < 0) {
      StepArgs sa;
      sa.hdrs = a.hdrs;
      sa.blob = a.blob;
      sa.ovl = a.ovl;
      sa.ovl_dir = a.ovl_dir;
      LanePuzzleT<const uint64_t*, 2> p;
      uint32_t OT[8];
      lane_puzzle<8>(sa, pid, p, OT);
      // the start: the item's row of `starts` or the initial state; only its first N movables count (the trap of the packed word)
      uint32_t P0[4] = {0u, 0u, 0u, 0u};
      if (a.starts) {
        const int8_t* row = a.starts + static_cast<int64_t>(item) * a.npad * 2;
        if (a.npad >= 8) {
          const uint4 v = *reinterpret_cast<const uint4*>(row);
          P0[0] = v.x, P0[1] = v.y, P0[2] = v.z, P0[3] = v.w;
        } else {
          const uint2 v = *reinterpret_cast<const uint2*>(row);
          P0[0] = v.x, P0[1] = v.y;
        }
      } else {
#pragma unroll
        for (int w = 0; w < 4; w++) P0[w] = reinterpret_cast<const uint32_t*>(h->init)[w];
      }
      if (!pw_psb_in_grid(P0, OT, N, W, H)) status = PW_SB_NOT_SEARCHED;  // a start outside its grid
      const uint64_t keep = pw_sb_keep(N);
      uint64_t gkey = 0, gmask = 0;
#pragma unroll
      for (int j = 1; j < 8; j++)
        if (j <= G) {
          const uint32_t g = reinterpret_cast<const uint16_t*>(h->goal)[j - 1];
          gkey |= static_cast<uint64_t>((g & 0xfu) | ((g >> 4) & 0xf0u)) << (8 * j);
          gmask |= 0xffull << (8 * j);
        }
      if (status < 0) {
        for (uint32_t i = tid; i < PW_PSB_LDS_SLOTS; i += 256u) s_tab[i] = PW_BS_EMPTY;
        if (tid == 0) {
          const uint32_t f = P0[0] & 0xffffu;
          s_canon0 = pw_psb_region<false>(p, h, OT, P0, static_cast<int>(f & 0xffu), static_cast<int>(f >> 8), b);
          s_total = 1u;
          s_overflow = 0u;
          s_goals = 0u;
          s_dead = 0u;
          s_missing = 0u;
          s_flag[0] = s_flag[1] = s_flag[2] = 0u;
        }
        __syncthreads();
        if (tid == 0) {
          const uint64_t k0 = ((pw_bs_pack(P0) & keep) & ~0xffull) | s_canon0;
          store[0] = k0;
          uint32_t sl;
          (void)pw_bs_insert_slot(s_tab, PW_PSB_LDS_SLOTS - 1u, k0, sl);
          s_idx[sl] = 0u;
          __threadfence();
        }
        unsigned long long* tab = s_tab;
        uint32_t* tidx = s_idx;
        uint32_t cap = PW_PSB_LDS_SLOTS, done = 0u;
        int level = 0;
        // ---- 1. the canonical states and their rows: parents in store order, 256 at a time (layers are contiguous: the parents
        // of layer d are all taken before the first of layer d + 1; goal states are expanded like any other)
        for (;;) {
          __syncthreads();
          const uint32_t cur = s_total;  // (workgroup-uniform: nothing adds to it between this barrier and the next)
          if (s_overflow) {
            status = PW_SB_TOO_MANY;
            break;
          }
          if (done >= cur) break;  // exhausted
          const uint32_t cnt = min(256u, cur - done);
          // A. one lane per parent: its region and where it pushes
          uint32_t npush = 0;
          if (static_cast<uint32_t>(tid) < cnt) {
            const uint64_t key = store[done + tid];
            uint32_t PP[4];
            pw_bs_unpack(key, PP);
            (void)pw_psb_region<true>(p, h, OT, PP, static_cast<int>(key & 15u), static_cast<int>((key >> 4) & 15u), b);
            for (int y = 0; y < 16; y++)
              npush += __popc(PW_PSB_B(b, 2, y)) + __popc(PW_PSB_B(b, 3, y)) + __popc(PW_PSB_B(b, 4, y)) + __popc(PW_PSB_B(b, 5, y));
          }
          uint32_t incl = npush;
#pragma unroll
          for (int d = 1; d < PW_WAVE; d <<= 1) {
            const uint32_t t = __shfl_up(incl, d);
            if ((tid & (PW_WAVE - 1)) >= d) incl += t;
          }
          if ((tid & (PW_WAVE - 1)) == PW_WAVE - 1) s_wsum[tid / PW_WAVE] = incl;
          __syncthreads();
          for (int w = 0; w < tid / PW_WAVE; w++) incl += s_wsum[w];
          s_incl[tid] = incl;
          const uint32_t T = s_wsum[0] + s_wsum[1] + s_wsum[2] + s_wsum[3];
          if (static_cast<uint64_t>(rows_done) + T > a.max_rows) {  // (uniform) the rows do not fit the slab
            status = PW_SB_TOO_MANY;
            break;
          }
          if (static_cast<uint32_t>(tid) < cnt) srow[done + tid] = rows_done + incl - npush;
          // growth: everything these rows can add must fit at half load
          const uint64_t need = min(static_cast<uint64_t>(cur) + T, static_cast<uint64_t>(a.max_states));
          bool grown = false;
          while (static_cast<uint64_t>(cap) < 2ull * need) {
            if (level >= 6 || a.level_slots[level] == 0u) break;  // (the top level holds 2 * max_states by construction)
            cap = a.level_slots[level];
            tab = reinterpret_cast<unsigned long long*>(slab + a.level_off[level]);
            tidx = reinterpret_cast<uint32_t*>(tab + cap);
            level++;
            grown = true;
          }
          if (grown) {
            for (uint32_t i = tid; i < cap; i += 256u) tab[i] = PW_BS_EMPTY;
            __threadfence();
            __syncthreads();
            for (uint32_t i = tid; i < cur; i += 256u) {
              uint32_t sl;
              (void)pw_bs_insert_slot(tab, cap - 1u, store[i], sl);
              tidx[sl] = i;
            }
          }
          __syncthreads();  // s_incl and the push boards of every parent are written
          const uint32_t mask = cap - 1u;
          // B. one lane per ROW of these parents
          for (uint32_t r = tid; r < T; r += 256u) {
            int lo = 0, hi = 255;  // the parent: the first lane whose inclusive count exceeds r
            while (lo < hi) {
              const int mid = (lo + hi) >> 1;
              if (s_incl[mid] > r) hi = mid;
              else lo = mid + 1;
            }
            const int j = lo;
            const uint16_t* bj = s_boards + j;
            uint32_t k = r - (j ? s_incl[j - 1] : 0u);
            // its k-th push in (y, x, action) order
            int y = 0;
            uint32_t r0 = 0, r1 = 0, r2 = 0, r3 = 0;
            for (; y < 16; y++) {
              r0 = PW_PSB_B(bj, 2, y), r1 = PW_PSB_B(bj, 3, y), r2 = PW_PSB_B(bj, 4, y), r3 = PW_PSB_B(bj, 5, y);
              const uint32_t c = __popc(r0) + __popc(r1) + __popc(r2) + __popc(r3);
              if (k < c) break;
              k -= c;
            }
            int x = 0, act = 0;
            bool found = false;
            for (int q = 0; q < 64 && !found; q++) {
              const int qx = q >> 2, qa = q & 3;
              const uint32_t rowbits = qa == 0 ? r0 : (qa == 1 ? r1 : (qa == 2 ? r2 : r3));
              if ((rowbits >> qx) & 1u) {
                if (k == 0u) {
                  x = qx, act = qa, found = true;
                } else {
                  k--;
                }
              }
            }
            const uint64_t pkey = store[done + j];
            uint32_t PP[4];
            pw_bs_unpack(pkey, PP);
            LaneEnv<8> s;
            const int kind = y < 16 && found ? pw_psb_step(p, h, OT, PP, x, y, act, s) : 0;
            uint32_t meta = static_cast<uint32_t>(x) | (static_cast<uint32_t>(y & 15) << 8) | (static_cast<uint32_t>(act) << 16);
            uint64_t ckey = 0;
            if (kind != 2) {  // (never: the boards hold push moves only) counted as a missing successor
              atomicAdd(&s_missing, 1u);
              meta |= PW_PSB_META_OUTSIDE;
            } else {
              if (s.term) meta |= PW_PSB_META_GOAL;
              // range check on the 16-bit fields BEFORE packing: a movable that leaves the grid never wraps into a nibble
              if (!pw_psb_in_grid(s.P, OT, N, W, H)) {
                meta |= PW_PSB_META_OUTSIDE;
              } else {
                const uint32_t f = s.P[0] & 0xffffu;
                const uint32_t canon = pw_psb_region<false>(p, h, OT, s.P, static_cast<int>(f & 0xffu), static_cast<int>(f >> 8), b);
                ckey = ((pw_bs_pack(s.P) & keep) & ~0xffull) | canon;
                // (once the store is full nothing more goes into the table: it has room for max_states + the inserts in flight)
                if (!*reinterpret_cast<volatile uint32_t*>(&s_overflow)) {
                  uint32_t sl;
                  if (pw_bs_insert_slot(tab, mask, ckey, sl)) {
                    const uint32_t idx = atomicAdd(&s_total, 1u);
                    if (idx < a.max_states) {
                      store[idx] = ckey;
                      tidx[sl] = idx;  // (read only after the search)
                    } else {
                      s_overflow = 1u;
                    }
                  }
                }
              }
            }
            rkey[rows_done + r] = ckey;
            rmeta[rows_done + r] = meta;
          }
          rows_done += T;
          done += cnt;
          __threadfence();
        }
        __syncthreads();
        total = min(s_total, a.max_states);
        if (status < 0) {
          // ---- 2. the rows' successors as local indices, the costs' starting values
          const uint32_t mask = cap - 1u;
          if (tid == 0) srow[total] = rows_done;
          for (uint32_t r = tid; r < rows_done; r += 256u) {
            int32_t idx = -1;
            if (!(rmeta[r] & PW_PSB_META_OUTSIDE)) {
              const uint32_t f = pw_bs_find(tab, tidx, mask, rkey[r]);
              if (f >= total) atomicAdd(&s_missing, 1u);  // inside its grid and not closed: counted, the item's status says so
              else idx = static_cast<int32_t>(f);
            }
            rkey[r] = static_cast<unsigned long long>(static_cast<uint32_t>(idx));
          }
          for (uint32_t i0 = 0; i0 < total; i0 += 256u) {  // (whole rounds: the ballot below needs every lane)
            const uint32_t i = i0 + tid;
            bool goal = false;
            if (i < total) {
              goal = (store[i] & gmask) == gkey;
              cost[i] = goal ? 0 : PW_SOLVE_INF;
              best[i] = PW_PSB_NOBEST;
            }
            const unsigned long long m = __ballot(goal);
            if ((tid & (PW_WAVE - 1)) == 0 && m) atomicAdd(&s_goals, static_cast<uint32_t>(__popcll(m)));
          }
          __threadfence();
          __syncthreads();
          if (s_missing) status = PW_SB_INTERNAL;
          // ---- 3. sweeps (K18): sweep k gives cost k to every unset state with a row of value k - 1, best = the lowest such
          // row.  Sweep k raises flag k % 3 and clears flag (k + 1) % 3, last read before the barrier that ended sweep k - 1.
          // (A cost written by sweep k is k, never k - 1, so reading it while others write is harmless.)
          if (status < 0) {
            if (s_goals) max_cost = 0;
            for (uint32_t k = 1; k <= PW_SOLVE_INF; k++) {
              if (tid == 0) s_flag[(k + 1u) % 3u] = 0u;
              const uint32_t want = k - 1u;
              bool any = false;
              for (uint32_t i = tid; i < total; i += 256u) {
                if (cost[i] != PW_SOLVE_INF) continue;
                const uint32_t r0 = srow[i], r1 = srow[i + 1u];
                for (uint32_t r = r0; r < r1; r++) {
                  const uint32_t m = rmeta[r];
                  const int32_t sc = static_cast<int32_t>(static_cast<uint32_t>(rkey[r]));
                  const uint32_t v = (m & PW_PSB_META_GOAL) ? 0u : (sc >= 0 ? static_cast<uint32_t>(cost[sc]) : PW_SOLVE_INF);
                  if (v == want) {
                    if (k < PW_SOLVE_INF) {
                      cost[i] = static_cast<uint16_t>(k);
                      best[i] = static_cast<uint16_t>(min(r - r0, PW_PSB_NOBEST - 1u));
                    }
                    any = true;
                    break;
                  }
                }
              }
              if (any) s_flag[k % 3u] = 1u;
              __syncthreads();
              if (!s_flag[k % 3u]) break;
              if (k == PW_SOLVE_INF) {
                status = PW_SB_COST_RANGE;
                break;
              }
              max_cost = static_cast<int32_t>(k);
            }
          }
          if (status < 0) {
            // the row bits (one lane per state: a row's bits need its state's cost) and the dead ends
            __syncthreads();
            for (uint32_t i0 = 0; i0 < total; i0 += 256u) {
              const uint32_t i = i0 + tid;
              bool dead = false;
              if (i < total) {
                const uint32_t mine = cost[i];
                dead = mine == PW_SOLVE_INF;
                const uint32_t r0 = srow[i], r1 = srow[i + 1u];
                for (uint32_t r = r0; r < r1; r++) {
                  uint32_t m = rmeta[r];
                  const int32_t sc = static_cast<int32_t>(static_cast<uint32_t>(rkey[r]));
                  const uint32_t v = (m & PW_PSB_META_GOAL) ? 0u : (sc >= 0 ? static_cast<uint32_t>(cost[sc]) : PW_SOLVE_INF);
                  if (v != PW_SOLVE_INF) {
                    m |= PW_PSB_META_SAFE;
                    if (mine != 0u && mine != PW_SOLVE_INF && v + 1u == mine) m |= PW_PSB_META_OPTIMAL;
                    rmeta[r] = m;
                  }
                }
              }
              const unsigned long long m = __ballot(dead);
              if ((tid & (PW_WAVE - 1)) == 0 && m) atomicAdd(&s_dead, static_cast<uint32_t>(__popcll(m)));
            }
            __threadfence();
          }
        }
      }
    }
    // ---- 4. out: the item's states and rows, when the pools have room
    __syncthreads();
    const bool built = status < 0;
    if (tid == 0) {
      long long st = -1, row = -1, slot = -1;
      uint32_t lg = 4;
      if (built) {
        st = static_cast<long long>(atomicAdd(&a.counters[0], static_cast<unsigned long long>(total) + 1ull));
        row = static_cast<long long>(atomicAdd(&a.counters[1], static_cast<unsigned long long>(rows_done)));
        while ((1ull << lg) < 2ull * total) lg++;
        if (st + static_cast<long long>(total) + 1 <= a.states_cap && row + static_cast<long long>(rows_done) <= a.rows_cap) {
          slot = static_cast<long long>(atomicAdd(&a.counters[2], 1ull << lg));
          if (slot + (1ll << lg) > a.slots_cap) slot = -1;
        }
        if (slot < 0) st = row = -1;
      }
      if (status == PW_SB_INTERNAL) atomicAdd(&a.counters[3], static_cast<unsigned long long>(s_missing));
      s_st = st;
      s_row = row;
      s_slot = slot;
      s_log2 = lg;
    }
    __syncthreads();
    const long long st = s_st, row = s_row;
    const bool stored = st >= 0;
    if (built && stored) {
      uint32_t* slots = a.pool_slots + s_slot;
      const uint32_t smask = (1u << s_log2) - 1u;
      for (uint32_t i = tid; i <= smask; i += 256u) slots[i] = PW_SB_NOROW;
      for (uint32_t i = tid; i <= total; i += 256u) {
        a.pool_srow[st + i] = static_cast<int64_t>(srow[i]);
        if (i < total) {
          const uint32_t c = cost[i], k = best[i];
          a.pool_key[st + i] = store[i];
          a.pool_cost[st + i] = c == PW_SOLVE_INF ? -1 : static_cast<int32_t>(c);
          a.pool_best[st + i] = k == PW_PSB_NOBEST ? -1 : static_cast<int32_t>(k);
        } else {
          a.pool_key[st + i] = PW_BS_EMPTY;
          a.pool_cost[st + i] = -1;
          a.pool_best[st + i] = -1;
        }
      }
      for (uint32_t r = tid; r < rows_done; r += 256u) {
        const uint32_t m = rmeta[r];
        a.pool_succ[row + r] = static_cast<int32_t>(static_cast<uint32_t>(rkey[r]));
        a.pool_from[row + r] = static_cast<uint16_t>(m & 0xffffu);
        a.pool_action[row + r] = static_cast<uint8_t>((m >> 16) & 0xffu);
        a.pool_flags[row + r] = static_cast<uint8_t>((m >> 24) & 7u);
      }
      __threadfence();
      __syncthreads();  // the slots are empty: every state takes the first free one on its probe path (the keys are distinct)
      for (uint32_t i = tid; i < total; i += 256u) {
        uint32_t sl = pw_bs_hash(store[i]) & smask;
        for (uint32_t walked = 0; walked <= smask; walked++) {
          if (atomicCAS(slots + sl, PW_SB_NOROW, i) == PW_SB_NOROW) break;
          sl = (sl + 1u) & smask;
        }
      }
    }
    __syncthreads();
    if (tid == 0) {
      int32_t* sum = a.summary + static_cast<int64_t>(item) * 6;
      sum[0] = static_cast<int32_t>(total);
      sum[1] = static_cast<int32_t>(rows_done);
      sum[2] = built ? static_cast<int32_t>(s_goals) : 0;
      sum[3] = built ? static_cast<int32_t>(s_dead) : 0;
      sum[4] = built ? max_cost : -1;
      sum[5] = built ? (cost[0] == PW_SOLVE_INF ? -1 : static_cast<int32_t>(cost[0])) : -1;
      a.status[item] = static_cast<uint8_t>(built ? (stored ? PW_SB_BUILT : PW_SB_SUMMARY_ONLY) : status);
      a.state_off[item] = st;
      a.row_off[item] = row;
      a.slot_off[item] = stored ? s_slot : -1;
      a.slot_log2[item] = static_cast<uint8_t>(s_log2);
      if (built && stored) atomicMax(&a.item_of_puzzle[pid], item);  // (a puzzle listed twice: the higher item answers the queries)
    }
  }
}

// ---- query: live states of a mixed batch -> nodes, costs and the best push ---------------------------------------------------
struct PushSolveBatchQueryArgs {
  const PwPuzzleHeader* hdrs;
  const uint8_t* blob;
  const uint64_t* ovl;
  const PwOvlDir* ovl_dir;
  int32_t num_puzzles;
  const int32_t* item_of_puzzle;
  const int64_t* state_off;
  const int64_t* row_off;
  const int64_t* slot_off;
  const uint8_t* slot_log2;
  const unsigned long long* pool_key;
  const int64_t* pool_srow;
  const int32_t* pool_cost;
  const int32_t* pool_best;
  const uint16_t* pool_from;
  const uint8_t* pool_action;
  const uint32_t* pool_slots;
  const int32_t* puzzle_id;  // [n]
  const int8_t* pos;         // [n][npad][2]
  const uint8_t* item_mask;  // or NULL
  int32_t npad, n;
  int32_t* out_index;
  int32_t* out_cost;
  int8_t* out_from;
  uint8_t* out_paction;
  int32_t* out_walk;
  int8_t* out_action;
};

// The walk region of PP from (x0, y0) as a layered breadth-first search, action-major inside a layer: the first discovery of a
// position carries its lowest parent action.  Board 0 visited, 1 the layer, 2 the next layer; with kParent boards 3 / 4 hold the
// 2-bit parent action of the cells x < 8 / x >= 8.  Returns canon as x | y << 4.
template <bool kParent, class P>
__device__ __forceinline__ uint32_t pw_psb_region_layers(const P& p, const PwPuzzleHeader* h, const uint32_t (&OT)[8],
                                                         const uint32_t (&PP)[4], int x0, int y0, uint16_t* b) {
  const int W = h->W, H = h->H, aw = static_cast<int>(OT[0] & 0xffu), ah = static_cast<int>((OT[0] >> 8) & 0xffu);
  for (int y = 0; y < 16; y++) {
    PW_PSB_B(b, 0, y) = 0;
    PW_PSB_B(b, 1, y) = 0;
    PW_PSB_B(b, 2, y) = 0;
    if (kParent) {
      PW_PSB_B(b, 3, y) = 0;
      PW_PSB_B(b, 4, y) = 0;
    }
  }
  PW_PSB_B(b, 0, y0) = static_cast<uint16_t>(1u << x0);
  PW_PSB_B(b, 1, y0) = static_cast<uint16_t>(1u << x0);
  for (int layer = 0; layer < 256; layer++) {
    bool any = false;
#pragma unroll 1
    for (int act = 0; act < 4; act++) {
      const int dx = act == 0 ? -1 : (act == 1 ? 1 : 0), dy = act == 2 ? -1 : (act == 3 ? 1 : 0);
      for (int y = 0; y < 16; y++) {
        uint32_t row = PW_PSB_B(b, 1, y);
        const int ry = y + dy;
        while (row) {
          const int x = __ffs(row) - 1;
          row &= row - 1u;
          const int rx = x + dx;
          // (the verdict of the step is only needed where the walk would reach a new cell of the grid)
          if (rx < 0 || ry < 0 || rx + aw > W || ry + ah > H || rx > 15 || ry > 15) continue;
          const uint32_t seen = PW_PSB_B(b, 0, ry);
          if ((seen >> rx) & 1u) continue;
          LaneEnv<8> s;
          if (pw_psb_step(p, h, OT, PP, x, y, act, s) != 1) continue;
          PW_PSB_B(b, 0, ry) = static_cast<uint16_t>(seen | (1u << rx));
          PW_PSB_B(b, 2, ry) = static_cast<uint16_t>(PW_PSB_B(b, 2, ry) | (1u << rx));
          if (kParent) PW_PSB_B(b, 3 + (rx >> 3), ry) = static_cast<uint16_t>(PW_PSB_B(b, 3 + (rx >> 3), ry) | (static_cast<uint32_t>(act) << (2 * (rx & 7))));
          any = true;
        }
      }
    }
    if (!any) break;
    for (int y = 0; y < 16; y++) {
      PW_PSB_B(b, 1, y) = PW_PSB_B(b, 2, y);
      PW_PSB_B(b, 2, y) = 0;
    }
  }
  for (int y = 0; y < 16; y++) {
    const uint32_t row = PW_PSB_B(b, 0, y);
    if (row) return static_cast<uint32_t>(__ffs(row) - 1) | (static_cast<uint32_t>(y) << 4);
  }
  return static_cast<uint32_t>(x0) | (static_cast<uint32_t>(y0) << 4);
}

__global__ __launch_bounds__(256) void pw_push_solve_batch_query_kernel(PushSolveBatchQueryArgs a) {
  __shared__ uint16_t s_boards[5 * 16 * 256];
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= a.n) return;
  if (a.item_mask && a.item_mask[i] == 0) return;
  const int32_t pid = a.puzzle_id[i];
  if (pid < 0 || pid >= a.num_puzzles) return;
  const int32_t item = a.item_of_puzzle[pid];
  if (item < 0) return;  // no stored table for this puzzle: another table's item, untouched
  uint16_t* const b = s_boards + threadIdx.x;
  const PwPuzzleHeader* h = a.hdrs + pid;
  const int N = h->N, W = h->W, H = h->H;  // (a stored table: N <= 8, W, H <= 16, overlap tables present)
  LanePuzzleT<const uint64_t*, 2> p;
  uint32_t OT[8];
  pw_bs_puzzle(a.hdrs, a.blob, a.ovl, a.ovl_dir, pid, p, OT);
  uint32_t P[4];
  pw_bs_load_row(a.pos + i * a.npad * 2, a.npad, P);
  const bool want_walk = a.out_walk != nullptr || a.out_action != nullptr;
  // the first N movables only: a pos row may hold anything beyond them
  const bool inside = N <= a.npad && pw_psb_in_grid(P, OT, N, W, H);
  const int x0 = static_cast<int>(P[0] & 0xffu), y0 = static_cast<int>((P[0] >> 8) & 0xffu);
  int64_t idx = -1;
  const int64_t sbase = a.state_off[item], rbase = a.row_off[item];
  if (inside) {
    const uint32_t canon = want_walk ? pw_psb_region_layers<true>(p, h, OT, P, x0, y0, b) : pw_psb_region_layers<false>(p, h, OT, P, x0, y0, b);
    const uint64_t key = ((pw_bs_pack(P) & pw_sb_keep(N)) & ~0xffull) | canon;
    idx = pw_sb_probe(a.pool_slots + a.slot_off[item], (1u << a.slot_log2[item]) - 1u, a.pool_key + sbase, key);
  }
  int32_t cost = -2, walk = -1, act = -1;
  uint32_t fxy = 0, pact = 0xFFu;
  if (idx >= 0) {
    cost = a.pool_cost[sbase + idx];
    const int32_t k = a.pool_best[sbase + idx];
    if (k >= 0) {
      const int64_t r = rbase + a.pool_srow[sbase + idx] + k;
      fxy = a.pool_from[r];
      pact = a.pool_action[r];
      if (want_walk) {
        // back from push_from along the parents to the live position: the steps are the walk, the last link the first action
        int x = static_cast<int>(fxy & 0xffu), y = static_cast<int>(fxy >> 8);
        int steps = 0, first = -1;
        bool ok = x < 16 && y < 16;
        for (int t = 0; t < 255 && ok && !(x == x0 && y == y0); t++) {
          if (!((PW_PSB_B(b, 0, y) >> x) & 1u)) {
            ok = false;
            break;
          }
          const int d = (PW_PSB_B(b, 3 + (x >> 3), y) >> (2 * (x & 7))) & 3;
          x -= d == 0 ? -1 : (d == 1 ? 1 : 0);
          y -= d == 2 ? -1 : (d == 3 ? 1 : 0);
          ok = x >= 0 && y >= 0 && x < 16 && y < 16;
          first = d;
          steps++;
        }
        if (ok && x == x0 && y == y0) {
          walk = steps;
          act = steps == 0 ? static_cast<int32_t>(pact) : first;
        }
      }
    }
  }
  if (a.out_index) a.out_index[i] = static_cast<int32_t>(idx);
  if (a.out_cost) a.out_cost[i] = cost;
  if (a.out_from) reinterpret_cast<int16_t*>(a.out_from)[i] = static_cast<int16_t>(fxy);
  if (a.out_paction) a.out_paction[i] = static_cast<uint8_t>(pact);
  if (a.out_walk) a.out_walk[i] = walk;
  if (a.out_action) a.out_action[i] = static_cast<int8_t>(act);
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
// (tests/test_push_solution_batch_host.py builds the head of this struct -- eng .. n -- by hand to reach the "no run yet" checks
//  without a device: keep those six members first and in this order)
struct PwPushSolveBatch {
  PwEngine* eng;
  int64_t states_cap, rows_cap, slots_cap;
  int32_t n_cap, n;  // items the per-item arrays hold / items of the last run (0: no run yet)
  unsigned long long* d_key;
  int64_t* d_srow;
  int32_t* d_cost;
  int32_t* d_best;
  int32_t* d_succ;
  uint16_t* d_from;
  uint8_t* d_action;
  uint8_t* d_flags;
  uint32_t* d_slots;
  uint8_t* d_status;
  int32_t* d_summary;
  int64_t* d_state_off;
  int64_t* d_row_off;
  int64_t* d_slot_off;
  uint8_t* d_slot_log2;
  int32_t* d_item_of_puzzle;
  unsigned long long* d_counters;
  // host copies of the last run's status / summary / offsets, fetched by the first read after it
  bool host_valid;
  std::vector<uint8_t> h_status;
  std::vector<int32_t> h_summary;
  std::vector<int64_t> h_state_off, h_row_off;
  // the cost index of the stored items (pw_push_batch_sample.inc, K26): built on demand, gone with the next run
  bool index_valid;
  int32_t* d_states_by_cost;  // the stored items' states one after the other: item i's at h_ix_off[i]
  uint32_t* d_cost_start;     // ragged: item i's max_cost + 3 words at h_cs_off[i]
  int64_t* d_ix_off;          // [n] each, -1: nothing stored
  int64_t* d_cs_off;
  std::vector<int64_t> h_ix_off, h_cs_off;
  int32_t index_max_cost;     // the largest max_cost over the stored items (-1: none)
};

static void push_solve_batch_index_discard(PwPushSolveBatch* b) {
  void* bufs[] = {b->d_states_by_cost, b->d_cost_start, b->d_ix_off, b->d_cs_off};
  for (void* p : bufs)
    if (p) (void)hipFree(p);
  b->d_states_by_cost = nullptr;
  b->d_cost_start = nullptr;
  b->d_ix_off = nullptr;
  b->d_cs_off = nullptr;
  b->index_valid = false;
  b->index_max_cost = -1;
}

static int push_solve_batch_host_copies(PwPushSolveBatch* b, hipStream_t st, const char* fn) {
  if (b->host_valid) return PW_OK;
  const size_t n = static_cast<size_t>(b->n);
  b->h_status.resize(n);
  b->h_summary.resize(n * 6);
  b->h_state_off.resize(n);
  b->h_row_off.resize(n);
  hipError_t err = hipMemcpyAsync(b->h_status.data(), b->d_status, n, hipMemcpyDeviceToHost, st);
  if (err == hipSuccess) err = hipMemcpyAsync(b->h_summary.data(), b->d_summary, n * 24, hipMemcpyDeviceToHost, st);
  if (err == hipSuccess) err = hipMemcpyAsync(b->h_state_off.data(), b->d_state_off, n * 8, hipMemcpyDeviceToHost, st);
  if (err == hipSuccess) err = hipMemcpyAsync(b->h_row_off.data(), b->d_row_off, n * 8, hipMemcpyDeviceToHost, st);
  if (err == hipSuccess) err = hipStreamSynchronize(st);
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string(fn) + ": " + hipGetErrorString(err));
  b->host_valid = true;
  return PW_OK;
}

static void push_solve_batch_free_items(PwPushSolveBatch* b) {
  void* bufs[] = {b->d_slots, b->d_status, b->d_summary, b->d_state_off, b->d_row_off, b->d_slot_off, b->d_slot_log2};
  for (void* p : bufs)
    if (p) (void)hipFree(p);
  b->d_slots = nullptr;
  b->d_status = nullptr;
  b->d_summary = nullptr;
  b->d_state_off = nullptr;
  b->d_row_off = nullptr;
  b->d_slot_off = nullptr;
  b->d_slot_log2 = nullptr;
  b->n_cap = 0;
  b->slots_cap = 0;
}

// the item's stored table for a read: PW_OK, or the error
static int push_solve_batch_stored(PwPushSolveBatch* b, int32_t item, hipStream_t st, const char* fn) {
  if (int rc = push_solve_batch_host_copies(b, st, fn)) return rc;
  const size_t it = static_cast<size_t>(item);
  if (b->h_status[it] != PW_SB_BUILT || b->h_state_off[it] < 0 || b->h_row_off[it] < 0)
    return pw_fail(PW_EINVAL, std::string(fn) + ": the item has no stored table (status " + std::to_string(b->h_status[it]) + ")");
  return PW_OK;
}

extern "C" {

void pw_push_solve_batch_destroy(PwPushSolveBatch* b) {
  if (!b) return;
  PwDeviceGuard guard(b->eng->set->device);
  push_solve_batch_free_items(b);
  push_solve_batch_index_discard(b);
  void* bufs[] = {b->d_key, b->d_srow, b->d_cost, b->d_best, b->d_succ, b->d_from, b->d_action, b->d_flags, b->d_item_of_puzzle, b->d_counters};
  for (void* p : bufs)
    if (p) (void)hipFree(p);
  delete b;
}

int pw_push_solve_batch_create(PwEngine* e, int64_t states_cap, int64_t rows_cap, PwPushSolveBatch** out) try {
  if (!e) return pw_fail(PW_EINVAL, "pw_push_solve_batch_create: null engine");
  if (!out) return pw_fail(PW_EINVAL, "pw_push_solve_batch_create: null out");
  if (states_cap < 0 || states_cap > (1ll << 40)) return pw_fail(PW_EINVAL, "pw_push_solve_batch_create: states_cap must be in 0 .. 2^40");
  if (rows_cap < 0 || rows_cap > (1ll << 40)) return pw_fail(PW_EINVAL, "pw_push_solve_batch_create: rows_cap must be in 0 .. 2^40");
  if (!e->d_ovl || !e->d_ovl_dir)
    return pw_fail(PW_EINVAL, "pw_push_solve_batch_create needs the engine's overlap tables (PW_OPT_STEP_TABLES)");
  PwPushSolveBatch* b = new (std::nothrow) PwPushSolveBatch();
  if (!b) return pw_fail(PW_ENOMEM, "out of memory");
  b->eng = e;
  b->states_cap = states_cap;
  b->rows_cap = rows_cap;
  PwDeviceGuard guard(e->set->device);
  PwHipChain c(guard.status());
  const size_t ns = static_cast<size_t>(states_cap), nr = static_cast<size_t>(rows_cap);
  c.alloc_nonzero(&b->d_key, ns * 8);
  c.alloc_nonzero(&b->d_srow, ns * 8);
  c.alloc_nonzero(&b->d_cost, ns * 4);
  c.alloc_nonzero(&b->d_best, ns * 4);
  c.alloc_nonzero(&b->d_succ, nr * 4);
  c.alloc_nonzero(&b->d_from, nr * 2);
  c.alloc_nonzero(&b->d_action, nr);
  c.alloc_nonzero(&b->d_flags, nr);
  c.alloc_nonzero(&b->d_item_of_puzzle, static_cast<size_t>(e->set->count) * 4);
  c.alloc_nonzero(&b->d_counters, 32);
  if (!c.ok()) {
    pw_push_solve_batch_destroy(b);
    return pw_hip_fail("pw_push_solve_batch_create", c.err);
  }
  *out = b;
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_push_solve_batch_run(PwPushSolveBatch* b, const int32_t* puzzles, const int8_t* starts, int32_t npad, int32_t n,
                            int64_t max_states_each, void* stream) try {
  if (!b) return pw_fail(PW_EINVAL, "pw_push_solve_batch_run: null handle");
  if (n < 1) return pw_fail(PW_EINVAL, "pw_push_solve_batch_run: n must be >= 1");
  if (max_states_each < 1 || max_states_each > (1ll << 26))
    return pw_fail(PW_EINVAL, "pw_push_solve_batch_run: max_states_each must be in 1 .. 2^26");
  if (starts)
    if (int rc = pw_check_npad("pw_push_solve_batch_run: ", npad)) return rc;
  PwEngine* e = b->eng;
  if (starts && npad < e->set->max_n)
    return pw_fail(PW_EINVAL, "pw_push_solve_batch_run: npad is smaller than the set's largest number of movables");
  PwDeviceGuard guard(e->set->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  b->host_valid = false;
  if (b->index_valid || b->d_states_by_cost) push_solve_batch_index_discard(b);  // (the index is of the last run's tables)
  if (n > b->n_cap) {  // the per-item arrays and the lookup pool (4 slots per state + 16 per item always hold what the states hold)
    if (hipStreamSynchronize(st) != hipSuccess) return pw_fail(PW_EDEVICE, "pw_push_solve_batch_run: stream error");
    push_solve_batch_free_items(b);
    b->n = 0;
    const size_t items = static_cast<size_t>(n);
    const int64_t slots_cap = b->states_cap ? 4 * b->states_cap + 16 * static_cast<int64_t>(n) : 0;
    PwHipChain c;
    c.alloc_nonzero(&b->d_slots, static_cast<size_t>(slots_cap) * 4);
    c.alloc_nonzero(&b->d_status, items);
    c.alloc_nonzero(&b->d_summary, items * 24);
    c.alloc_nonzero(&b->d_state_off, items * 8);
    c.alloc_nonzero(&b->d_row_off, items * 8);
    c.alloc_nonzero(&b->d_slot_off, items * 8);
    c.alloc_nonzero(&b->d_slot_log2, items);
    if (!c.ok()) {
      push_solve_batch_free_items(b);
      return pw_hip_fail("pw_push_solve_batch_run", c.err);
    }
    b->n_cap = n;
    b->slots_cap = slots_cap;
  }
  PushSolveBatchArgs a;
  a.hdrs = e->set->d_headers;
  a.blob = e->set->d_blob;
  a.ovl = e->d_ovl;
  a.ovl_dir = e->d_ovl_dir;
  a.puzzles = puzzles;
  a.starts = starts;
  a.npad = npad;
  a.n = n;
  a.num_puzzles = e->set->count;
  a.max_states = static_cast<uint32_t>(max_states_each);
  a.max_rows = static_cast<uint32_t>(max_states_each * PW_PSB_ROWS_PER_STATE);
  // slab of one workgroup: the state store, the states' first rows, cost, best, the rows (12 bytes each, PW_PSB_ROWS_PER_STATE per
  // state of the cap), then tables of 2^16, 2^20, 2^22 ... slots up to >= 2 * max_states, 12 bytes per slot
  const uint64_t ms = static_cast<uint64_t>(max_states_each), mr = static_cast<uint64_t>(a.max_rows);
  uint64_t off = pw_pad256(ms * 8);
  a.srow_off = off;
  off += pw_pad256((ms + 1) * 4);
  a.cost_off = off;
  off += pw_pad256(ms * 2);
  a.best_off = off;
  off += pw_pad256(ms * 2);
  a.rkey_off = off;
  off += pw_pad256(mr * 8);
  a.rmeta_off = off;
  off += pw_pad256(mr * 4);
  // (+ 256: the inserts in flight when the store fills, at most one per lane beyond max_states)
  a.slab_bytes = pw_pad256(pw_bs_ladder(ms + 256ull, PW_PSB_LDS_SLOTS, 12, off, a.level_slots, a.level_off));
  // persistent workgroups by pw_search_batch's rule; the slabs are the engine's, shared with pw_search_batch
  int64_t groups = 0;
  if (int rc = engine_search_slab(e, n, a.slab_bytes, st, "pw_push_solve_batch_run", &groups, &a.slab, &a.next)) return rc;
  a.counters = b->d_counters;
  a.status = b->d_status;
  a.summary = b->d_summary;
  a.state_off = b->d_state_off;
  a.row_off = b->d_row_off;
  a.slot_off = b->d_slot_off;
  a.slot_log2 = b->d_slot_log2;
  a.item_of_puzzle = b->d_item_of_puzzle;
  a.states_cap = b->states_cap;
  a.rows_cap = b->rows_cap;
  a.slots_cap = b->slots_cap;
  a.pool_key = b->d_key;
  a.pool_srow = b->d_srow;
  a.pool_cost = b->d_cost;
  a.pool_best = b->d_best;
  a.pool_succ = b->d_succ;
  a.pool_from = b->d_from;
  a.pool_action = b->d_action;
  a.pool_flags = b->d_flags;
  a.pool_slots = b->d_slots;
  hipError_t err = hipMemsetAsync(a.next, 0, 4, st);
  if (err == hipSuccess) err = hipMemsetAsync(b->d_counters, 0, 32, st);
  if (err == hipSuccess) err = hipMemsetAsync(b->d_item_of_puzzle, 0xFF, static_cast<size_t>(e->set->count) * 4, st);
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string("pw_push_solve_batch_run: ") + hipGetErrorString(err));
  hipLaunchKernelGGL(pw_push_solve_batch_kernel, dim3(static_cast<unsigned>(groups)), dim3(256), 0, st, a);
  b->n = n;
  return check_launch("pw_push_solve_batch_run");
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_push_solve_batch_results(PwPushSolveBatch* b, const uint8_t** status, const int32_t** summary, const int64_t** state_off,
                                const int64_t** row_off) try {
  if (!b) return pw_fail(PW_EINVAL, "pw_push_solve_batch_results: null handle");
  if (b->n < 1) return pw_fail(PW_EINVAL, "pw_push_solve_batch_results: no run yet (call pw_push_solve_batch_run)");
  if (status) *status = b->d_status;
  if (summary) *summary = b->d_summary;
  if (state_off) *state_off = b->d_state_off;
  if (row_off) *row_off = b->d_row_off;
  return b->n;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_push_solve_batch_copy_results(PwPushSolveBatch* b, uint8_t* status, int32_t* summary, int64_t* state_off, int64_t* row_off,
                                     void* stream) try {
  if (!b) return pw_fail(PW_EINVAL, "pw_push_solve_batch_copy_results: null handle");
  if (b->n < 1) return pw_fail(PW_EINVAL, "pw_push_solve_batch_copy_results: no run yet (call pw_push_solve_batch_run)");
  PwDeviceGuard guard(b->eng->set->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t n = static_cast<size_t>(b->n);
  hipError_t err = hipSuccess;
  if (status) err = hipMemcpyAsync(status, b->d_status, n, hipMemcpyDeviceToDevice, st);
  if (err == hipSuccess && summary) err = hipMemcpyAsync(summary, b->d_summary, n * 24, hipMemcpyDeviceToDevice, st);
  if (err == hipSuccess && state_off) err = hipMemcpyAsync(state_off, b->d_state_off, n * 8, hipMemcpyDeviceToDevice, st);
  if (err == hipSuccess && row_off) err = hipMemcpyAsync(row_off, b->d_row_off, n * 8, hipMemcpyDeviceToDevice, st);
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string("pw_push_solve_batch_copy_results: ") + hipGetErrorString(err));
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_push_solve_batch_totals(PwPushSolveBatch* b, int64_t totals[4], void* stream) try {
  if (!b) return pw_fail(PW_EINVAL, "pw_push_solve_batch_totals: null handle");
  if (!totals) return pw_fail(PW_EINVAL, "pw_push_solve_batch_totals: null totals");
  if (b->n < 1) return pw_fail(PW_EINVAL, "pw_push_solve_batch_totals: no run yet (call pw_push_solve_batch_run)");
  PwDeviceGuard guard(b->eng->set->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  unsigned long long host[4] = {0, 0, 0, 0};
  hipError_t err = hipMemcpyAsync(host, b->d_counters, sizeof(host), hipMemcpyDeviceToHost, st);
  if (err == hipSuccess) err = hipStreamSynchronize(st);
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string("pw_push_solve_batch_totals: ") + hipGetErrorString(err));
  for (int k = 0; k < 4; k++) totals[k] = static_cast<int64_t>(host[k]);
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_push_solve_batch_read_states(PwPushSolveBatch* b, int32_t item, int64_t first, int64_t count, uint64_t* key, int64_t* row_off,
                                    int32_t* cost, int32_t* best, void* stream) try {
  if (!b) return pw_fail(PW_EINVAL, "pw_push_solve_batch_read_states: null handle");
  if (b->n < 1) return pw_fail(PW_EINVAL, "pw_push_solve_batch_read_states: no run yet (call pw_push_solve_batch_run)");
  if (item < 0 || item >= b->n) return pw_fail(PW_EINVAL, "pw_push_solve_batch_read_states: item out of bounds");
  if (first < 0 || count < 0) return pw_fail(PW_EINVAL, "pw_push_solve_batch_read_states: state range out of bounds");
  PwDeviceGuard guard(b->eng->set->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (int rc = push_solve_batch_stored(b, item, st, "pw_push_solve_batch_read_states")) return rc;
  const size_t it = static_cast<size_t>(item);
  if (first + count > b->h_summary[it * 6]) return pw_fail(PW_EINVAL, "pw_push_solve_batch_read_states: state range out of bounds");
  const int64_t base = b->h_state_off[it] + first;
  const size_t c = static_cast<size_t>(count);
  hipError_t err = hipSuccess;
  if (row_off) err = hipMemcpyAsync(row_off, b->d_srow + base, (c + 1) * 8, hipMemcpyDeviceToDevice, st);
  if (err == hipSuccess && c && key) err = hipMemcpyAsync(key, b->d_key + base, c * 8, hipMemcpyDeviceToDevice, st);
  if (err == hipSuccess && c && cost) err = hipMemcpyAsync(cost, b->d_cost + base, c * 4, hipMemcpyDeviceToDevice, st);
  if (err == hipSuccess && c && best) err = hipMemcpyAsync(best, b->d_best + base, c * 4, hipMemcpyDeviceToDevice, st);
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string("pw_push_solve_batch_read_states: ") + hipGetErrorString(err));
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_push_solve_batch_read_rows(PwPushSolveBatch* b, int32_t item, int64_t first, int64_t count, int32_t* succ, int8_t* from,
                                  uint8_t* action, uint8_t* flags, void* stream) try {
  if (!b) return pw_fail(PW_EINVAL, "pw_push_solve_batch_read_rows: null handle");
  if (b->n < 1) return pw_fail(PW_EINVAL, "pw_push_solve_batch_read_rows: no run yet (call pw_push_solve_batch_run)");
  if (item < 0 || item >= b->n) return pw_fail(PW_EINVAL, "pw_push_solve_batch_read_rows: item out of bounds");
  if (first < 0 || count < 0) return pw_fail(PW_EINVAL, "pw_push_solve_batch_read_rows: row range out of bounds");
  PwDeviceGuard guard(b->eng->set->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (int rc = push_solve_batch_stored(b, item, st, "pw_push_solve_batch_read_rows")) return rc;
  const size_t it = static_cast<size_t>(item);
  if (first + count > b->h_summary[it * 6 + 1]) return pw_fail(PW_EINVAL, "pw_push_solve_batch_read_rows: row range out of bounds");
  if (count == 0) return PW_OK;
  const int64_t base = b->h_row_off[it] + first;
  const size_t c = static_cast<size_t>(count);
  hipError_t err = hipSuccess;
  if (succ) err = hipMemcpyAsync(succ, b->d_succ + base, c * 4, hipMemcpyDeviceToDevice, st);
  if (err == hipSuccess && from) err = hipMemcpyAsync(from, b->d_from + base, c * 2, hipMemcpyDeviceToDevice, st);
  if (err == hipSuccess && action) err = hipMemcpyAsync(action, b->d_action + base, c, hipMemcpyDeviceToDevice, st);
  if (err == hipSuccess && flags) err = hipMemcpyAsync(flags, b->d_flags + base, c, hipMemcpyDeviceToDevice, st);
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string("pw_push_solve_batch_read_rows: ") + hipGetErrorString(err));
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_push_solve_batch_query(PwPushSolveBatch* b, const int32_t* puzzle_id, const int8_t* pos, int32_t npad, const uint8_t* mask,
                              int32_t n, int32_t* index, int32_t* cost, int8_t* push_from, uint8_t* push_action, int32_t* walk,
                              int8_t* action, void* stream) try {
  if (!b) return pw_fail(PW_EINVAL, "pw_push_solve_batch_query: null handle");
  if (n < 1) return pw_fail(PW_EINVAL, "pw_push_solve_batch_query: n must be >= 1");
  if (!puzzle_id) return pw_fail(PW_EINVAL, "pw_push_solve_batch_query: null puzzle_id");
  if (!pos) return pw_fail(PW_EINVAL, "pw_push_solve_batch_query: null pos");
  if (int rc = pw_check_npad("pw_push_solve_batch_query: ", npad)) return rc;
  if (b->n < 1) return pw_fail(PW_EINVAL, "pw_push_solve_batch_query: no run yet (call pw_push_solve_batch_run)");
  if (npad < b->eng->set->max_n)
    return pw_fail(PW_EINVAL, "pw_push_solve_batch_query: npad is smaller than the set's largest number of movables");
  PwDeviceGuard guard(b->eng->set->device);
  PushSolveBatchQueryArgs a;
  a.hdrs = b->eng->set->d_headers;
  a.blob = b->eng->set->d_blob;
  a.ovl = b->eng->d_ovl;
  a.ovl_dir = b->eng->d_ovl_dir;
  a.num_puzzles = b->eng->set->count;
  a.item_of_puzzle = b->d_item_of_puzzle;
  a.state_off = b->d_state_off;
  a.row_off = b->d_row_off;
  a.slot_off = b->d_slot_off;
  a.slot_log2 = b->d_slot_log2;
  a.pool_key = b->d_key;
  a.pool_srow = b->d_srow;
  a.pool_cost = b->d_cost;
  a.pool_best = b->d_best;
  a.pool_from = b->d_from;
  a.pool_action = b->d_action;
  a.pool_slots = b->d_slots;
  a.puzzle_id = puzzle_id;
  a.pos = pos;
  a.item_mask = mask;
  a.npad = npad;
  a.n = n;
  a.out_index = index;
  a.out_cost = cost;
  a.out_from = push_from;
  a.out_paction = push_action;
  a.out_walk = walk;
  a.out_action = action;
  const dim3 grid(static_cast<unsigned>((static_cast<int64_t>(n) + 255) / 256)), block(256);
  hipLaunchKernelGGL(pw_push_solve_batch_query_kernel, grid, block, 0, static_cast<hipStream_t>(stream), a);
  return check_launch("pw_push_solve_batch_query");
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

}  // extern "C"

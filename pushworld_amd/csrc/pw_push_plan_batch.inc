// ====================================================================================================
// K24 batched best-first search OVER PUSHES: MANY puzzles' or live states' K17 runs (pw_push_planner.inc) in ONE launch.
// Included from pw_kernels.hip after pw_plan_batch.inc and pw_push_solution_batch.inc (one translation unit).
//
// pw_push_planner_* runs one puzzle with about twenty launches and one host wait per round.  Here, as in pw_plan_batch (K9),
// persistent workgroups of ONE wavefront take items off a device counter and the whole search of an item runs inside the
// kernel; workgroups never wait on each other.  The two halves exist already and are used as they are: the flood of a walk
// region and the push rows on the packed state word are K22's (pw_psb_step, pw_psb_region_lanes, pw_psb_in_grid, pw_bs_pack
// of pw_push_solution_batch.inc, boards of 64 lanes instead of 256), the bucket queue (pb_next_bucket, head / next / bits0 /
// bits1), the tagged closed set, rgd_eval_pos on an LDS stack, the per-item clock and the cancel word are K9's.
// An item's info[0..9], store and links equal pw_push_planner_create + begin + run(max_rounds) with the same K, max_states and
// RGD budget, round by round, as long as no finite key reaches cost_range:
//
//   pop       lane 0: the lowest non-empty buckets, newest entry first, up to K states
//   flood     lane k floods popped state k with push boards (192 B of LDS per lane); T = the wave sum of the push counts;
//             push rows += T; states + T > max_states: PW_PLAN_LIMIT, nothing appended
//   rows      (pop rank, y, x, action) order, 64 at a time, one lane per row: step, range check on the 16-bit fields BEFORE
//             packing, goal test, flood of the successor for its canon and region size; the candidate is the canonical 64-bit
//             key and the agent's byte as reached.  A chunk is claimed before the next is computed: no row buffer in memory
//   claim     lane 0, rows in order: a successor inside its grid whose key is neither closed nor claimed earlier is appended;
//             the first goal row is appended whatever else holds (out of its grid included), ends the store and the search
//   key, push rgd_eval_pos, one lane per new state, on the state as reached; pushes in store order
//
// Slab of one workgroup (reused by the items it takes; sizes from pw_push_plan_batch_create):
//   key       uint64 [max_states]   the canonical key: movable j at bits 8 j (x low nibble, y high), the agent at canon
//   agent     uint8 [max_states]    the agent's byte as reached
//   parent    int32, from uint16 (x | y << 8), action uint8, goal uint8, next int32, each [max_states]
//   table     uint64 [slots]        exact closed set: tag << 32 | index + 1, confirmed against key[index]; an entry of another
//                                   tag is empty, so a new item needs no clearing (every (run, item) pair has its own tag)
//   head      int32 [nb], bits0 / bits1 uint64: K9's buckets (finite 0 .. cost_range - 1, then +inf, then NaN)
//   last      int32 [8]: the item this slab ran last, its states, its N, the index of a goal state outside its grid (-1: none)
//             and that state's 16-bit fields (a packed nibble cannot hold them)
// Every loop is bounded by the items, 256 cells x 4 actions, the slots, max_states, max_rounds or the chain of parents.
// There is no device printf and no device assert.
// ====================================================================================================
static constexpr int kPpbInfo = PW_PUSH_PLAN_BATCH_INFO;
static constexpr int kPpbLanes = PW_WAVE;  // lanes whose boards are interleaved

struct PpbItem {
  RgdEvalArgs rgd;   // the puzzle's RGD tables (unset for a puzzle beyond the limits)
  int32_t pid;       // index in the engine's set
  int32_t eligible;  // within 16 x 16 cells and 8 movables, with overlap tables
};

struct PpbArgs {
  const PwPuzzleHeader* hdrs;
  const uint8_t* blob;
  const uint64_t* ovl;
  const PwOvlDir* ovl_dir;
  const PpbItem* items;
  int32_t n;
  int32_t K;
  int64_t max_states;
  int64_t max_rounds;  // <= 0: no limit
  uint32_t cost_range, nb, n0, n1;
  uint32_t slot_mask;  // table slots - 1
  uint8_t* slab;
  uint64_t slab_bytes;
  uint64_t off_agent, off_parent, off_from, off_action, off_goal, off_next, off_table, off_head, off_bits0, off_bits1, off_last;
  uint64_t time_ticks; // per-item time limit in wall-clock ticks, 0 = none
  uint32_t clock_khz;
  // pinned host words.  [0]: an eager launch is cancelled once cancel[0] >= seq (launches still queued included); a captured
  // launch has seq = INT64_MAX, so no cancel outlives the replay it was meant for.  [1]: the cancel generation, which
  // ppb_begin_kernel copies when a launch or a replay begins: a change since then cancels whatever is running
  const volatile int64_t* cancel;
  int64_t seq;
  uint32_t* next_item;   // the launch's words (PpbWord): the item counter, and the tags that ppb_begin_kernel hands out
  int64_t* info;         // [n][kPpbInfo]
  int32_t* plan_len;     // [n] or NULL
  int8_t* plan_from;     // [n][push_cap][2] or NULL
  uint8_t* plan_action;  // [n][push_cap] or NULL
  int8_t* plan_pos;      // [n][push_cap][npad_out][2] or NULL
  int32_t push_cap, npad_out;
  int32_t levels;        // RGD LDS frames per lane (the largest prepared puzzle's)
  // states form (pw_push_plan_batch_run_states); state_pos == NULL: item i is handle item i from its puzzle's initial state
  const int32_t* state_pid;  // [n] set indices
  const int8_t* state_pos;   // [n][npad][2] start states, or NULL
  const uint8_t* mask;       // [n] or NULL: 0 = skip
  const int32_t* slot_of;    // [set_count] handle item of each set index, -1 = not prepared
  int32_t npad, set_count;
  int8_t* first_from;        // [n][2] or NULL
  uint8_t* first_action;     // [n] or NULL: PW_PUSH_NONE without a non-empty plan
};

enum PpbLast { kPpbLastItem = 0, kPpbLastStates, kPpbLastN, kPpbLastOutside, kPpbLastFields, kPpbLastEpoch = 8 };  // (fields: 4 words)
// the words in front of the slabs: the item counter, the next free tag, this launch's first tag (item i: base + i) and the epoch
// of the tags (bumped when they wrap: a slab of an older epoch empties its table before it is used)
enum PpbWord { kPpbItem = 0, kPpbTagNext, kPpbTagBase, kPpbEpoch, kPpbCancelGen };  // (the generation: an int32 copy)

// One thread in front of every launch, in the same stream: the item counter back to 0 and n fresh tags.  The tags live on the
// device, so a captured launch takes new ones at every replay and never meets the closed-set entries of the replay before.
__global__ void pw_push_plan_batch_begin_kernel(uint32_t* words, uint32_t n, const volatile int64_t* cancel) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  words[kPpbItem] = 0u;
  words[kPpbCancelGen] = static_cast<uint32_t>(cancel[1]);
  uint32_t next = words[kPpbTagNext];
  if (next == 0u) next = 1u;  // (tag 0 is no item's: zeroed tables are empty)
  if (static_cast<unsigned long long>(next) + n >= 0xFFFFFFFFull) {
    words[kPpbEpoch] += 1u;
    next = 1u;
  }
  words[kPpbTagBase] = next;
  words[kPpbTagNext] = next + n;
}

// the state as reached of store entry `idx`: the key with the agent's byte put back, as 16-bit fields
__device__ __forceinline__ void ppb_reached(const unsigned long long* key, const uint8_t* agent, int64_t idx, uint32_t (&P)[4]) {
  pw_bs_unpack((key[idx] & ~0xffull) | agent[idx], P);
}

__device__ __forceinline__ void ppb_skip(const PpbArgs& a, int item, int64_t status) {
  int64_t* info = a.info + static_cast<int64_t>(item) * kPpbInfo;
  info[0] = status;
  for (int k = 1; k < kPpbInfo; k++) info[k] = 0;
  if (status == PW_PLAN_RUNNING) info[5] = info[9] = -1;  // (not started: as a search that ran no round)
  if (a.plan_len) a.plan_len[item] = -1;
  if (a.first_from) a.first_from[2 * item] = a.first_from[2 * item + 1] = 0;
  if (a.first_action) a.first_action[item] = PW_PUSH_NONE;
}

__global__ __launch_bounds__(64) void pw_push_plan_batch_kernel(PpbArgs a) {
  extern __shared__ uint4 ppb_lds[];  // RGD frames [levels][64], then positions uint16 [8][64]
  __shared__ uint16_t s_boards[6 * 16 * kPpbLanes];
  __shared__ uint32_t s_incl[PW_WAVE];
  __shared__ int32_t s_plist[PW_WAVE];
  __shared__ unsigned long long s_ckey[PW_WAVE];
  __shared__ uint4 s_fields[PW_WAVE];  // the successor's 16-bit fields (kept for a goal state outside its grid)
  __shared__ uint32_t s_meta[PW_WAVE];  // from x | y << 8 | action << 16 | goal row << 24 | inside its grid << 25
  __shared__ uint8_t s_abyte[PW_WAVE];
  __shared__ int32_t s_par[PW_WAVE];
  __shared__ int32_t s_rsize[PW_WAVE];
  __shared__ float s_cost[PW_WAVE];
  __shared__ long long s_info[4];
  __shared__ int32_t s_ctl[4];  // the item, the number popped, go on (16 bytes: the dynamic region stays 16-byte aligned)
  int32_t& s_item = s_ctl[0];
  int32_t& s_n = s_ctl[1];
  int32_t& s_go = s_ctl[2];
  const int lane = threadIdx.x;
  uint16_t* const b = s_boards + lane;
  uint8_t* slab = a.slab + static_cast<uint64_t>(blockIdx.x) * a.slab_bytes;
  unsigned long long* key = reinterpret_cast<unsigned long long*>(slab);
  uint8_t* agent = slab + a.off_agent;
  int32_t* parent = reinterpret_cast<int32_t*>(slab + a.off_parent);
  uint16_t* from = reinterpret_cast<uint16_t*>(slab + a.off_from);
  uint8_t* action = slab + a.off_action;
  uint8_t* goalf = slab + a.off_goal;
  int32_t* next = reinterpret_cast<int32_t*>(slab + a.off_next);
  unsigned long long* table = reinterpret_cast<unsigned long long*>(slab + a.off_table);
  int32_t* head = reinterpret_cast<int32_t*>(slab + a.off_head);
  unsigned long long* bits0 = reinterpret_cast<unsigned long long*>(slab + a.off_bits0);
  unsigned long long* bits1 = reinterpret_cast<unsigned long long*>(slab + a.off_bits1);
  int32_t* last = reinterpret_cast<int32_t*>(slab + a.off_last);
  uint4* stk = ppb_lds + lane;
  uint16_t* pos = reinterpret_cast<uint16_t*>(ppb_lds + a.levels * PW_WAVE) + lane;
  if (lane == 0) last[kPpbLastItem] = -1;  // (a launch that runs nothing here leaves no store of an earlier launch to read)
  const uint32_t tag_base = a.next_item[kPpbTagBase], epoch = a.next_item[kPpbEpoch], cancel_gen = a.next_item[kPpbCancelGen];
  auto cancelled = [&]() { return a.cancel[0] >= a.seq || static_cast<uint32_t>(a.cancel[1]) != cancel_gen; };
  if (static_cast<uint32_t>(last[kPpbLastEpoch]) != epoch) {  // the tags wrapped since this slab was used: its table is emptied
    for (uint64_t i = lane; i <= a.slot_mask; i += PW_WAVE) table[i] = 0ull;
    __syncthreads();
    if (lane == 0) last[kPpbLastEpoch] = static_cast<int32_t>(epoch);
    __threadfence_block();
  }
  for (;;) {  // one item per iteration; at most n iterations over all workgroups
    __syncthreads();
    if (lane == 0) s_item = static_cast<int32_t>(atomicAdd(a.next_item, 1u));
    __syncthreads();
    const int item = s_item;
    if (item >= a.n) return;
    // ---- which puzzle, which start; the limits (nothing of a skipped item is read past the test that skips it) ------------
    int slot = item;
    const int8_t* srow = nullptr;
    bool skip = false;
    if (a.state_pos) {
      const int32_t spid = a.state_pid[item];
      skip = (a.mask && a.mask[item] == 0) || spid < 0 || spid >= a.set_count;
      if (!skip) {
        slot = a.slot_of[spid];
        skip = slot < 0;
      }
      srow = a.state_pos + static_cast<int64_t>(item) * a.npad * 2;
    }
    if (!skip) skip = a.items[slot].eligible == 0;
    if (skip) {
      if (lane == 0) ppb_skip(a, item, PW_PLAN_SKIPPED);
      continue;
    }
    const PpbItem& it = a.items[slot];
    const RgdEvalArgs& ra = it.rgd;
    const int pid = it.pid;
    const PwPuzzleHeader* h = a.hdrs + pid;
    const int N = h->N, W = h->W, H = h->H;
    LanePuzzleT<const uint64_t*, 2> p;
    uint32_t OT[8];
    pw_bs_puzzle(a.hdrs, a.blob, a.ovl, a.ovl_dir, pid, p, OT);
    uint32_t P0[4];
    if (srow) pw_bs_load_row(srow, a.npad, P0);
    else pw_bs_load_init(h, P0);
#pragma unroll
    for (int j = 0; j < 8; j++)  // only the first N movables count
      if (j >= N) P0[j >> 1] &= (j & 1) ? 0x0000ffffu : 0u;
    if (!pw_psb_in_grid(P0, OT, N, W, H)) {  // a start outside its grid
      if (lane == 0) ppb_skip(a, item, PW_PLAN_SKIPPED);
      continue;
    }
    if (cancelled()) {
      if (lane == 0) ppb_skip(a, item, PW_PLAN_RUNNING);
      continue;
    }
    const unsigned long long t0 = wall_clock64();
    const uint32_t tag = tag_base + static_cast<uint32_t>(item);
    const uint64_t keep = pw_sb_keep(N);
    uint64_t gkey, gmask;
    pw_bs_goal_word(h, gkey, gmask);
    // ---- begin: the start's canon and region (every lane floods the same state into its own boards), the empty queue -------
    for (uint32_t w = lane; w < a.n0; w += PW_WAVE) bits0[w] = 0ull;
    for (uint32_t w = lane; w < a.n1; w += PW_WAVE) bits1[w] = 0ull;
    const uint32_t canon0 = pw_psb_region_lanes<false, kPpbLanes>(p, h, OT, P0, static_cast<int>(P0[0] & 0xffu),
                                                                   static_cast<int>((P0[0] >> 8) & 0xffu), b);
    int rsize0 = 0;
    for (int y = 0; y < 16; y++) rsize0 += __popc(PW_PSB_BS(b, 0, y, kPpbLanes));
    const uint64_t packed0 = pw_bs_pack(P0) & keep;
    const uint64_t k0 = (packed0 & ~0xffull) | canon0;
    const bool goal0 = (k0 & gmask) == gkey;
    // (lane 0 owns the counters; what the other lanes need of them goes through s_info / s_go / s_n)
    unsigned long long status = goal0 ? PW_PLAN_SOLVED : PW_PLAN_RUNNING;
    unsigned long long rounds = 0, expanded = 0, open = 0, gidx = goal0 ? 0ull : ~0ull, exceeded = 0, push_rows = 0;
    unsigned long long stored = 1, minb = a.nb;
    int32_t largest_region = 0, round_region = rsize0, outside = -1;
    uint32_t maxkey = 0;  // float bits of the largest finite key pushed (0: none)
    if (lane == 0) {
      key[0] = k0;
      agent[0] = static_cast<uint8_t>(packed0 & 0xffull);
      parent[0] = -1;
      from[0] = 0;
      action[0] = PW_PUSH_NONE;
      goalf[0] = goal0 ? 1 : 0;
      table[pw_bs_hash(k0) & a.slot_mask] = (static_cast<unsigned long long>(tag) << 32) | 1ull;  // (an empty table: no probing)
    }
    __threadfence_block();
    __syncthreads();
    int64_t new_first = 0, nnew = goal0 ? 0 : 1;
    int64_t round_no = 0;
    for (;;) {
      // ---- key and push the states [new_first, new_first + nnew), 64 at a time -----------------------------------------------
      for (int64_t k0s = 0; k0s < nnew; k0s += PW_WAVE) {
        const int64_t k = k0s + lane;
        bool over = false;
        if (k < nnew) {
          uint32_t PR[4];
          ppb_reached(key, agent, new_first + k, PR);
          bool on_graph = true;
          for (int j = 0; j < N; j++) {
            const uint32_t f = (PR[j >> 1] >> (16 * (j & 1))) & 0xffffu;
            const int x = f & 0xff, y = f >> 8;
            const bool ok = x < ra.W && y < ra.H && (rgd_mask(ra, j, x, y) & PW_RGD_NODE);
            on_graph = on_graph && ok;
            pos[j * PW_WAVE] = ok ? static_cast<uint16_t>(f) : 0;
          }
          s_cost[lane] = on_graph ? rgd_eval_pos(ra, pos, stk, over) : __builtin_nanf("");
        }
        exceeded += static_cast<unsigned long long>(__popcll(__ballot(over)));
        __syncthreads();
        if (lane == 0) {
          const int cnt = static_cast<int>(nnew - k0s < PW_WAVE ? nnew - k0s : PW_WAVE);
          for (int c = 0; c < cnt && status == PW_PLAN_RUNNING; c++) {
            const float r = s_cost[c];
            uint32_t bk;
            if (r != r) {
              bk = a.nb - 1;
            } else if (isinf(r)) {
              bk = a.nb - 2;
            } else if (r >= static_cast<float>(a.cost_range)) {
              status = PW_PLAN_RANGE;
              break;
            } else {
              bk = static_cast<uint32_t>(r);
              const uint32_t rb = __float_as_uint(r);
              maxkey = rb > maxkey ? rb : maxkey;  // (non-negative floats order as their bits)
            }
            const int32_t idx = static_cast<int32_t>(new_first + k0s + c);
            const bool occupied = (bits0[bk >> 6] >> (bk & 63u)) & 1ull;
            next[idx] = occupied ? head[bk] : -1;
            head[bk] = idx;
            if (!occupied) {
              bits0[bk >> 6] |= 1ull << (bk & 63u);
              bits1[bk >> 12] |= 1ull << ((bk >> 6) & 63u);
            }
            minb = bk < minb ? bk : minb;
          }
        }
        __syncthreads();
      }
      // ---- between rounds: limits, time, cancel; then the pop -------------------------------------------------------------
      if (lane == 0) {
        if (nnew > 0 && status == PW_PLAN_RUNNING) {
          open += static_cast<unsigned long long>(nnew);
          largest_region = round_region > largest_region ? round_region : largest_region;
        }
        round_region = 0;
        int go = status == PW_PLAN_RUNNING && (a.max_rounds <= 0 || round_no < a.max_rounds);
        if (go && a.time_ticks && wall_clock64() - t0 >= a.time_ticks) {
          status = PW_PLAN_TIMEOUT;
          go = 0;
        }
        if (go && round_no > 0 && round_no % kPbCancelRounds == 0 && cancelled()) go = 0;
        int n = 0;
        if (go) {
          round_no++;
          if (open == 0) {
            status = PW_PLAN_EXHAUSTED;
            go = 0;
          } else {
            const int want = static_cast<int>(open < static_cast<unsigned long long>(a.K) ? open : a.K);
            uint32_t bk = pb_next_bucket(a, bits0, bits1, static_cast<uint32_t>(minb));
            while (n < want && bk < a.nb) {
              const int32_t v = head[bk];
              s_plist[n++] = v;
              const int32_t below = next[v];
              head[bk] = below;
              if (below < 0) {
                bits0[bk >> 6] &= ~(1ull << (bk & 63u));
                if (bits0[bk >> 6] == 0ull) bits1[bk >> 12] &= ~(1ull << ((bk >> 6) & 63u));
                if (n < want) bk = pb_next_bucket(a, bits0, bits1, bk + 1);
              }
            }
            minb = bk;
            open -= static_cast<unsigned long long>(n);
            expanded += static_cast<unsigned long long>(n);
            rounds++;
          }
        }
        s_go = go;
        s_n = n;
      }
      __threadfence_block();
      __syncthreads();
      if (!s_go) break;
      const int n = s_n;
      // ---- flood the parents: lane k the popped state k, with push boards ----------------------------------------------------
      uint32_t npush = 0;
      if (lane < n) {
        // from where the agent stands in the state as reached, as K17 floods it: with overlaps a walk need not lead back, so
        // the region seen from canon can be smaller
        uint32_t PP[4];
        ppb_reached(key, agent, s_plist[lane], PP);
        (void)pw_psb_region_lanes<true, kPpbLanes>(p, h, OT, PP, static_cast<int>(PP[0] & 0xffu),
                                                   static_cast<int>((PP[0] >> 8) & 0xffu), b);
        for (int y = 0; y < 16; y++)
          npush += __popc(PW_PSB_BS(b, 2, y, kPpbLanes)) + __popc(PW_PSB_BS(b, 3, y, kPpbLanes)) +
                   __popc(PW_PSB_BS(b, 4, y, kPpbLanes)) + __popc(PW_PSB_BS(b, 5, y, kPpbLanes));
      }
      uint32_t incl = npush;
#pragma unroll
      for (int d = 1; d < PW_WAVE; d <<= 1) {
        const uint32_t t = __shfl_up(incl, d);
        if (lane >= d) incl += t;
      }
      s_incl[lane] = incl;
      const uint32_t T = __shfl(incl, PW_WAVE - 1);  // at most 64 x 1024 rows
      if (lane == 0) {
        push_rows += T;
        const int fits = stored + T <= static_cast<unsigned long long>(a.max_states);
        if (!fits) status = PW_PLAN_LIMIT;
        s_go = fits;
        s_info[0] = s_info[1] = static_cast<long long>(stored);
        s_info[2] = 0;
      }
      __syncthreads();  // s_incl, the push boards of every parent and the verdict are written
      if (!s_go) break;
      const int64_t first = s_info[0];
      bool solved = false;
      // ---- rows, 64 at a time: one lane per row, then the claim of the chunk ------------------------------------------------
      for (uint32_t r0 = 0; r0 < T && !solved; r0 += PW_WAVE) {
        const uint32_t r = r0 + lane;
        if (r < T) {
          int lo = 0, hi = PW_WAVE - 1;  // the parent: the first lane whose inclusive count exceeds r
          while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (s_incl[mid] > r) hi = mid;
            else lo = mid + 1;
          }
          const int j = lo;
          const uint16_t* bj = s_boards + j;
          uint32_t k = r - (j ? s_incl[j - 1] : 0u);
          int y = 0;  // its k-th push in (y, x, action) order
          uint32_t q0 = 0, q1 = 0, q2 = 0, q3 = 0;
          for (; y < 16; y++) {
            q0 = PW_PSB_BS(bj, 2, y, kPpbLanes), q1 = PW_PSB_BS(bj, 3, y, kPpbLanes);
            q2 = PW_PSB_BS(bj, 4, y, kPpbLanes), q3 = PW_PSB_BS(bj, 5, y, kPpbLanes);
            const uint32_t c = __popc(q0) + __popc(q1) + __popc(q2) + __popc(q3);
            if (k < c) break;
            k -= c;
          }
          int x = 0, act = 0;
          bool found = false;
          for (int q = 0; q < 64 && !found; q++) {
            const int qx = q >> 2, qa = q & 3;
            const uint32_t rowbits = qa == 0 ? q0 : (qa == 1 ? q1 : (qa == 2 ? q2 : q3));
            if ((rowbits >> qx) & 1u) {
              if (k == 0u) {
                x = qx, act = qa, found = true;
              } else {
                k--;
              }
            }
          }
          const int32_t pidx = s_plist[j];
          uint32_t PP[4];
          pw_bs_unpack(key[pidx], PP);
          LaneEnv<8> s;
          const int kind = y < 16 && found ? pw_psb_step(p, h, OT, PP, x, y, act, s) : 0;
          uint32_t meta = static_cast<uint32_t>(x) | (static_cast<uint32_t>(y & 15) << 8) | (static_cast<uint32_t>(act) << 16);
          uint64_t ck = 0;
          int rs = 0;
          uint32_t ab = 0;
          if (kind == 2) {  // (always: the boards hold push moves only; anything else is a row that appends nothing)
            if (s.term) meta |= 1u << 24;
            ab = (s.P[0] & 0xfu) | ((s.P[0] >> 4) & 0xf0u);
            if (pw_psb_in_grid(s.P, OT, N, W, H)) {  // the range check on the 16-bit fields BEFORE packing
              meta |= 1u << 25;
              const uint32_t f = s.P[0] & 0xffffu;
              const uint32_t canon =
                  pw_psb_region_lanes<false, kPpbLanes>(p, h, OT, s.P, static_cast<int>(f & 0xffu), static_cast<int>(f >> 8), b);
              for (int yy = 0; yy < 16; yy++) rs += __popc(PW_PSB_BS(b, 0, yy, kPpbLanes));
              ck = ((pw_bs_pack(s.P) & keep) & ~0xffull) | canon;
            }
            s_fields[lane] = make_uint4(s.P[0], s.P[1], s.P[2], s.P[3]);
          }
          s_ckey[lane] = ck;
          s_meta[lane] = meta;
          s_abyte[lane] = static_cast<uint8_t>(ab);
          s_par[lane] = pidx;
          s_rsize[lane] = rs;
        }
        __syncthreads();
        if (lane == 0) {
          const int cnt = static_cast<int>(T - r0 < PW_WAVE ? T - r0 : PW_WAVE);
          for (int c = 0; c < cnt; c++) {
            const uint32_t meta = s_meta[c];
            const bool goal = (meta >> 24) & 1u, inside = (meta >> 25) & 1u;
            if (!goal && !inside) continue;
            const uint64_t ck = s_ckey[c];
            uint32_t sl = pw_bs_hash(ck) & a.slot_mask;
            if (!goal) {
              bool seen = false;
              for (uint32_t probe = 0; probe <= a.slot_mask; probe++) {  // (at most half full: ends at an empty slot)
                const unsigned long long e = table[sl];
                if (static_cast<uint32_t>(e >> 32) != tag) break;
                if (key[static_cast<uint32_t>(e) - 1u] == ck) {
                  seen = true;
                  break;
                }
                sl = (sl + 1u) & a.slot_mask;
              }
              if (seen) continue;
            }
            const int64_t idx = static_cast<int64_t>(stored++);  // (stored + T <= max_states: the store has room)
            key[idx] = ck;
            agent[idx] = s_abyte[c];
            parent[idx] = s_par[c];
            from[idx] = static_cast<uint16_t>(meta & 0xffffu);
            action[idx] = static_cast<uint8_t>((meta >> 16) & 3u);
            goalf[idx] = goal ? 1 : 0;
            if (goal) {  // the first goal row: the last state of the store
              gidx = static_cast<unsigned long long>(idx);
              status = PW_PLAN_SOLVED;
              if (!inside) {
                outside = static_cast<int32_t>(idx);
                const uint4 f = s_fields[c];
                last[kPpbLastFields] = static_cast<int32_t>(f.x);
                last[kPpbLastFields + 1] = static_cast<int32_t>(f.y);
                last[kPpbLastFields + 2] = static_cast<int32_t>(f.z);
                last[kPpbLastFields + 3] = static_cast<int32_t>(f.w);
              }
              break;
            }
            table[sl] = (static_cast<unsigned long long>(tag) << 32) | static_cast<unsigned long long>(idx + 1);
            round_region = s_rsize[c] > round_region ? s_rsize[c] : round_region;
          }
          s_info[1] = static_cast<long long>(stored);
          s_info[2] = status == PW_PLAN_SOLVED ? 1 : 0;
        }
        __threadfence_block();
        __syncthreads();
        solved = s_info[2] != 0;
      }
      new_first = first;
      nnew = solved ? 0 : s_info[1] - first;
    }
    // ---- results ------------------------------------------------------------------------------------------------------------
    if (lane == 0) {
      int64_t* info = a.info + static_cast<int64_t>(item) * kPpbInfo;
      info[0] = static_cast<int64_t>(status);
      info[1] = static_cast<int64_t>(rounds);
      info[2] = static_cast<int64_t>(expanded);
      info[3] = static_cast<int64_t>(stored);
      info[4] = static_cast<int64_t>(open);
      info[5] = gidx == ~0ull ? -1 : static_cast<int64_t>(gidx);
      info[6] = static_cast<int64_t>(exceeded);
      info[7] = static_cast<int64_t>(push_rows);
      info[8] = largest_region;
      info[9] = maxkey == 0u ? -1 : static_cast<int64_t>(__uint_as_float(maxkey));
      info[10] = static_cast<int64_t>((wall_clock64() - t0) * 1000000ull / a.clock_khz);  // nanoseconds
      last[kPpbLastItem] = item;
      last[kPpbLastStates] = static_cast<int32_t>(stored);
      last[kPpbLastN] = N;
      last[kPpbLastOutside] = outside;
      s_info[0] = gidx == ~0ull ? -1 : static_cast<long long>(gidx);
    }
    __threadfence_block();
    __syncthreads();
    // ---- the plan: the chain of parents, written forwards (every lane walks the chain; lane j writes movable j) -----------------
    if (a.plan_len || a.first_action || a.first_from) {
      const int64_t g = s_info[0];
      int32_t len = -1;
      if (g >= 0) {
        len = 0;
        for (int64_t at = g; at > 0 && len <= a.max_states; at = parent[at]) len++;
      }
      const bool arrays = a.plan_from || a.plan_action || a.plan_pos;
      if (arrays && len > a.push_cap) len = -2;
      uint32_t ffrom = 0u, fact = PW_PUSH_NONE;
      int64_t at = g;
      for (int t = len - 1; t >= 0; t--) {
        const int64_t par = parent[at];
        const uint32_t f = from[at];
        if (arrays) {
          const int64_t o = static_cast<int64_t>(item) * a.push_cap + t;
          if (lane == 0) {
            if (a.plan_from) {
              a.plan_from[2 * o] = static_cast<int8_t>(f & 0xffu);
              a.plan_from[2 * o + 1] = static_cast<int8_t>(f >> 8);
            }
            if (a.plan_action) a.plan_action[o] = action[at];
          }
          if (a.plan_pos && lane < a.npad_out) {
            uint32_t PR[4] = {0u, 0u, 0u, 0u};
            ppb_reached(key, agent, par, PR);
            const uint32_t fj = lane < N ? (PR[(lane & 7) >> 1] >> (16 * (lane & 1))) & 0xffffu : 0u;
            int8_t* out = a.plan_pos + (o * a.npad_out + lane) * 2;
            out[0] = static_cast<int8_t>(fj & 0xffu);
            out[1] = static_cast<int8_t>(fj >> 8);
          }
        }
        if (t == 0) ffrom = f, fact = action[at];
        at = par;
      }
      if (lane == 0) {
        if (a.plan_len) a.plan_len[item] = len;
        if (a.first_from) {
          a.first_from[2 * item] = static_cast<int8_t>(ffrom & 0xffu);
          a.first_from[2 * item + 1] = static_cast<int8_t>(ffrom >> 8);
        }
        if (a.first_action) a.first_action[item] = static_cast<uint8_t>(fact);
      }
    }
  }
}

// ---- reads of a slab's store: the states as reached and their canon; the links ------------------------------------------------
struct PpbReadArgs {
  const uint8_t* slab;  // the workgroup's slab
  uint64_t off_agent, off_parent, off_from, off_action, off_goal, off_last;
  int64_t first, count;
  int32_t npad;
  int8_t* pos;      // [count][npad][2] or NULL
  int8_t* canon;    // [count][2] or NULL
  int32_t* parent;  // [count] or NULL
  int8_t* from;     // [count][2] or NULL
  uint8_t* action;  // [count] or NULL
  uint8_t* goal;    // [count] or NULL
};

__global__ __launch_bounds__(256) void pw_push_plan_batch_read_kernel(PpbReadArgs a) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= a.count) return;
  const int64_t idx = a.first + i;
  const unsigned long long* key = reinterpret_cast<const unsigned long long*>(a.slab);
  const int32_t* last = reinterpret_cast<const int32_t*>(a.slab + a.off_last);
  const int N = last[kPpbLastN];
  uint32_t P[4];
  uint32_t canon = static_cast<uint32_t>(key[idx] & 0xffull);
  if (idx == last[kPpbLastOutside]) {  // a goal state outside its grid: its fields as the step left them, canon (0, 0)
    for (int w = 0; w < 4; w++) P[w] = static_cast<uint32_t>(last[kPpbLastFields + w]);
    canon = 0u;
  } else {
    ppb_reached(key, a.slab + a.off_agent, idx, P);
  }
  if (a.pos)
    for (int j = 0; j < a.npad; j++) {
      const uint32_t f = j < N && j < 8 ? (P[j >> 1] >> (16 * (j & 1))) & 0xffffu : 0u;
      a.pos[(i * a.npad + j) * 2] = static_cast<int8_t>(f & 0xffu);
      a.pos[(i * a.npad + j) * 2 + 1] = static_cast<int8_t>(f >> 8);
    }
  if (a.canon) {
    a.canon[2 * i] = static_cast<int8_t>(canon & 15u);
    a.canon[2 * i + 1] = static_cast<int8_t>(canon >> 4);
  }
  if (a.parent) a.parent[i] = reinterpret_cast<const int32_t*>(a.slab + a.off_parent)[idx];
  if (a.from) {
    const uint32_t f = reinterpret_cast<const uint16_t*>(a.slab + a.off_from)[idx];
    a.from[2 * i] = static_cast<int8_t>(f & 0xffu);
    a.from[2 * i + 1] = static_cast<int8_t>(f >> 8);
  }
  if (a.action) a.action[i] = (a.slab + a.off_action)[idx];
  if (a.goal) a.goal[i] = (a.slab + a.off_goal)[idx];
}

// ---- host -------------------------------------------------------------------------------------------------------------------
// (tests/test_push_plan_batch_host.py builds the head of this struct -- eng .. max_n -- by hand to reach the argument checks
//  without a device: keep those four members first and in this order)
struct PwPushPlanBatch {
  PwEngine* eng;
  int32_t n, K, max_n;  // prepared items, states popped per round, the largest prepared eligible puzzle's movables
  int64_t max_states;
  uint32_t cost_range;
  std::vector<PwRgd*> rgd;
  PpbItem* d_items;
  int32_t* d_slot_of;  // [set count] the first item of each set index, -1 = none (the states form)
  PwSlabPool pool;
  int64_t ran_groups;  // workgroups of the last launch (0: no run yet)
  PpbArgs args;        // everything but the per-run fields
  size_t lds;
  PwCancelWord cancel;
};

extern "C" {

void pw_push_plan_batch_destroy(PwPushPlanBatch* b) {
  if (!b) return;
  PwDeviceGuard guard(b->eng->set->device);
  if (b->d_items) (void)hipFree(b->d_items);
  if (b->d_slot_of) (void)hipFree(b->d_slot_of);
  if (b->pool.d_slab) (void)hipFree(b->pool.d_slab);
  cancel_word_destroy(&b->cancel);
  for (PwRgd* r : b->rgd) pw_rgd_destroy(r);
  delete b;
}

int pw_push_plan_batch_create(PwEngine* e, const int32_t* puzzles, int32_t n, int64_t max_states, int32_t batch,
                              int64_t rgd_budget, int32_t cost_range, PwPushPlanBatch** out) try {
  if (!e) return pw_fail(PW_EINVAL, "pw_push_plan_batch_create: null engine");
  if (!out) return pw_fail(PW_EINVAL, "pw_push_plan_batch_create: null out");
  if (n < 1) return pw_fail(PW_EINVAL, "pw_push_plan_batch_create: n must be >= 1");
  if (batch < 1 || batch > kPbMaxK) return pw_fail(PW_EINVAL, "pw_push_plan_batch_create: batch (K) must be in 1 .. 64");
  if (max_states < 1 || max_states > (1ll << 28))
    return pw_fail(PW_EINVAL, "pw_push_plan_batch_create: max_states must be in 1 .. 2^28");
  if (rgd_budget < 0) return pw_fail(PW_EINVAL, "pw_push_plan_batch_create: rgd_budget must be >= 0 (0 = the default)");
  if (cost_range < 0 || cost_range > static_cast<int32_t>(kPbCostRange))
    return pw_fail(PW_EINVAL, "pw_push_plan_batch_create: cost_range must be in 1 .. 65536 (0 = 65536)");
  *out = nullptr;
  if (!pw_puzzles_ok(e, puzzles, n)) return pw_fail(PW_EINVAL, "pw_push_plan_batch_create: puzzle index out of range");
  PwPushPlanBatch* b = new (std::nothrow) PwPushPlanBatch();
  if (!b) return pw_fail(PW_ENOMEM, "pw_push_plan_batch_create: out of memory");
  b->eng = e;
  b->n = n;
  b->K = batch;
  b->max_states = max_states;
  b->cost_range = cost_range > 0 ? static_cast<uint32_t>(cost_range) : kPbCostRange;
  std::vector<PpbItem> items(static_cast<size_t>(n));
  int max_n = 0, levels = 1;
  const bool tables = e->d_ovl && e->d_ovl_dir;
  for (int32_t i = 0; i < n; i++) {  // (one PwRgd per eligible item: a puzzle listed twice is cheap to list twice)
    const int32_t pid = puzzles ? puzzles[i] : i;
    const PwPuzzleHeader& h = e->set->headers[pid];
    PpbItem& it = items[static_cast<size_t>(i)];
    std::memset(static_cast<void*>(&it), 0, sizeof(it));
    it.pid = pid;
    it.eligible = tables && h.N >= 1 && h.N <= 8 && h.W <= 16 && h.H <= 16 && !e->ovl_has.empty() &&
                  e->ovl_has[static_cast<size_t>(pid)];
    if (!it.eligible) continue;
    PwRgd* r = nullptr;
    if (int rc = pw_rgd_create(e, pid, 1, rgd_budget, &r)) {
      pw_push_plan_batch_destroy(b);
      return rc;
    }
    b->rgd.push_back(r);
    it.rgd = rgd_eval_args(r, nullptr, nullptr, 0);
    max_n = std::max<int>(max_n, h.N);
    levels = std::max(levels, std::max(h.N - 2, 1));
  }
  b->max_n = max_n;
  const std::vector<int32_t> slot_of = pw_slot_of(items, e->set->count);
  PpbArgs& a = b->args;
  std::memset(static_cast<void*>(&a), 0, sizeof(a));
  a.hdrs = e->set->d_headers;
  a.blob = e->set->d_blob;
  a.ovl = e->d_ovl;
  a.ovl_dir = e->d_ovl_dir;
  a.n = n;
  a.K = batch;
  a.max_states = max_states;
  a.cost_range = b->cost_range;
  a.nb = b->cost_range + 2u;
  a.n0 = (a.nb + 63u) / 64u;
  a.n1 = (a.n0 + 63u) / 64u;
  const uint64_t ms = static_cast<uint64_t>(max_states), slots = pw_table_slots(ms);
  a.slot_mask = static_cast<uint32_t>(slots - 1u);
  a.levels = levels;
  uint64_t off = pw_pad256(ms * 8);
  a.off_agent = off;
  off += pw_pad256(ms);
  a.off_parent = off;
  off += pw_pad256(ms * 4);
  a.off_from = off;
  off += pw_pad256(ms * 2);
  a.off_action = off;
  off += pw_pad256(ms);
  a.off_goal = off;
  off += pw_pad256(ms);
  a.off_next = off;
  off += pw_pad256(ms * 4);
  a.off_table = off;
  off += pw_pad256(slots * 8);
  a.off_head = off;
  off += pw_pad256(static_cast<uint64_t>(a.nb) * 4);
  a.off_bits0 = off;
  off += pw_pad256(static_cast<uint64_t>(a.n0) * 8);
  a.off_bits1 = off;
  off += pw_pad256(static_cast<uint64_t>(a.n1) * 8);
  a.off_last = off;
  off += 256;
  a.slab_bytes = off;
  b->lds = static_cast<size_t>(PW_WAVE) * (16 * levels + 2 * 8);
  PwDeviceGuard guard(e->set->device);
  PwHipChain c(guard.status());
  slab_pool_create(&b->pool, c, n, e->num_cus, a.slab_bytes);
  c.alloc(&b->d_items, sizeof(PpbItem) * items.size());
  c.alloc(&b->d_slot_of, sizeof(int32_t) * slot_of.size());
  cancel_word_create(&b->cancel, c);
  c.then([&] { return hipMemcpy(b->d_items, items.data(), sizeof(PpbItem) * items.size(), hipMemcpyHostToDevice); });
  c.then([&] { return hipMemcpy(b->d_slot_of, slot_of.data(), sizeof(int32_t) * slot_of.size(), hipMemcpyHostToDevice); });
  c.then([] { return hipDeviceSynchronize(); });
  if (!c.ok()) {
    pw_push_plan_batch_destroy(b);
    return pw_hip_fail("pw_push_plan_batch_create", c.err);
  }
  a.items = b->d_items;
  a.slot_of = b->d_slot_of;
  a.set_count = e->set->count;
  a.slab = b->pool.slabs();
  a.next_item = b->pool.counter();
  a.cancel = b->cancel.d;
  a.clock_khz = pw_wall_clock_khz(e->set->device);
  *out = b;
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

}  // extern "C"

// the checks that both runs share, before anything of the handle but its head is read
static int ppb_check_run(const char* fn, const PwPushPlanBatch* b, double time_limit, const int64_t* info, const int32_t* plan_len,
                         const int8_t* plan_from, const uint8_t* plan_action, const int8_t* plan_pos, int32_t push_cap,
                         int32_t npad) {
  const std::string f(fn);
  if (!b) return pw_fail(PW_EINVAL, f + ": null handle");
  if (!info) return pw_fail(PW_EINVAL, f + ": null info");
  if (!(time_limit >= 0.0)) return pw_fail(PW_EINVAL, f + ": time_limit must be >= 0 seconds (0 = none)");
  if (push_cap < 0) return pw_fail(PW_EINVAL, f + ": push_cap must be >= 0");
  if ((plan_from || plan_action || plan_pos) && !plan_len)
    return pw_fail(PW_EINVAL, f + ": plan_from, plan_action and plan_pos need plan_len");
  if (int rc = pw_check_npad(f + ": ", npad)) return rc;
  if (npad < b->max_n) return pw_fail(PW_EINVAL, f + ": npad is smaller than the largest prepared puzzle's number of movables");
  return PW_OK;
}

// the per-run fields of both forms and the two nodes of a run: the begin kernel (item counter, n fresh tags) and the search
// kernel on at most one workgroup per item.  Nothing here depends on how often the pair is replayed.
static int ppb_launch(PwPushPlanBatch* b, PpbArgs& a, int32_t n, int64_t max_rounds, double time_limit, int64_t* info,
                      int32_t* plan_len, int8_t* plan_from, uint8_t* plan_action, int8_t* plan_pos, int32_t push_cap,
                      int32_t npad_out, hipStream_t st, const char* what) {
  a.n = n;
  a.max_rounds = max_rounds;
  a.time_ticks = pw_deadline_ticks(time_limit, a.clock_khz);
  hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &capturing) != hipSuccess) {
    (void)hipGetLastError();
    capturing = hipStreamCaptureStatusNone;
  }
  a.seq = ++b->cancel.seq;
  if (capturing != hipStreamCaptureStatusNone) a.seq = INT64_MAX;  // (replays: cancelled by the generation alone)
  a.info = info;
  a.plan_len = plan_len;
  a.plan_from = plan_from;
  a.plan_action = plan_action;
  a.plan_pos = plan_pos;
  a.push_cap = push_cap;
  a.npad_out = npad_out;
  hipLaunchKernelGGL(pw_push_plan_batch_begin_kernel, dim3(1), dim3(1), 0, st, a.next_item, static_cast<uint32_t>(n), a.cancel);
  const int64_t groups = std::min<int64_t>(b->pool.groups, n);
  hipLaunchKernelGGL(pw_push_plan_batch_kernel, dim3(static_cast<unsigned>(groups)), dim3(PW_WAVE), b->lds, st, a);
  b->ran_groups = groups;
  return check_launch(what);
}

// the slab that ran `item` last, for a read: PW_OK and the slab, or the error (synchronises `st` for the slabs' last words)
static int ppb_find_slab(PwPushPlanBatch* b, int32_t item, int64_t first, int64_t count, hipStream_t st, const char* fn,
                         const uint8_t** slab) {
  const std::string f(fn);
  std::vector<int32_t> lastw(static_cast<size_t>(b->ran_groups) * 2);
  hipError_t err = hipMemcpy2DAsync(lastw.data(), 8, b->args.slab + b->args.off_last, static_cast<size_t>(b->args.slab_bytes), 8,
                                    static_cast<size_t>(b->ran_groups), hipMemcpyDeviceToHost, st);
  if (err == hipSuccess) err = hipStreamSynchronize(st);
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, f + ": " + hipGetErrorString(err));
  for (int64_t g = 0; g < b->ran_groups; g++) {
    if (lastw[static_cast<size_t>(2 * g)] != item || lastw[static_cast<size_t>(2 * g + 1)] < 1) continue;
    if (first + count > lastw[static_cast<size_t>(2 * g + 1)]) return pw_fail(PW_EINVAL, f + ": state range out of bounds");
    *slab = b->args.slab + static_cast<uint64_t>(g) * b->args.slab_bytes;
    return PW_OK;
  }
  return pw_fail(PW_EINVAL, f + ": the item's store is gone (its workgroup ran another item after it, or the item was not searched)");
}

static int ppb_read(PwPushPlanBatch* b, int32_t item, int64_t first, int64_t count, PpbReadArgs r, void* stream, const char* fn) {
  const std::string f(fn);
  if (!b) return pw_fail(PW_EINVAL, f + ": null handle");
  if (item < 0) return pw_fail(PW_EINVAL, f + ": item out of bounds");
  if (first < 0 || count < 0) return pw_fail(PW_EINVAL, f + ": state range out of bounds");
  if (b->ran_groups < 1) return pw_fail(PW_EINVAL, f + ": no run yet (call pw_push_plan_batch_run)");
  PwDeviceGuard guard(b->eng->set->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const uint8_t* slab = nullptr;
  if (int rc = ppb_find_slab(b, item, first, count, st, fn, &slab)) return rc;
  if (count == 0) return PW_OK;
  const PpbArgs& a = b->args;
  r.slab = slab;
  r.off_agent = a.off_agent;
  r.off_parent = a.off_parent;
  r.off_from = a.off_from;
  r.off_action = a.off_action;
  r.off_goal = a.off_goal;
  r.off_last = a.off_last;
  r.first = first;
  r.count = count;
  hipLaunchKernelGGL(pw_push_plan_batch_read_kernel, dim3(static_cast<unsigned>((count + 255) / 256)), dim3(256), 0, st, r);
  return check_launch(fn);
}

extern "C" {

int pw_push_plan_batch_run(PwPushPlanBatch* b, int64_t max_rounds, double time_limit, int64_t* info, int32_t* plan_len,
                           int8_t* plan_from, uint8_t* plan_action, int8_t* plan_pos, int32_t push_cap, int32_t npad,
                           void* stream) try {
  if (int rc = ppb_check_run("pw_push_plan_batch_run", b, time_limit, info, plan_len, plan_from, plan_action, plan_pos, push_cap, npad))
    return rc;
  PwDeviceGuard guard(b->eng->set->device);
  PpbArgs a = b->args;
  return ppb_launch(b, a, b->n, max_rounds, time_limit, info, plan_len, plan_from, plan_action, plan_pos, push_cap, npad,
                    static_cast<hipStream_t>(stream), "pw_push_plan_batch_run");
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_push_plan_batch_run_states(PwPushPlanBatch* b, const int32_t* puzzle_id, const int8_t* pos, int32_t npad,
                                  const uint8_t* mask, int32_t n, int64_t max_rounds, double time_limit, int64_t* info,
                                  int32_t* plan_len, int8_t* plan_from, uint8_t* plan_action, int8_t* plan_pos, int32_t push_cap,
                                  int8_t* first_from, uint8_t* first_action, void* stream) try {
  const char* fn = "pw_push_plan_batch_run_states";
  if (int rc = ppb_check_run(fn, b, time_limit, info, plan_len, plan_from, plan_action, plan_pos, push_cap, npad)) return rc;
  if (n < 1) return pw_fail(PW_EINVAL, std::string(fn) + ": n must be >= 1");
  if (!puzzle_id) return pw_fail(PW_EINVAL, std::string(fn) + ": null puzzle_id");
  if (!pos) return pw_fail(PW_EINVAL, std::string(fn) + ": null pos");
  PwDeviceGuard guard(b->eng->set->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  bool replaced = false;
  if (int rc = slab_pool_grow(&b->pool, n, b->eng->num_cus, fn, &replaced)) return rc;
  if (replaced) {  // (the counter is zeroed: the tags start again on empty tables)
    b->args.slab = b->pool.slabs();
    b->args.next_item = b->pool.counter();
    b->ran_groups = 0;
  }
  PpbArgs a = b->args;
  a.state_pid = puzzle_id;
  a.state_pos = pos;
  a.mask = mask;
  a.npad = npad;
  a.first_from = first_from;
  a.first_action = first_action;
  return ppb_launch(b, a, n, max_rounds, time_limit, info, plan_len, plan_from, plan_action, plan_pos, push_cap, npad, st, fn);
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_push_plan_batch_read_states(PwPushPlanBatch* b, int32_t item, int64_t first, int64_t count, int8_t* pos, int32_t npad,
                                   int8_t* canon, void* stream) try {
  if (pos)
    if (int rc = pw_check_npad("pw_push_plan_batch_read_states: ", npad)) return rc;
  PpbReadArgs r{};
  r.pos = pos;
  r.npad = npad;
  r.canon = canon;
  return ppb_read(b, item, first, count, r, stream, "pw_push_plan_batch_read_states");
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_push_plan_batch_read_links(PwPushPlanBatch* b, int32_t item, int64_t first, int64_t count, int32_t* parent, int8_t* from,
                                  uint8_t* action, uint8_t* goal, void* stream) try {
  PpbReadArgs r{};
  r.parent = parent;
  r.from = from;
  r.action = action;
  r.goal = goal;
  return ppb_read(b, item, first, count, r, stream, "pw_push_plan_batch_read_links");
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_push_plan_batch_cancel(PwPushPlanBatch* b) try {
  if (!b) return pw_fail(PW_EINVAL, "pw_push_plan_batch_cancel: null handle");
  cancel_word_cancel(&b->cancel);  // every eager launch made so far
  __atomic_store_n(b->cancel.h + 1, b->cancel.h[1] + 1, __ATOMIC_RELEASE);  // and whatever has begun, replays of a capture included
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

}  // extern "C"

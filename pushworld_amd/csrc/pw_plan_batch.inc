// ====================================================================================================
// K9 batched best-first search: MANY puzzles' planner runs (pw_planner.inc) in ONE launch.
// Included after pw_planner.inc (one translation unit).
//
// pw_planner_* runs one puzzle with about ten launches per round, so at K = 1 a round costs the launch floor while the GPU
// idles.  Here, as in pw_search_batch (K5b), persistent workgroups of ONE wavefront take puzzles off a device counter, and
// the whole search of a puzzle -- pop, expand, closed set, goal test, novelty, RGD, push -- runs inside the kernel.
// Workgroups never wait on each other.  A puzzle's result (info[0..7], plan) equals pw_planner_create + begin +
// run(max_rounds) with the same mode, K, action order, max_states and RGD budget, round by round:
//
//   pop       lane 0: the lowest non-empty buckets, newest entry first, up to K of them; the action group of each
//   expand    32 lanes per parent (the lane-group step of pw_search_expand_kernel, lane = movable): 4 candidates each, in
//             (pop rank, position in the action group) order
//   claim     lane 0, candidates in order: a moved candidate whose state is neither stored nor held by an earlier candidate
//             is appended to the store; the first new goal ends the search (solved; the rest of the round is stored too)
//   novelty   N+RGD: every new state in store order, one atomicOr per atom (lanes over the (moved object, object) pairs):
//             fetch-or is the test and the insertion at once, so the tables are plain bits
//   RGD       one lane per new state (rgd_eval_pos, the recursion on an LDS stack)
//   push      lane 0, store order: each state on top of its bucket's stack (a linked list through `next`)
//
// Slab of one workgroup (reused by the puzzles it takes; sizes from pw_plan_batch_create):
//   store     uint32 [max_states][nw]   x | y << 8 per movable, two per word
//   parent    int32 [max_states], action uint8 [max_states]
//   next      int32 [max_states]        the state below in its bucket's stack
//   table     uint64 [slots]            exact closed set: tag << 32 | index + 1; an entry of another tag is empty, so a
//                                       new puzzle needs no clearing (every (run, item) pair has its own tag)
//   head      int32 [nb]                top of bucket b (valid while its occupancy bit is set)
//   bits0/1   uint64                    occupancy: bit b of level 0 = bucket b non-empty, bit w of level 1 = word w != 0
//   cand      uint32 [4 K][nw]          the round's candidates
//   nov       uint32 [...]              N+RGD: single [N][D] and pair [N (N - 1) / 2][D][D] bits (D = W * H), cleared per puzzle
// Buckets: finite costs 0 .. cost_range - 1 (RGD), or (novelty - 1) * cost_range + cost (N+RGD), then +inf (nb - 2) and
// NaN (nb - 1).  A finite cost at or above cost_range ends that puzzle with PW_PLAN_RANGE.
// Between rounds: the wall clock against the per-puzzle time limit (PW_PLAN_TIMEOUT) and, every kPbCancelRounds rounds,
// the cancel word in pinned host memory (the search stops as it stands: status running).
//
// States form (pw_plan_batch_run_states, state_pos != NULL): item i of the run is (state_pid[i], state_pos[i]) in the
// engine's layout (int8 [n][npad][2], x then y: byte for byte the store's x | y << 8).  It searches with the tables of the
// handle item slot_of[pid] prepared, from state_pos[i] in place of the puzzle's initial state.  An item that is masked out,
// names a puzzle outside the set or one the handle did not prepare, or has a movable outside its grid (pw_validate_state's
// range test) is PW_PLAN_SKIPPED: nothing of it is read past that test.
// ====================================================================================================
static constexpr int kPbMaxK = 64;             // states popped per round at most (4 K candidates in LDS)
static constexpr uint32_t kPbCostRange = 65536u;  // default and largest cost_range
static constexpr int kPbCancelRounds = 32;     // rounds between two reads of the cancel word
static constexpr int kPbInfo = PW_PLAN_BATCH_INFO;

struct PbItem {
  RgdEvalArgs rgd;  // the puzzle's RGD tables (states / cost / count / exceeded unused)
  int32_t pid;      // index in the engine's set
  int32_t nov_words;  // N+RGD: uint32 words of novelty bits
};

// the start of a states-form item: (x, y) of movable j as the store's x | y << 8 (bytes: any alignment of state_pos)
__device__ __forceinline__ uint32_t pb_start_xy(const int8_t* row, int j) {
  return static_cast<uint32_t>(static_cast<uint8_t>(row[2 * j])) | (static_cast<uint32_t>(static_cast<uint8_t>(row[2 * j + 1])) << 8);
}

struct PbArgs {
  const PwPuzzleHeader* hdrs;
  const uint8_t* blob;
  const PbItem* items;
  int32_t n;
  int32_t mode, K;
  const uint8_t* groups;  // [kPlanGroups] packed action groups, or NULL (L R U D)
  int64_t max_states;
  int64_t max_rounds;     // <= 0: no limit
  uint32_t cost_range, nb, n0, n1;
  uint32_t slot_mask;     // table slots - 1
  int32_t nw;             // words per stored state (the largest puzzle's)
  uint8_t* slab;
  uint64_t slab_bytes;
  uint64_t off_parent, off_action, off_next, off_table, off_head, off_bits0, off_bits1, off_cand, off_nov;
  uint32_t tag_base;      // tag of item i: tag_base + i
  uint64_t time_ticks;    // per-puzzle time limit in wall-clock ticks, 0 = none
  uint32_t clock_khz;
  const volatile int64_t* cancel;  // pinned host word: this launch is cancelled once *cancel >= seq
  int64_t seq;
  uint32_t* next_item;
  int64_t* info;          // [n][kPbInfo]
  uint8_t* plans;         // [n][plan_cap] or NULL
  int32_t* plan_len;      // [n] or NULL
  int32_t plan_cap;
  int32_t levels;         // RGD LDS frames per lane (the largest puzzle's)
  // states form (pw_plan_batch_run_states); state_pos == NULL: item i is handle item i from its puzzle's initial state
  const int32_t* state_pid;  // [n] set indices
  const int8_t* state_pos;   // [n][npad][2] start states, or NULL
  const uint8_t* mask;       // [n] or NULL: 0 = skip
  const int32_t* slot_of;    // [set_count] handle item of each set index, -1 = not prepared
  int32_t npad, set_count;
  int8_t* first_action;      // [n] or NULL: plan[0], -1 without a non-empty plan
};

__device__ __forceinline__ uint32_t pb_hash(const uint32_t* w, int nw) {
  uint32_t t = 0x811C9DC5u;
  for (int k = 0; k < nw; k++) t = search_final(t ^ w[k]) + 0x9E3779B9u;
  return search_final(t);
}

// lowest non-empty bucket >= b, nb when there is none (lane-serial; level 1 has at most 64 words)
template <class A>  // (PbArgs, or pw_push_plan_batch.inc's arguments: nb, n0, n1)
__device__ uint32_t pb_next_bucket(const A& a, const unsigned long long* bits0, const unsigned long long* bits1, uint32_t b) {
  uint32_t w0 = b >> 6;
  if (w0 >= a.n0) return a.nb;
  unsigned long long m = bits0[w0] & (~0ull << (b & 63u));
  if (m) return (w0 << 6) + static_cast<uint32_t>(__ffsll(static_cast<long long>(m)) - 1);
  for (uint32_t w1 = (w0 + 1) >> 6; w1 < a.n1; w1++) {
    m = bits1[w1];
    if (w1 == ((w0 + 1) >> 6)) m &= ~0ull << ((w0 + 1) & 63u);
    if (m) {
      w0 = (w1 << 6) + static_cast<uint32_t>(__ffsll(static_cast<long long>(m)) - 1);
      return (w0 << 6) + static_cast<uint32_t>(__ffsll(static_cast<long long>(bits0[w0])) - 1);
    }
  }
  return a.nb;
}

// N+RGD novelty of one state (all lanes; xy: its stored positions, x | y << 8, position index y * W + x):
// 1 when a moved movable stands where it never stood, 2 when a (moved movable, movable) pair of positions is new, else 3.
// Every atom of the moved movables is inserted.
__device__ int pb_novelty(uint32_t* bits, int N, int D, int lane, uint32_t moved, const uint16_t* xy, int W) {
  bool new1 = false, new2 = false;
  for (int t = lane; t < N * N; t += PW_WAVE) {
    const int i = t / N, j = t - i * N;
    if (!((moved >> i) & 1u)) continue;
    const int pi = (xy[i] >> 8) * W + (xy[i] & 0xff), pj = (xy[j] >> 8) * W + (xy[j] & 0xff);
    int64_t bit;
    if (i == j) {
      bit = static_cast<int64_t>(i) * D + pi;
    } else {
      const int lo = i < j ? i : j, hi = i < j ? j : i;
      const int pid = lo * N - (lo * (lo + 1)) / 2 + (hi - lo - 1);
      bit = static_cast<int64_t>(N) * D + static_cast<int64_t>(pid) * D * D + static_cast<int64_t>(lo == i ? pi : pj) * D +
            (lo == i ? pj : pi);
    }
    const uint32_t m = 1u << (bit & 31);
    const bool fresh = (atomicOr(&bits[bit >> 5], m) & m) == 0u;
    new1 = new1 || (fresh && i == j);
    new2 = new2 || (fresh && i != j);
  }
  if (__ballot(new1)) return 1;
  return __ballot(new2) ? 2 : 3;
}

__global__ __launch_bounds__(64) void pw_plan_batch_kernel(PbArgs a) {
  extern __shared__ uint4 pb_lds[];  // RGD frames [levels][64], then positions uint16 [32][64]
  __shared__ int32_t s_plist[kPbMaxK];
  __shared__ uint8_t s_pperm[kPbMaxK];
  __shared__ uint32_t s_moved[4 * kPbMaxK];  // moved-movable mask of each candidate, 0 = did not move
  __shared__ uint8_t s_goal[4 * kPbMaxK];
  __shared__ int16_t s_cand[4 * kPbMaxK];    // candidate of each new state of the round
  __shared__ uint8_t s_nov[4 * kPbMaxK];
  __shared__ float s_cost[4 * kPbMaxK];
  __shared__ unsigned long long s_info[8];
  __shared__ int32_t s_item, s_n, s_go;
  const int lane = threadIdx.x;
  uint8_t* slab = a.slab + static_cast<uint64_t>(blockIdx.x) * a.slab_bytes;
  uint32_t* store = reinterpret_cast<uint32_t*>(slab);
  int32_t* parent = reinterpret_cast<int32_t*>(slab + a.off_parent);
  uint8_t* action = slab + a.off_action;
  int32_t* next = reinterpret_cast<int32_t*>(slab + a.off_next);
  unsigned long long* table = reinterpret_cast<unsigned long long*>(slab + a.off_table);
  int32_t* head = reinterpret_cast<int32_t*>(slab + a.off_head);
  unsigned long long* bits0 = reinterpret_cast<unsigned long long*>(slab + a.off_bits0);
  unsigned long long* bits1 = reinterpret_cast<unsigned long long*>(slab + a.off_bits1);
  uint32_t* cand = reinterpret_cast<uint32_t*>(slab + a.off_cand);
  uint32_t* nov = reinterpret_cast<uint32_t*>(slab + a.off_nov);
  uint4* stk = pb_lds + lane;
  uint16_t* pos = reinterpret_cast<uint16_t*>(pb_lds + a.levels * PW_WAVE) + lane;
  const int nw = a.nw;
  for (;;) {  // one puzzle per iteration; at most n iterations over all workgroups
    __syncthreads();
    if (lane == 0) s_item = static_cast<int32_t>(atomicAdd(a.next_item, 1u));
    __syncthreads();
    const int item = s_item;
    if (item >= a.n) return;
    int slot = item;
    const int8_t* srow = nullptr;  // states form: the item's start state
    if (a.state_pos) {
      const int32_t spid = a.state_pid[item];
      bool skip = (a.mask && a.mask[item] == 0) || spid < 0 || spid >= a.set_count;
      if (!skip) {
        slot = a.slot_of[spid];
        skip = slot < 0;
      }
      if (!skip) {  // every movable inside the grid (lanes over movables; nothing past N is read)
        const PwPuzzleHeader* sh = a.hdrs + spid;
        srow = a.state_pos + static_cast<int64_t>(item) * a.npad * 2;
        bool bad = false;
        if (lane < sh->N) {
          const int x = srow[2 * lane], y = srow[2 * lane + 1];
          bad = x < 0 || y < 0 || x + sh->objtab[lane].w > sh->W || y + sh->objtab[lane].h > sh->H;
        }
        skip = __ballot(bad) != 0ull;
      }
      if (skip) {
        if (lane == 0) {
          int64_t* sinfo = a.info + static_cast<int64_t>(item) * kPbInfo;
          sinfo[0] = PW_PLAN_SKIPPED;
          for (int k = 1; k < kPbInfo; k++) sinfo[k] = 0;
          if (a.plan_len) a.plan_len[item] = -1;
          if (a.first_action) a.first_action[item] = -1;
        }
        continue;
      }
    }
    const PbItem& it = a.items[slot];
    const RgdEvalArgs& ra = it.rgd;
    const PwPuzzleHeader* h = a.hdrs + it.pid;
    const int N = h->N, G = h->G, W = h->W, D = h->W * h->H;
    const uint32_t tag = a.tag_base + static_cast<uint32_t>(item);
    int64_t* info = a.info + static_cast<int64_t>(item) * kPbInfo;
    const bool cancelled = *a.cancel >= a.seq;
    if (cancelled) {  // not started: as a search that ran no round
      if (lane == 0) {
        info[0] = PW_PLAN_RUNNING;
        for (int k = 1; k < kPbInfo; k++) info[k] = 0;
        info[5] = -1;
        if (a.plan_len) a.plan_len[item] = -1;
        if (a.first_action) a.first_action[item] = -1;
      }
      continue;
    }
    const unsigned long long t0 = wall_clock64();
    // ---- begin: store the start state, clear the queue (and the novelty bits) -------------------------------------------
    for (uint32_t w = lane; w < a.n0; w += PW_WAVE) bits0[w] = 0ull;
    for (uint32_t w = lane; w < a.n1; w += PW_WAVE) bits1[w] = 0ull;
    if (a.mode == PW_PLAN_N_RGD)
      for (int w = lane; w < it.nov_words; w += PW_WAVE) nov[w] = 0u;
    const uint16_t* init = reinterpret_cast<const uint16_t*>(h->init);
    const uint16_t* goal = reinterpret_cast<const uint16_t*>(h->goal);
    // (words and halves past this puzzle's movables are 0, in the store and in the candidates: a slab serves puzzles of
    //  every size, and the closed set compares all nw words)
    auto start = [&](int j) -> uint32_t { return srow ? pb_start_xy(srow, j) : static_cast<uint32_t>(init[j]); };
    if (lane < nw)
      store[lane] = (2 * lane < N ? start(2 * lane) : 0u) | (2 * lane + 1 < N ? start(2 * lane + 1) << 16 : 0u);
    if (lane == 0) s_cand[0] = -1;  // the start state is scored like a round's new state, with every movable moved
    int at_goal = 0;
    for (int g = 0; g < G; g++) at_goal += start(g + 1) == static_cast<uint32_t>(goal[g]);
    // info slots as pw_planner's: status, rounds, expanded, visited, open, goal, rgd overruns, store size
    unsigned long long status = at_goal == G ? PW_PLAN_SOLVED : PW_PLAN_RUNNING;
    unsigned long long rounds = 0, expanded = 0, visited = 1, open = 0, gidx = at_goal == G ? 0ull : ~0ull, exceeded = 0;
    unsigned long long stored = 1, minb = a.nb;
    __threadfence_block();
    __syncthreads();
    if (lane == 0) {
      parent[0] = -1;
      action[0] = 0;
      const uint32_t hsh = pb_hash(store, nw);
      table[hsh & a.slot_mask] = (static_cast<unsigned long long>(tag) << 32) | 1ull;  // (an empty table: no probing)
    }
    int64_t new_first = 0, nnew = status == PW_PLAN_RUNNING ? 1 : 0;
    int64_t round_no = 0;
    for (;;) {
      // ---- score and push the states [new_first, new_first + nnew) ----------------------------------------------------
      if (nnew > 0) {
        if (a.mode == PW_PLAN_N_RGD) {
          for (int k = 0; k < nnew; k++) {
            const int c = s_cand[k];
            const uint32_t mv = c < 0 ? (N >= 32 ? 0xFFFFFFFFu : ((1u << N) - 1u)) : s_moved[c];
            const int v = pb_novelty(nov, N, D, lane, mv, reinterpret_cast<const uint16_t*>(store + (new_first + k) * nw), W);
            if (lane == 0) s_nov[k] = static_cast<uint8_t>(c < 0 ? 1 : v);
          }
        }
        for (int k0 = 0; k0 < nnew; k0 += PW_WAVE) {  // RGD: one lane per new state
          const int k = k0 + lane;
          bool over = false;
          if (k < nnew) {
            const uint16_t* xy = reinterpret_cast<const uint16_t*>(store + (new_first + k) * nw);
            bool on_graph = true;
            for (int j = 0; j < N; j++) {
              const int x = xy[j] & 0xff, y = xy[j] >> 8;
              const bool ok = x < ra.W && y < ra.H && (rgd_mask(ra, j, x, y) & PW_RGD_NODE);
              on_graph = on_graph && ok;
              pos[j * PW_WAVE] = ok ? xy[j] : 0;
            }
            s_cost[k] = on_graph ? rgd_eval_pos(ra, pos, stk, over) : __builtin_nanf("");
          }
          exceeded += static_cast<unsigned long long>(__popcll(__ballot(over)));
        }
        __syncthreads();
        if (lane == 0) {  // keys, pushes in store order
          for (int k = 0; k < nnew && status == PW_PLAN_RUNNING; k++) {
            const float r = s_cost[k];
            uint32_t b;
            if (r != r) {
              b = a.nb - 1;
            } else if (isinf(r)) {
              b = a.nb - 2;
            } else if (r >= static_cast<float>(a.cost_range)) {
              status = PW_PLAN_RANGE;
              break;
            } else {
              b = static_cast<uint32_t>(r);
              if (a.mode == PW_PLAN_N_RGD) b += (static_cast<uint32_t>(s_nov[k]) - 1u) * a.cost_range;
            }
            const int32_t idx = static_cast<int32_t>(new_first + k);
            const bool occupied = (bits0[b >> 6] >> (b & 63u)) & 1ull;
            next[idx] = occupied ? head[b] : -1;
            head[b] = idx;
            if (!occupied) {
              bits0[b >> 6] |= 1ull << (b & 63u);
              bits1[b >> 12] |= 1ull << ((b >> 6) & 63u);
            }
            minb = b < minb ? b : minb;
          }
          if (status == PW_PLAN_RUNNING) open += static_cast<unsigned long long>(nnew);
        }
      }
      // ---- between rounds: limits, time, cancel ---------------------------------------------------------------------
      if (lane == 0) {
        int go = status == PW_PLAN_RUNNING && (a.max_rounds <= 0 || round_no < a.max_rounds);
        if (go && a.time_ticks && wall_clock64() - t0 >= a.time_ticks) {
          status = PW_PLAN_TIMEOUT;
          go = 0;
        }
        if (go && round_no > 0 && round_no % kPbCancelRounds == 0 && *a.cancel >= a.seq) go = 0;
        int n = 0;
        if (go) {  // ---- pop ----
          round_no++;
          if (stored + 4ull * static_cast<unsigned long long>(a.K) > static_cast<unsigned long long>(a.max_states)) {
            status = PW_PLAN_LIMIT;
            go = 0;
          } else if (open == 0) {
            status = PW_PLAN_EXHAUSTED;
            go = 0;
          } else {
            const int want = static_cast<int>(open < static_cast<unsigned long long>(a.K) ? open : a.K);
            uint32_t b = pb_next_bucket(a, bits0, bits1, static_cast<uint32_t>(minb));
            while (n < want && b < a.nb) {
              const int32_t v = head[b];
              s_plist[n] = v;
              // RandomActionIterator::next() advances before it returns: global pop p takes group (p + 1) mod 1000
              s_pperm[n] = a.groups ? a.groups[(expanded + static_cast<unsigned long long>(n) + 1ull) % kPlanGroups] : 0xE4u;
              n++;
              const int32_t below = next[v];
              head[b] = below;
              if (below < 0) {
                bits0[b >> 6] &= ~(1ull << (b & 63u));
                if (bits0[b >> 6] == 0ull) bits1[b >> 12] &= ~(1ull << ((b >> 6) & 63u));
                if (n < want) b = pb_next_bucket(a, bits0, bits1, b + 1);
              }
            }
            minb = b;
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
      // ---- expand: 32 lanes per parent, two parents at a time ---------------------------------------------------------
      for (int r0 = 0; r0 < n; r0 += 2) {
        constexpr int GS = 32;
        const int lj = lane & (GS - 1), gbase = lane & ~(GS - 1);
        const unsigned long long gmask = 0xFFFFFFFFull << gbase;
        const int rank = r0 + (lane >> 5);
        const bool live = rank < n;
        const int64_t pidx = live ? s_plist[rank] : 0;
        const uint32_t perm = live ? s_pperm[rank] : 0xE4u;
        uint32_t slot_of = 0u;  // 2-bit candidate slot of each action
        for (int p = 0; p < 4; p++) slot_of |= static_cast<uint32_t>(p) << (2 * ((perm >> (2 * p)) & 3u));
        LanePuzzleT<const uint64_t*, 0> p;
        p.h = h;
        {
          const uint8_t* bb = a.blob + h->base;
          p.wall = reinterpret_cast<const uint64_t*>(bb + h->off_wall);
          p.awall = reinterpret_cast<const uint64_t*>(bb + h->off_awall);
          p.shapes = reinterpret_cast<const uint64_t*>(bb + h->off_shapes);
        }
        lane_tables(p, nullptr, nullptr, it.pid);
        p.H = h->H;
        p.N = N;
        p.G = G;
        const uint16_t* srow = reinterpret_cast<const uint16_t*>(store + pidx * nw);
        const uint64_t* smalls = reinterpret_cast<const uint64_t*>(a.blob + h->base + h->off_small);
        const int xy = (lj < N) ? static_cast<int>(srow[lj]) : 0;
        const uint32_t ot = (lj < N) ? reinterpret_cast<const uint32_t*>(h->objtab)[lj] : 0u;
        const uint64_t small = (lj < N) ? smalls[lj] : 0ull;
        const bool is_goal_lane = lj >= 1 && lj <= G;
        const int gxy = is_goal_lane ? static_cast<int>(goal[lj - 1]) : -1;
        const LaneSlot s0 = lane_slot(xy, ot, small);
        const LaneSlot s1 = lane_slot(0, 0u, 0ull);
        const uint32_t agent_blocked = group_agent_blocked4<GS>(p, xy, ot, small, lj, gbase, gmask, live);
        const LaneObj ag = lane_obj(static_cast<uint32_t>(__shfl(static_cast<int>(ot), gbase, PW_WAVE)), __shfl(xy, gbase, PW_WAVE));
        const uint64_t asmall = __shfl(static_cast<unsigned long long>(small), gbase, PW_WAVE);
        const uint32_t hit4 = agent_pushes4(p, ag, asmall, s0, lj, live && lj >= 1 && lj < N);
#pragma unroll 1
        for (int act = 0; act < 4; act++) {
          const int dx = act == 0 ? -1 : (act == 1 ? 1 : 0);
          const int dy = act == 2 ? -1 : (act == 3 ? 1 : 0);
          const uint32_t pushed = group_push_closure_swept<GS, false>(p, s0, s1, hit4, 0u, lj, gbase, gmask, live,
                                                                      ((agent_blocked >> act) & 1u) != 0u, act, dx, dy);
          const bool moved = live && pushed != 0u;
          int nxy = xy;
          if (moved && ((pushed >> lj) & 1u)) {
            const int x = static_cast<int8_t>(xy & 0xff) + dx, y = static_cast<int8_t>((xy >> 8) & 0xff) + dy;
            nxy = (x & 0xff) | ((y & 0xff) << 8);
          }
          const int after = __popcll(__ballot(is_goal_lane && nxy == gxy) & gmask);
          const int hi = __shfl_down(nxy, 1, PW_WAVE);
          const int c = rank * 4 + static_cast<int>((slot_of >> (2 * act)) & 3u);
          if (live && lj == 0) {
            s_moved[c] = moved ? pushed : 0u;
            s_goal[c] = static_cast<uint8_t>(moved && after == G);
          }
          if (moved && !(lj & 1) && lj < 2 * nw)
            cand[c * nw + (lj >> 1)] = lj < N ? static_cast<uint32_t>(nxy) | (lj + 1 < N ? static_cast<uint32_t>(hi) << 16 : 0u) : 0u;
        }
      }
      __threadfence_block();
      __syncthreads();
      // ---- claim: new states in candidate order -----------------------------------------------------------------------
      if (lane == 0) {
        const int64_t first = static_cast<int64_t>(stored);
        int k = 0;
        for (int c = 0; c < 4 * n; c++) {
          if (!s_moved[c]) continue;
          const uint32_t* my = cand + c * nw;
          uint32_t slot = pb_hash(my, nw) & a.slot_mask;
          bool seen = false;
          for (uint32_t probe = 0; probe <= a.slot_mask; probe++) {  // (at most half full: ends at an empty slot)
            const unsigned long long e = table[slot];
            if (static_cast<uint32_t>(e >> 32) != tag) break;
            const uint32_t* other = store + static_cast<int64_t>(static_cast<uint32_t>(e) - 1u) * nw;
            bool eq = true;
            for (int w = 0; w < nw; w++) eq = eq && my[w] == other[w];
            if (eq) {
              seen = true;
              break;
            }
            slot = (slot + 1u) & a.slot_mask;
          }
          if (seen) continue;
          const int64_t idx = static_cast<int64_t>(stored++);
          for (int w = 0; w < nw; w++) store[idx * nw + w] = my[w];
          parent[idx] = s_plist[c >> 2];
          action[idx] = static_cast<uint8_t>((s_pperm[c >> 2] >> (2 * (c & 3))) & 3u);
          table[slot] = (static_cast<unsigned long long>(tag) << 32) | static_cast<unsigned long long>(idx + 1);
          if (s_goal[c] && gidx == ~0ull) gidx = static_cast<unsigned long long>(idx);
          s_cand[k++] = static_cast<int16_t>(c);
        }
        if (gidx != ~0ull) {  // the first goal in candidate order: everything numbered before it was visited
          status = PW_PLAN_SOLVED;
          visited = gidx;
          k = 0;
        } else {
          visited = stored;
        }
        s_info[0] = static_cast<unsigned long long>(first);
        s_info[1] = static_cast<unsigned long long>(k);
      }
      __threadfence_block();
      __syncthreads();
      new_first = static_cast<int64_t>(s_info[0]);
      nnew = static_cast<int64_t>(s_info[1]);
    }
    // ---- results ----------------------------------------------------------------------------------------------------
    if (lane == 0) {
      info[0] = static_cast<int64_t>(status);
      info[1] = static_cast<int64_t>(rounds);
      info[2] = static_cast<int64_t>(expanded);
      info[3] = static_cast<int64_t>(visited);
      info[4] = static_cast<int64_t>(open);
      info[5] = gidx == ~0ull ? -1 : static_cast<int64_t>(gidx);
      info[6] = static_cast<int64_t>(exceeded);
      info[7] = static_cast<int64_t>(stored);
      info[8] = static_cast<int64_t>((wall_clock64() - t0) * 1000000ull / a.clock_khz);  // nanoseconds
      if (a.plan_len || a.first_action) {
        int32_t len = -1;
        int first = -1;
        if (gidx != ~0ull) {
          len = 0;
          for (int64_t at = static_cast<int64_t>(gidx); at > 0 && len <= a.max_states; at = parent[at]) len++;
          uint8_t* out = a.plans ? a.plans + static_cast<int64_t>(item) * a.plan_cap : nullptr;
          int64_t at = static_cast<int64_t>(gidx);
          for (int k = len - 1; k >= 0 && (out || a.first_action); k--) {
            if (out && k < a.plan_cap) out[k] = action[at];
            if (k == 0) first = action[at];
            at = parent[at];
          }
        }
        if (a.plan_len) a.plan_len[item] = len;
        if (a.first_action) a.first_action[item] = static_cast<int8_t>(first);
      }
    }
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------
struct PwPlanBatch {
  PwEngine* eng;
  int32_t n, mode, K, flags;
  int64_t max_states;
  uint32_t cost_range;
  std::vector<PwRgd*> rgd;
  PbItem* d_items;
  int32_t* d_slot_of;  // [set count] the first item of each set index, -1 = none (the states form)
  int32_t max_n;       // the largest prepared puzzle's movables
  uint8_t* d_groups;
  PwSlabPool pool;
  PbArgs args;         // everything but the per-run fields
  size_t lds;
  PwCancelWord cancel;
  uint64_t tags_used;
};

extern "C" {

void pw_plan_batch_destroy(PwPlanBatch* b) {
  if (!b) return;
  PwDeviceGuard guard(b->eng->set->device);
  if (b->d_items) (void)hipFree(b->d_items);
  if (b->d_slot_of) (void)hipFree(b->d_slot_of);
  if (b->d_groups) (void)hipFree(b->d_groups);
  if (b->pool.d_slab) (void)hipFree(b->pool.d_slab);
  cancel_word_destroy(&b->cancel);
  for (PwRgd* r : b->rgd) pw_rgd_destroy(r);
  delete b;
}

int pw_plan_batch_create(PwEngine* e, const int32_t* puzzles, int32_t n, int32_t mode, int64_t max_states, int32_t batch,
                         int32_t flags, int64_t rgd_budget, int32_t cost_range, PwPlanBatch** out) try {
  if (mode != PW_PLAN_RGD && mode != PW_PLAN_N_RGD) return pw_fail(PW_EINVAL, "mode must be PW_PLAN_RGD (0) or PW_PLAN_N_RGD (1)");
  if (batch < 1 || batch > kPbMaxK) return pw_fail(PW_EINVAL, "batch (K) must be in 1 .. 64");
  if (flags != PW_PLAN_ACTIONS_REFERENCE && flags != PW_PLAN_ACTIONS_FIXED)
    return pw_fail(PW_EINVAL, "flags must be PW_PLAN_ACTIONS_REFERENCE (0) or PW_PLAN_ACTIONS_FIXED (1)");
  if (rgd_budget < 0) return pw_fail(PW_EINVAL, "rgd_budget must be >= 0 (0 = the default)");
  if (cost_range < 0 || cost_range > static_cast<int32_t>(kPbCostRange))
    return pw_fail(PW_EINVAL, "cost_range must be in 1 .. 65536 (0 = 65536)");
  if (max_states < 4ll * batch + 1) return pw_fail(PW_EINVAL, "max_states must be at least 4 * batch + 1");
  if (max_states > (1ll << 28)) return pw_fail(PW_EINVAL, "max_states must be at most 2^28");
  if (n < 1) return pw_fail(PW_EINVAL, "n must be >= 1");
  if (!e || !out) return pw_fail(PW_EINVAL, "null argument");
  *out = nullptr;
  if (!pw_puzzles_ok(e, puzzles, n)) return pw_fail(PW_EINVAL, "puzzle index out of range");
  PwPlanBatch* b = new (std::nothrow) PwPlanBatch();
  if (!b) return pw_fail(PW_ENOMEM, "out of memory");
  b->eng = e;
  b->n = n;
  b->mode = mode;
  b->K = batch;
  b->flags = flags;
  b->max_states = max_states;
  b->cost_range = cost_range > 0 ? static_cast<uint32_t>(cost_range) : kPbCostRange;
  std::vector<PbItem> items(static_cast<size_t>(n));
  int max_n = 1, levels = 1;
  int64_t nov_words = 0;
  for (int32_t i = 0; i < n; i++) {  // (one PwRgd per item: a puzzle listed twice is cheap to list twice)
    const int32_t pid = puzzles ? puzzles[i] : i;
    PwRgd* r = nullptr;
    if (int rc = pw_rgd_create(e, pid, 1, rgd_budget, &r)) {
      pw_plan_batch_destroy(b);
      return rc;
    }
    b->rgd.push_back(r);
    PbItem& it = items[static_cast<size_t>(i)];
    std::memset(static_cast<void*>(&it), 0, sizeof(it));
    it.rgd = rgd_eval_args(r, nullptr, nullptr, 0);
    it.pid = pid;
    const PwPuzzleHeader& h = e->set->headers[pid];
    const int64_t D = static_cast<int64_t>(h.W) * h.H;
    const int64_t bits = mode == PW_PLAN_N_RGD ? h.N * D + static_cast<int64_t>(h.N) * (h.N - 1) / 2 * D * D : 0;
    if ((bits + 31) / 32 > (1ll << 30)) {
      pw_plan_batch_destroy(b);
      return pw_fail(PW_ELIMIT, "pw_plan_batch_create: a puzzle's novelty bits exceed 4 GiB");
    }
    it.nov_words = static_cast<int32_t>((bits + 31) / 32);
    nov_words = std::max<int64_t>(nov_words, it.nov_words);
    max_n = std::max<int>(max_n, h.N);
    levels = std::max(levels, std::max(h.N - 2, 1));
  }
  b->max_n = max_n;
  const std::vector<int32_t> slot_of = pw_slot_of(items, e->set->count);
  PbArgs& a = b->args;
  std::memset(static_cast<void*>(&a), 0, sizeof(a));
  a.hdrs = e->set->d_headers;
  a.blob = e->set->d_blob;
  a.n = n;
  a.mode = mode;
  a.K = batch;
  a.max_states = max_states;
  a.cost_range = b->cost_range;
  a.nb = (mode == PW_PLAN_RGD ? b->cost_range : 3u * b->cost_range) + 2u;
  a.n0 = (a.nb + 63u) / 64u;
  a.n1 = (a.n0 + 63u) / 64u;
  const uint64_t ms = static_cast<uint64_t>(max_states), slots = pw_table_slots(ms);
  a.slot_mask = static_cast<uint32_t>(slots - 1u);
  a.nw = (max_n + 1) / 2;
  a.levels = levels;
  uint64_t off = pw_pad256(ms * a.nw * 4);
  a.off_parent = off;
  off += pw_pad256(ms * 4);
  a.off_action = off;
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
  a.off_cand = off;
  off += pw_pad256(4ull * kPbMaxK * a.nw * 4);
  a.off_nov = off;
  off += pw_pad256(static_cast<uint64_t>(nov_words) * 4);
  a.slab_bytes = off;
  b->lds = static_cast<size_t>(PW_WAVE) * (16 * levels + 2 * 32);
  PwDeviceGuard guard(e->set->device);
  PwHipChain c(guard.status());
  slab_pool_create(&b->pool, c, n, e->num_cus, a.slab_bytes);
  c.alloc(&b->d_items, sizeof(PbItem) * items.size());
  c.alloc(&b->d_slot_of, sizeof(int32_t) * slot_of.size());
  c.alloc(&b->d_groups, kPlanGroups);
  cancel_word_create(&b->cancel, c);
  c.then([&] { return hipMemcpy(b->d_items, items.data(), sizeof(PbItem) * items.size(), hipMemcpyHostToDevice); });
  c.then([&] { return hipMemcpy(b->d_slot_of, slot_of.data(), sizeof(int32_t) * slot_of.size(), hipMemcpyHostToDevice); });
  c.then([&] { return plan_upload_groups(b->d_groups); });
  c.then([] { return hipDeviceSynchronize(); });
  if (!c.ok()) {
    pw_plan_batch_destroy(b);
    return pw_hip_fail("pw_plan_batch_create", c.err);
  }
  a.items = b->d_items;
  a.slot_of = b->d_slot_of;
  a.set_count = e->set->count;
  a.groups = flags == PW_PLAN_ACTIONS_FIXED ? nullptr : b->d_groups;
  a.slab = b->pool.slabs();
  a.next_item = b->pool.counter();
  a.cancel = b->cancel.d;
  a.clock_khz = pw_wall_clock_khz(e->set->device);
  b->tags_used = 0;
  *out = b;
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

}  // extern "C"

// the per-run fields of both forms and the launch: n items (tags tag_base .. tag_base + n - 1), at most one workgroup each
static int pb_launch(PwPlanBatch* b, PbArgs& a, int32_t n, int64_t max_rounds, double time_limit, int64_t* info,
                     uint8_t* plans, int32_t* plan_len, int32_t plan_cap, hipStream_t st, const char* what) {
  if (b->tags_used + static_cast<uint64_t>(n) >= 0xFFFFFFFFull) {  // tags would wrap: empty the slabs once more
    if (hipMemsetAsync(a.slab, 0, static_cast<size_t>(b->pool.groups) * static_cast<size_t>(a.slab_bytes), st) != hipSuccess)
      return pw_fail(PW_EDEVICE, std::string(what) + ": hipMemsetAsync failed");
    b->tags_used = 0;
  }
  a.n = n;
  a.tag_base = static_cast<uint32_t>(b->tags_used + 1u);
  b->tags_used += static_cast<uint64_t>(n);
  a.max_rounds = max_rounds;
  a.time_ticks = pw_deadline_ticks(time_limit, a.clock_khz);
  a.seq = ++b->cancel.seq;
  a.info = info;
  a.plans = plans;
  a.plan_len = plan_len;
  a.plan_cap = plans ? plan_cap : 0;
  if (hipMemsetAsync(a.next_item, 0, 4, st) != hipSuccess) return pw_fail(PW_EDEVICE, std::string(what) + ": hipMemsetAsync failed");
  const int64_t groups = std::min<int64_t>(b->pool.groups, n);
  hipLaunchKernelGGL(pw_plan_batch_kernel, dim3(static_cast<unsigned>(groups)), dim3(PW_WAVE), b->lds, st, a);
  return check_launch(what);
}

extern "C" {

int pw_plan_batch_run(PwPlanBatch* b, int64_t max_rounds, double time_limit, int64_t* info, uint8_t* plans, int32_t* plan_len,
                      int32_t plan_cap, void* stream) try {
  if (!b || !info) return pw_fail(PW_EINVAL, "null argument");
  if (!(time_limit >= 0.0)) return pw_fail(PW_EINVAL, "time_limit must be >= 0 seconds (0 = none)");
  if (plans && (!plan_len || plan_cap < 1)) return pw_fail(PW_EINVAL, "plans need plan_len and plan_cap >= 1");
  PwDeviceGuard guard(b->eng->set->device);
  PbArgs a = b->args;
  return pb_launch(b, a, b->n, max_rounds, time_limit, info, plans, plan_len, plan_cap, static_cast<hipStream_t>(stream),
                   "pw_plan_batch_run");
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_plan_batch_run_states(PwPlanBatch* b, const int32_t* puzzle_id, const int8_t* pos, int32_t npad, const uint8_t* mask,
                             int32_t n, int64_t max_rounds, double time_limit, int64_t* info, uint8_t* plans,
                             int32_t* plan_len, int32_t plan_cap, int8_t* first_action, void* stream) try {
  // (every check but the last needs no handle)
  if (n < 1) return pw_fail(PW_EINVAL, "n must be >= 1");
  if (int rc = pw_check_npad("", npad)) return rc;
  if (!puzzle_id || !pos || !info) return pw_fail(PW_EINVAL, "null argument (puzzle_id, pos and info are required)");
  if (!(time_limit >= 0.0)) return pw_fail(PW_EINVAL, "time_limit must be >= 0 seconds (0 = none)");
  if (plans && (!plan_len || plan_cap < 1)) return pw_fail(PW_EINVAL, "plans need plan_len and plan_cap >= 1");
  if (!b) return pw_fail(PW_EINVAL, "null handle");
  if (npad < b->max_n) return pw_fail(PW_EINVAL, "npad is smaller than the largest prepared puzzle's number of movables");
  PwDeviceGuard guard(b->eng->set->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  bool replaced = false;
  if (int rc = slab_pool_grow(&b->pool, n, b->eng->num_cus, "pw_plan_batch_run_states", &replaced)) return rc;
  if (replaced) {
    b->args.slab = b->pool.slabs();
    b->args.next_item = b->pool.counter();
    b->tags_used = 0;
  }
  PbArgs a = b->args;
  a.state_pid = puzzle_id;
  a.state_pos = pos;
  a.mask = mask;
  a.npad = npad;
  a.first_action = first_action;
  return pb_launch(b, a, n, max_rounds, time_limit, info, plans, plan_len, plan_cap, st, "pw_plan_batch_run_states");
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_plan_batch_cancel(PwPlanBatch* b) try {
  if (!b) return pw_fail(PW_EINVAL, "null argument");
  cancel_word_cancel(&b->cancel);
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

}  // extern "C"

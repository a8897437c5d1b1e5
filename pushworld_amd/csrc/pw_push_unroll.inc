// pw_push_unroll.inc -- K21: pushes unrolled into primitive actions (pw_push_unroll_count / _write), and the gather of the
// unrolled rows into plan arrays (pw_push_unroll_plans).
// Part of the single translation unit pw_kernels.hip (included there after pw_push_step.inc: uses pw_walk.inc's launch shape,
// pw_push_step.inc's board layout, the replay workspace's item counters and rocPRIM's scan).
//
// Definitions (include/pushworld_amd.h): a choice (from, a) of a state s is valid by pw_step_push's rule -- a in 0..3, from in
// the walk region R(s), (from, a) a push move.  Its unrolled sequence is L = path(R, from) + [a]: the parent actions of
// pw_walk_regions' map from the agent's position to `from`, then the push; len(L) = dist(from) + 1, the L of pw_step_push.
//
// The kernel is pw_push_step_kernel's frame as it is: one wavefront per workgroup, 64 / GS lane groups, one movable per lane,
// items off a device counter, five row bitboards per item in LDS (visited, current, next, parent bit 0, parent bit 1), every
// (q, a) verdict one group_push_set -- no second copy of the dynamics.  The flood goes layer by layer until `from` is
// discovered, then (from, a) is evaluated ONCE.
//   count  length[i] = dist + 1 (or -1) and the same number (or 0) into offset[i]; a rocPRIM exclusive scan over n + 1 values
//          turns the lengths into byte offsets.
//   write  the same flood again (the writing call recomputes), then the walk back from `from` along the two parent bits:
//          the k-th cell of the way back holds action L[dist - 1 - k], stored at offset[i] + dist - 1 - k; `a` goes to
//          offset[i] + dist.  One lane of the group stores, one byte per plain vector store.
//
// Equivalence with pw_walk_regions' map.  The parent bits of a cell are the action of its first discovery: layers in order,
// inside a layer action by action (the iterator runs ai = 0..3 over the whole current layer before ai + 1), so the first
// discovery of a cell of layer d + 1 is by the lowest action a for which some cell q' of layer d has the walk move (q', a)
// onto it -- pw_walk_regions' parent(q), written by the same discover() at the same moment.  A flood that stops at the
// discovery of `from` has completed every layer before dist(from), and the ancestors of `from` all lie in those layers; the
// parent of `from` itself is fixed by its first discovery, which is the one that stops the flood.  The order of the cells
// inside an action does not matter: for one action two different cells never discover the same cell.
//
// Every loop is bounded by the items, the W x H cells of a board times four actions, the rows of a board, or the layers of a
// region (at most 4 095: the walk back); there is no wait on another workgroup and no device assert.
//
// The gather is one launch of lane groups of 16, one group per plan: the rows of a plan are consecutive, so their spans are
// one contiguous run of `actions` and the plan's length is offset[last + 1] - offset[first].

struct PushUnrollArgs {
  const PwPuzzleHeader* hdrs;
  const uint8_t* blob;
  const uint64_t* ovl;
  const PwOvlDir* ovl_dir;
  const int32_t* puzzle_id;    // [n]
  const int8_t* pos;           // [n][npad][2] or NULL (initial states)
  const int8_t* push_from;     // [n][2]
  const uint8_t* push_action;  // [n]
  const uint8_t* mask;         // [n] or NULL
  int32_t n, npad, num_puzzles, rows, write;  // rows: LDS rows per board (the set's largest height)
  uint32_t* next_item;
  int32_t* length;  // count: [n]
  int64_t* offset;  // count: written; write: read
  int64_t cap;      // write: bytes of `actions`
  uint8_t* actions;
  unsigned long long* dropped;  // or NULL
};

template <int GS, int kTab>
__global__ __launch_bounds__(64) void pw_push_unroll_kernel(PushUnrollArgs a) {
  extern __shared__ uint64_t pw_punroll_lds[];
  const int lane = threadIdx.x;
  const int lj = lane & (GS - 1);
  const int gbase = lane & ~(GS - 1);
  const unsigned long long gmask = ((1ull << (GS - 1) << 1) - 1ull) << gbase;
  if (!a.write && blockIdx.x == 0 && lane == 0) a.offset[a.n] = 0;  // the scan's last input: offset[n] becomes the total
  uint64_t* const B = pw_punroll_lds + static_cast<size_t>(lane / GS) * PW_PSTEP_BOARDS * a.rows;
  uint64_t* const VIS = B;
  uint64_t* const CUR = B + a.rows;
  uint64_t* const NXT = B + 2 * a.rows;
  uint64_t* const PAR0 = B + 3 * a.rows;
  uint64_t* const PAR1 = B + 4 * a.rows;

  LanePuzzleT<const uint64_t*, kTab> p;
  const PwPuzzleHeader* h = a.hdrs;
  p.h = h;
  p.wall = p.awall = p.shapes = reinterpret_cast<const uint64_t*>(a.blob + h->base);
  p.pair = nullptr;
  p.wtab = nullptr;
  p.R = p.Hs = 0;
  p.H = p.N = p.G = 0;
  bool active = false, exhausted = false;
  int item = 0, xy = 0;
  int W = 0, aw = 0, ah = 0, q0x = 0, q0y = 0;
  int fx = 0, fy = 0, fa = 0;
  // the group's iterator: phase (0 the flood, 1 the push itself), layer, action, row, what is left of the row / of the layer
  int phase = 0, d = 0, ai = 0, cy = 0, dist = 0;
  uint64_t rowbits = 0, ymask = 0, cur_rows = 0, next_rows = 0;
  uint32_t ot = 0;
  uint64_t small = 0;
  int64_t base = 0;
  unsigned long long n_dropped = 0;
  const LaneSlot none = lane_slot(0, 0u, 0ull);

  // a refused item: length -1 and no bytes (the writing call writes nothing for it)
  auto refuse = [&]() {
    if (!a.write && lj == 0) {
      a.length[item] = -1;
      a.offset[item] = 0;
    }
    active = false;
  };
  // the agent walks from (x, y) by action `act` onto a cell of the next layer
  auto discover = [&](int x, int y, int act) {
    const int nx = x + (act == 0 ? -1 : (act == 1 ? 1 : 0)), ny = y + (act == 2 ? -1 : (act == 3 ? 1 : 0));
    if (nx < 0 || ny < 0 || nx + aw > W || ny + ah > p.H) return;
    const uint64_t bit = 1ull << nx;
    if (VIS[ny] & bit) return;
    VIS[ny] |= bit;
    NXT[ny] |= bit;
    next_rows |= 1ull << ny;
    if (act & 1) PAR0[ny] |= bit;
    if (act & 2) PAR1[ny] |= bit;
    if (nx == fx && ny == fy) {  // the flood need not go on: the ancestors of `from` lie in the layers before it
      dist = d + 1;
      phase = 1;
    }
  };

  for (;;) {
    const bool need = !active && !exhausted;
    if (__ballot(need) != 0ull) {
      if (need) {  // (group-uniform: the GS lanes of a group are all here or all not)
        int idx = 0;
        if (lj == 0) idx = static_cast<int>(atomicAdd(a.next_item, 1u));
        idx = __shfl(idx, gbase, PW_WAVE);
        if (static_cast<unsigned>(idx) >= static_cast<unsigned>(a.n)) {
          exhausted = true;
        } else {
          item = idx;
          xy = 0;
          const int spid = a.puzzle_id[idx];
          bool skip = (a.mask && a.mask[idx] == 0) || spid < 0 || spid >= a.num_puzzles;
          if (a.write && !skip) {
            base = a.offset[idx];
            skip = a.offset[idx + 1] == base;  // (refused by the first call)
          }
          int N = 0;
          if (!skip) {
            h = a.hdrs + spid;
            N = h->N;
            if (lj < N) {  // every movable inside its grid (pw_validate_state's range test); nothing past N is read
              int v;
              if (a.pos) v = reinterpret_cast<const uint16_t*>(a.pos)[static_cast<int64_t>(idx) * a.npad + lj];
              else v = reinterpret_cast<const uint16_t*>(h->init)[lj];
              xy = v;
              ot = reinterpret_cast<const uint32_t*>(h->objtab)[lj];
            }
            const int x = static_cast<int8_t>(xy & 0xff), y = static_cast<int8_t>((xy >> 8) & 0xff);
            const bool bad = lj < N && (x < 0 || y < 0 || x + static_cast<int>(ot & 0xffu) > h->W ||
                                        y + static_cast<int>((ot >> 8) & 0xffu) > h->H);
            skip = (__ballot(bad) & gmask) != 0ull;
          }
          if (!skip) {
            if (lj >= N) ot = 0u;
            const int axy = __shfl(xy, gbase, PW_WAVE);
            const uint32_t aot = static_cast<uint32_t>(__shfl(static_cast<int>(ot), gbase, PW_WAVE));
            q0x = axy & 0xff;
            q0y = (axy >> 8) & 0xff;
            aw = static_cast<int>(aot & 0xffu);
            ah = static_cast<int>((aot >> 8) & 0xffu);
            W = h->W;
            p.H = min(static_cast<int>(h->H), a.rows);  // (a.rows is the set's largest height: never the smaller one)
            fx = a.push_from[2 * static_cast<int64_t>(idx)];
            fy = a.push_from[2 * static_cast<int64_t>(idx) + 1];
            fa = a.push_action[idx];
            // an action outside 0..3 or a position at which the agent leaves its grid: no push move
            skip = fa > 3 || fx < 0 || fy < 0 || fx + aw > W || fy + ah > p.H;
          }
          if (skip) {
            refuse();
          } else {
            const uint8_t* b = a.blob + h->base;
            p.h = h;
            p.wall = reinterpret_cast<const uint64_t*>(b + h->off_wall);
            p.awall = reinterpret_cast<const uint64_t*>(b + h->off_awall);
            p.shapes = reinterpret_cast<const uint64_t*>(b + h->off_shapes);
            lane_tables(p, a.ovl, a.ovl_dir, spid);
            p.N = N;
            p.G = h->G;
            small = (lj < N) ? reinterpret_cast<const uint64_t*>(b + h->off_small)[lj] : 0ull;
            for (int y = 0; y < p.H; y++) VIS[y] = CUR[y] = NXT[y] = PAR0[y] = PAR1[y] = 0ull;
            VIS[q0y] = CUR[q0y] = 1ull << q0x;
            cur_rows = 1ull << q0y;
            next_rows = 0ull;
            ymask = cur_rows;
            rowbits = 0ull;
            d = 0;
            ai = 0;
            dist = 0;
            phase = (fx == q0x && fy == q0y) ? 1 : 0;
            active = true;
          }
        }
      }
    }
    if (__ballot(active) == 0ull) {
      if (__ballot(!exhausted) == 0ull) break;
      continue;
    }

    // ---- the next candidate (cx, cy, ai) of every active lane group: plain per-lane code, no cross-lane operation -------------
    bool have = false;
    int cx = 0;
    if (active) {
      while (phase == 0) {
        if (rowbits != 0ull) {
          cx = __ffsll(static_cast<unsigned long long>(rowbits)) - 1;
          rowbits &= rowbits - 1ull;
          have = true;
          break;
        }
        if (ymask != 0ull) {
          cy = __ffsll(static_cast<unsigned long long>(ymask)) - 1;
          ymask &= ymask - 1ull;
          rowbits = CUR[cy];
          continue;
        }
        if (ai < 3) {
          ai++;
          ymask = cur_rows;
          continue;
        }
        if (next_rows == 0ull) break;  // the region is exhausted and `from` is not in it
        for (uint64_t m = cur_rows | next_rows; m != 0ull; m &= m - 1ull) {
          const int y = __ffsll(static_cast<unsigned long long>(m)) - 1;
          CUR[y] = NXT[y];
          NXT[y] = 0ull;
        }
        cur_rows = next_rows;
        next_rows = 0ull;
        ymask = cur_rows;
        d++;
        ai = 0;
      }
      if (phase == 1) {
        have = true;
        cx = fx;
        cy = fy;
      } else if (!have) {
        refuse();
      }
    }
    if (!active) {  // (a group between items plays nothing: no movable)
      p.N = 0;
      xy = 0;
      ot = 0u;
      small = 0ull;
    }

    // ---- one step of every lane group that has a candidate: the agent's slot stands at the candidate ------------------------
    const bool play = active && have;
    const int act = (phase == 1 ? fa : ai) & 3;  // (a group that plays nothing may hold a refused action: never an index)
    const int dx = act == 0 ? -1 : (act == 1 ? 1 : 0);
    const int dy = act == 2 ? -1 : (act == 3 ? 1 : 0);
    const int sxy = (play && lj == 0) ? ((cx & 0xff) | ((cy & 0xff) << 8)) : xy;
    const LaneSlot s0 = lane_slot(sxy, ot, small);
    const uint32_t moved = group_push_set<GS, false>(p, s0, none, lj, gbase, gmask, play, act, dx, dy);
    if (play && phase == 0) {
      if (moved == 1u) discover(cx, cy, ai);
    } else if (play) {
      if (moved == 0u || moved == 1u) {  // a step that displaces nothing, or a walk move
        refuse();
      } else {
        if (!a.write) {
          if (lj == 0) {
            a.length[item] = dist + 1;
            a.offset[item] = dist + 1;
          }
        } else if (lj == 0) {  // (a lane reads the words it wrote itself: every lane of the group wrote all of them)
          int x = fx, y = fy;
          for (int k = dist; k > 0; k--) {  // the cell of layer k holds L[k - 1]
            const int pa = static_cast<int>((PAR0[y] >> x) & 1ull) | (static_cast<int>((PAR1[y] >> x) & 1ull) << 1);
            const int64_t at = base + k - 1;
            if (at >= 0 && at < a.cap) a.actions[at] = static_cast<uint8_t>(pa);
            else n_dropped++;
            x -= pa == 0 ? -1 : (pa == 1 ? 1 : 0);
            y -= pa == 2 ? -1 : (pa == 3 ? 1 : 0);
          }
          const int64_t at = base + dist;
          if (at >= 0 && at < a.cap) a.actions[at] = static_cast<uint8_t>(fa);
          else n_dropped++;
        }
        active = false;
      }
    }
  }
  if (a.write && a.dropped && n_dropped) atomicAdd(a.dropped, n_dropped);
}

struct PushUnrollPlansArgs {
  const int64_t* item_offset;  // [m + 1]
  const int32_t* length;       // [rows]
  const int64_t* offset;       // [rows + 1]
  const uint8_t* actions;      // [cap]
  int64_t rows, cap, m;
  int32_t plan_cap;
  uint8_t* plans;     // [m][plan_cap]
  int32_t* plan_len;  // [m]
};

#define PW_PUNROLL_GROUP 16  // lanes per plan of the gather

__global__ __launch_bounds__(256) void pw_push_unroll_plans_kernel(PushUnrollPlansArgs a) {
  const int lj = threadIdx.x & (PW_PUNROLL_GROUP - 1);
  const int gbase = (threadIdx.x & (PW_WAVE - 1)) & ~(PW_PUNROLL_GROUP - 1);
  const unsigned long long gmask = ((1ull << PW_PUNROLL_GROUP) - 1ull) << gbase;
  const int64_t j = static_cast<int64_t>(blockIdx.x) * (256 / PW_PUNROLL_GROUP) + threadIdx.x / PW_PUNROLL_GROUP;
  if (j >= a.m) return;  // (group-uniform)
  const int64_t r0 = a.item_offset[j], r1 = a.item_offset[j + 1];
  bool bad = r0 < 0 || r1 < r0 || r1 > a.rows;
  if (!bad)
    for (int64_t r = r0 + lj; r < r1; r += PW_PUNROLL_GROUP) bad |= a.length[r] < 0;  // a refused row
  bad = (__ballot(bad) & gmask) != 0ull;
  int64_t len = -1, b0 = 0;
  if (!bad) {
    b0 = a.offset[r0];
    const int64_t b1 = a.offset[r1];
    len = b1 - b0;
    // (bytes the writing call dropped are not there to be copied: no plan; a plan without rows reads none)
    if (b0 < 0 || len < 0 || (len > 0 && b1 > a.cap) || len > 0x7fffffffll) len = -1;
  }
  if (lj == 0) a.plan_len[j] = static_cast<int32_t>(len);
  const int64_t copy = len < a.plan_cap ? len : static_cast<int64_t>(a.plan_cap);
  uint8_t* out = a.plans + j * a.plan_cap;
  for (int64_t k = lj; k < copy; k += PW_PUNROLL_GROUP) out[k] = a.actions[b0 + k];
}

// the argument checks of count and write; everything but the last two needs no engine
static int push_unroll_check_args(const PwEngine* e, const int32_t* puzzle_id, int32_t npad, const int8_t* push_from,
                                  const uint8_t* push_action, int32_t n, const int64_t* offset, int64_t cap, const char* what) {
  const std::string w = std::string(what) + ": ";
  if (n < 1) return pw_fail(PW_EINVAL, w + "n must be >= 1");
  if (int rc = pw_check_npad(w, npad)) return rc;
  if (!puzzle_id) return pw_fail(PW_EINVAL, w + "null puzzle_id");
  if (!push_from) return pw_fail(PW_EINVAL, w + "null push_from");
  if (!push_action) return pw_fail(PW_EINVAL, w + "null push_action");
  if (!offset) return pw_fail(PW_EINVAL, w + "null offset");
  if (cap < 0) return pw_fail(PW_EINVAL, w + "cap must be >= 0");
  if (!e) return pw_fail(PW_EINVAL, w + "null engine");
  if (npad < e->set->max_n) return pw_fail(PW_EINVAL, w + "npad is smaller than the set's largest number of movables");
  return PW_OK;
}

static void push_unroll_launch(PwEngine* e, PushUnrollArgs& a, hipStream_t st) {
  a.hdrs = e->set->d_headers;
  a.blob = e->set->d_blob;
  a.ovl = e->d_ovl;
  a.ovl_dir = e->d_ovl_dir;
  a.num_puzzles = e->set->count;
  a.rows = std::min(std::max(e->set->max_h, 1), PW_MAX_DIM);
  a.next_item = reinterpret_cast<uint32_t*>(e->d_replay + 64 * (e->replay_seq++ & 63u));
  (void)hipMemsetAsync(a.next_item, 0, 4, st);
  const int tab = e->ovl_puzzles == 0 ? 0 : (e->ovl_puzzles == e->set->count ? 2 : 1);
  const int gs = a.npad <= 8 ? 8 : a.npad;
  // the boards of the wavefront's 64 / GS items: at most 5 * 64 * 8 * 8 = 20 KB
  const size_t lds = static_cast<size_t>(PW_WAVE / gs) * PW_PSTEP_BOARDS * a.rows * sizeof(uint64_t);
  const int64_t waves = (static_cast<int64_t>(a.n) + (PW_WAVE / gs) - 1) / (PW_WAVE / gs);
  const dim3 grid(static_cast<unsigned>(std::min<int64_t>(waves, 16ll * std::max(e->num_cus, 1)))), block(PW_WAVE);
#define PW_LAUNCH_PUNROLL(GS)                                                                        \
  do {                                                                                               \
    if (tab == 0) hipLaunchKernelGGL((pw_push_unroll_kernel<GS, 0>), grid, block, lds, st, a);       \
    else if (tab == 1) hipLaunchKernelGGL((pw_push_unroll_kernel<GS, 1>), grid, block, lds, st, a);  \
    else hipLaunchKernelGGL((pw_push_unroll_kernel<GS, 2>), grid, block, lds, st, a);                \
  } while (0)
  if (gs == 8) PW_LAUNCH_PUNROLL(8);
  else if (gs == 16) PW_LAUNCH_PUNROLL(16);
  else PW_LAUNCH_PUNROLL(32);
#undef PW_LAUNCH_PUNROLL
}

extern "C" {

int pw_push_unroll_count(PwEngine* e, const int32_t* puzzle_id, const int8_t* pos, int32_t npad, const int8_t* push_from,
                         const uint8_t* push_action, const uint8_t* mask, int32_t n, int32_t* length, int64_t* offset,
                         void* stream) try {
  if (!length) return pw_fail(PW_EINVAL, "pw_push_unroll_count: null length");
  if (int rc = push_unroll_check_args(e, puzzle_id, npad, push_from, push_action, n, offset, 0, "pw_push_unroll_count")) return rc;
  PwDeviceGuard guard(e->set->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  size_t scan_bytes = 0;
  const size_t count = static_cast<size_t>(n) + 1;
  hipError_t err = rocprim::exclusive_scan(nullptr, scan_bytes, offset, offset, static_cast<int64_t>(0), count,
                                           rocprim::plus<int64_t>(), st);
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string("pw_push_unroll_count: ") + hipGetErrorString(err));
  scan_bytes = pw_pad256(scan_bytes);
  if (int rc = replay_workspace(e, scan_bytes, "pw_push_unroll_count")) return rc;
  PushUnrollArgs a{};
  a.puzzle_id = puzzle_id;
  a.pos = pos;
  a.push_from = push_from;
  a.push_action = push_action;
  a.mask = mask;
  a.n = n;
  a.npad = npad;
  a.write = 0;
  a.length = length;
  a.offset = offset;
  push_unroll_launch(e, a, st);
  if (int rc = check_launch("pw_push_unroll_count")) return rc;
  size_t tmp = e->replay_bytes - kReplayCounterBytes;
  err = rocprim::exclusive_scan(e->d_replay + kReplayCounterBytes, tmp, offset, offset, static_cast<int64_t>(0), count,
                                rocprim::plus<int64_t>(), st);
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string("pw_push_unroll_count: ") + hipGetErrorString(err));
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_push_unroll_write(PwEngine* e, const int32_t* puzzle_id, const int8_t* pos, int32_t npad, const int8_t* push_from,
                         const uint8_t* push_action, const uint8_t* mask, int32_t n, const int64_t* offset, int64_t cap,
                         uint8_t* actions, int64_t* dropped, void* stream) try {
  if (!actions && cap > 0) return pw_fail(PW_EINVAL, "pw_push_unroll_write: null actions");
  if (int rc = push_unroll_check_args(e, puzzle_id, npad, push_from, push_action, n, offset, cap, "pw_push_unroll_write")) return rc;
  PwDeviceGuard guard(e->set->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (int rc = replay_workspace(e, 0, "pw_push_unroll_write")) return rc;
  if (dropped && hipMemsetAsync(dropped, 0, 8, st) != hipSuccess)
    return pw_fail(PW_EDEVICE, "pw_push_unroll_write: hipMemsetAsync failed");
  PushUnrollArgs a{};
  a.puzzle_id = puzzle_id;
  a.pos = pos;
  a.push_from = push_from;
  a.push_action = push_action;
  a.mask = mask;
  a.n = n;
  a.npad = npad;
  a.write = 1;
  a.offset = const_cast<int64_t*>(offset);
  a.cap = actions ? cap : 0;
  a.actions = actions;
  a.dropped = reinterpret_cast<unsigned long long*>(dropped);
  push_unroll_launch(e, a, st);
  return check_launch("pw_push_unroll_write");
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_push_unroll_plans(PwEngine* e, const int64_t* item_offset, const int32_t* length, const int64_t* offset,
                         const uint8_t* actions, int64_t rows, int64_t cap, int32_t m, int32_t plan_cap, uint8_t* plans,
                         int32_t* plan_len, void* stream) try {
  if (m < 1) return pw_fail(PW_EINVAL, "pw_push_unroll_plans: m must be >= 1");
  if (rows < 0) return pw_fail(PW_EINVAL, "pw_push_unroll_plans: rows must be >= 0");
  if (cap < 0) return pw_fail(PW_EINVAL, "pw_push_unroll_plans: cap must be >= 0");
  if (plan_cap < 1 || plan_cap > PW_PLAN_MAX_ACTIONS)
    return pw_fail(PW_EINVAL, "pw_push_unroll_plans: plan_cap must be 1 .. PW_PLAN_MAX_ACTIONS");
  if (!item_offset) return pw_fail(PW_EINVAL, "pw_push_unroll_plans: null item_offset");
  if (!length && rows > 0) return pw_fail(PW_EINVAL, "pw_push_unroll_plans: null length");
  if (!offset) return pw_fail(PW_EINVAL, "pw_push_unroll_plans: null offset");
  if (!actions && cap > 0) return pw_fail(PW_EINVAL, "pw_push_unroll_plans: null actions");
  if (!plans) return pw_fail(PW_EINVAL, "pw_push_unroll_plans: null plans");
  if (!plan_len) return pw_fail(PW_EINVAL, "pw_push_unroll_plans: null plan_len");
  if (!e) return pw_fail(PW_EINVAL, "pw_push_unroll_plans: null engine");
  PwDeviceGuard guard(e->set->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  PushUnrollPlansArgs a{};
  a.item_offset = item_offset;
  a.length = length;
  a.offset = offset;
  a.actions = actions;
  a.rows = rows;
  a.cap = actions ? cap : 0;
  a.m = m;
  a.plan_cap = plan_cap;
  a.plans = plans;
  a.plan_len = plan_len;
  const int per_block = 256 / PW_PUNROLL_GROUP;
  const dim3 grid(static_cast<unsigned>((static_cast<int64_t>(m) + per_block - 1) / per_block)), block(256);
  hipLaunchKernelGGL(pw_push_unroll_plans_kernel, grid, block, 0, st, a);
  return check_launch("pw_push_unroll_plans");
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

}  // extern "C"

// pw_walk.inc -- K15: the agent's walk region and the push moves of a batch of states.
// Part of the single translation unit pw_kernels.hip (included there after pw_plan_replay.inc: uses its workspace, the
// lane-group step helpers of pw_step_kernels.inc and rocPRIM's scan).
//
// Definitions (include/pushworld_amd.h): a walk move (q, a) displaces the agent and nothing else; the walk region R is what
// the agent reaches by walk moves with the other movables fixed; a push move (q, a), q in R, displaces the agent and at
// least one other movable.  Positions at which the agent would leave its grid are not part of R (the range test of the
// inputs).
//
// The lane-group closure of K1d / K11 with the region as bitboards in LDS (not one of SURVEY section 7's forms: no table lookup
// per lane, no wavefront per state): one wavefront per workgroup holds 64 / GS lane groups (one movable per lane, as the plan
// replay); a lane group takes items off a device counter and runs a breadth-first search over agent positions, one layer
// after the other, action by action inside a layer (so the first discovery of a cell carries its lowest parent action).  Every
// (q, a) is ONE group_push_set -- the push-set logic of pw_step -- with the agent's slot moved to q: there is no second copy
// of the dynamics, and overlapping states get what the step function gives them.  The region lives in LDS as row bitboards
// (visited / current layer / next layer, a walk board and a push board per action): 12 boards of the set's largest height,
// 96 bytes per row and item.  Every lane of a group keeps the same iterator in registers and writes the same words, so a
// lane only ever reads what it wrote itself: no barrier, no cross-lane ordering.
//
//   regions  pass 1 only: region_size, canon, the walk map (dist | parent << 12, written at discovery) and the number of
//            push moves into offset[i]; a rocPRIM exclusive scan over n + 1 values turns the counts into row offsets.
//            With a push_mask (pw_push_mask, pw_push_step.inc) the push boards are written out as one byte per position when an
//            item's flood ends; region_size / offset may be NULL then and no scan follows.
//   pushes   pass 1 again (the emitting call recomputes), then pass 2 walks the layers a second time over the walk boards
//            -- bit operations only -- and calls group_push_set for the push candidates alone: a row's index is its rank in
//            (y, x, action) order, read off the push boards, its walk distance is the layer.
//
// Every loop is bounded by the items, the W x H cells of a board times four actions, or the rows of a board; there is no
// wait on another workgroup.

#define PW_WALK_BOARDS 12  // visited, current, next, walk[4], push[4], row prefix of the push counts

struct WalkArgs {
  const PwPuzzleHeader* hdrs;
  const uint8_t* blob;
  const uint64_t* ovl;
  const PwOvlDir* ovl_dir;
  const int32_t* puzzle_id;  // [n]
  const int8_t* pos;         // [n][npad][2] or NULL (initial states)
  const uint8_t* mask;       // [n] or NULL
  int32_t n, npad, num_puzzles, emit, rows;  // rows: LDS rows per board (the set's largest height)
  uint32_t* next_item;
  // regions
  int32_t* region_size;
  int8_t* canon;
  int64_t* offset;  // regions: written; pushes: read
  uint16_t* walk_map;
  int32_t map_h, map_w;
  // the push boards written out (pw_push_mask, pw_push_step.inc): region_size / offset may be NULL then
  uint8_t* push_mask;   // [n][map_h][map_w], zeroed by the caller: bit a of [y][x] = ((x, y), a) is a push move
  int32_t* num_pushes;  // [n] or NULL
  // pushes
  int64_t cap;
  int32_t* row_item;
  int8_t* row_from;
  uint8_t* row_action;
  int32_t* row_walk;
  uint32_t* row_moved;
  uint8_t* row_goal;
  int8_t* row_next_pos;
  unsigned long long* dropped;
};

template <int GS, int kTab>
__global__ __launch_bounds__(64) void pw_walk_kernel(WalkArgs a) {
  extern __shared__ uint64_t pw_walk_lds[];
  const int lane = threadIdx.x;
  const int lj = lane & (GS - 1);
  const int gbase = lane & ~(GS - 1);
  const unsigned long long gmask = ((1ull << (GS - 1) << 1) - 1ull) << gbase;
  if (!a.emit && a.offset && blockIdx.x == 0 && lane == 0) a.offset[a.n] = 0;  // the scan's last input: offset[n] becomes the total
  uint64_t* const B = pw_walk_lds + static_cast<size_t>(lane / GS) * PW_WALK_BOARDS * a.rows;
  uint64_t* const VIS = B;
  uint64_t* const CUR = B + a.rows;
  uint64_t* const NXT = B + 2 * a.rows;
  uint64_t* const WALK = B + 3 * a.rows;  // [4][rows]
  uint64_t* const PUSH = B + 7 * a.rows;  // [4][rows]
  uint64_t* const PRE = B + 11 * a.rows;

  LanePuzzleT<const uint64_t*, kTab> p;
  const PwPuzzleHeader* h = a.hdrs;
  p.h = h;
  p.wall = p.awall = p.shapes = reinterpret_cast<const uint64_t*>(a.blob + h->base);
  p.pair = nullptr;
  p.wtab = nullptr;
  p.R = p.Hs = 0;
  p.H = p.N = p.G = 0;
  bool active = false, exhausted = false, is_goal_lane = false;
  int item = 0, pid = 0, xy = 0, gxy = -1;
  int W = 0, aw = 0, ah = 0, q0x = 0, q0y = 0;
  // the group's iterator: pass, layer, action, row, what is left of the row / of the layer's rows
  int pass = 1, d = 0, ai = 0, cy = 0, rsize = 0, npush = 0, ckey = 0;
  uint64_t rowbits = 0, ymask = 0, cur_rows = 0, next_rows = 0;
  uint32_t ot = 0;
  uint64_t small = 0;
  int64_t base = 0;
  unsigned long long n_dropped = 0;
  const LaneSlot none = lane_slot(0, 0u, 0ull);

  // the agent walks from (x, y) by action `act` onto a cell of the next layer
  auto discover = [&](int x, int y, int act) {
    const int nx = x + (act == 0 ? -1 : (act == 1 ? 1 : 0)), ny = y + (act == 2 ? -1 : (act == 3 ? 1 : 0));
    if (nx < 0 || ny < 0 || nx + aw > W || ny + ah > p.H) return;
    const uint64_t bit = 1ull << nx;
    if (VIS[ny] & bit) return;
    VIS[ny] |= bit;
    NXT[ny] |= bit;
    next_rows |= 1ull << ny;
    if (pass == 1) {
      rsize++;
      ckey = min(ckey, ny * 64 + nx);
      if (a.walk_map && lj == 0)
        a.walk_map[(static_cast<int64_t>(item) * a.map_h + ny) * a.map_w + nx] = static_cast<uint16_t>((d + 1) | (act << 12));
    }
  };
  // layer 0 of a pass: the agent's own position
  auto seed = [&]() {
    for (int y = 0; y < p.H; y++) VIS[y] = CUR[y] = NXT[y] = 0ull;
    VIS[q0y] = CUR[q0y] = 1ull << q0x;
    cur_rows = 1ull << q0y;
    next_rows = 0ull;
    ymask = cur_rows;
    rowbits = 0ull;
    d = 0;
    ai = 0;
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
          if (a.emit && !skip) {
            base = a.offset[idx];
            skip = a.offset[idx + 1] == base;  // (no push moves, or skipped by the first call)
          }
          int N = 0;
          if (!skip) {
            pid = spid;
            h = a.hdrs + pid;
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
          if (skip) {
            if (!a.emit) {
              if (lj == 0) {
                if (a.region_size) a.region_size[item] = -1;
                if (a.offset) a.offset[item] = 0;
                if (a.num_pushes) a.num_pushes[item] = 0;
              }
              if (a.canon && lj == 0) reinterpret_cast<int16_t*>(a.canon)[item] = 0;
            }
          } else {
            const uint8_t* b = a.blob + h->base;
            p.h = h;
            p.wall = reinterpret_cast<const uint64_t*>(b + h->off_wall);
            p.awall = reinterpret_cast<const uint64_t*>(b + h->off_awall);
            p.shapes = reinterpret_cast<const uint64_t*>(b + h->off_shapes);
            lane_tables(p, a.ovl, a.ovl_dir, pid);
            p.H = min(static_cast<int>(h->H), a.rows);  // (a.rows is the set's largest height: never the smaller one)
            p.N = N;
            p.G = h->G;
            W = h->W;
            if (lj >= N) ot = 0u;
            small = (lj < N) ? reinterpret_cast<const uint64_t*>(b + h->off_small)[lj] : 0ull;
            is_goal_lane = lj >= 1 && lj <= p.G;
            gxy = is_goal_lane ? static_cast<int>(reinterpret_cast<const uint16_t*>(h->goal)[lj - 1]) : -1;
            const int axy = __shfl(xy, gbase, PW_WAVE);
            const uint32_t aot = static_cast<uint32_t>(__shfl(static_cast<int>(ot), gbase, PW_WAVE));
            q0x = axy & 0xff;
            q0y = (axy >> 8) & 0xff;
            aw = static_cast<int>(aot & 0xffu);
            ah = static_cast<int>((aot >> 8) & 0xffu);
            for (int y = 0; y < p.H; y++) {
#pragma unroll
              for (int k = 0; k < 4; k++) WALK[k * a.rows + y] = PUSH[k * a.rows + y] = 0ull;
            }
            pass = 1;
            rsize = 1;
            npush = 0;
            ckey = q0y * 64 + q0x;
            seed();
            if (!a.emit && a.walk_map && lj == 0) a.walk_map[(static_cast<int64_t>(item) * a.map_h + q0y) * a.map_w + q0x] = 0;
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
      for (;;) {
        if (rowbits != 0ull) {
          cx = __ffsll(static_cast<unsigned long long>(rowbits)) - 1;
          rowbits &= rowbits - 1ull;
          if (pass == 1) {
            have = true;
            break;
          }
          const uint64_t bit = 1ull << cx;  // pass 2: walk moves are replayed from the boards, push moves are recomputed
          if (WALK[ai * a.rows + cy] & bit) {
            discover(cx, cy, ai);
          } else if (PUSH[ai * a.rows + cy] & bit) {
            have = true;
            break;
          }
          continue;
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
        if (next_rows == 0ull) break;  // the pass is over
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
      if (!have) {
        if (!a.emit) {
          if (a.push_mask) {  // (a lane reads the words it wrote itself: every lane of the group wrote all of them)
            for (int y = lj; y < p.H; y += GS) {
              const uint64_t r0 = PUSH[y], r1 = PUSH[a.rows + y], r2 = PUSH[2 * a.rows + y], r3 = PUSH[3 * a.rows + y];
              uint8_t* out = a.push_mask + (static_cast<int64_t>(item) * a.map_h + y) * a.map_w;
              for (uint64_t m = r0 | r1 | r2 | r3; m != 0ull; m &= m - 1ull) {
                const int x = __ffsll(static_cast<unsigned long long>(m)) - 1;
                out[x] = static_cast<uint8_t>(((r0 >> x) & 1ull) | (((r1 >> x) & 1ull) << 1) | (((r2 >> x) & 1ull) << 2) |
                                              (((r3 >> x) & 1ull) << 3));
              }
            }
          }
          if (lj == 0) {
            if (a.region_size) a.region_size[item] = rsize;
            if (a.offset) a.offset[item] = npush;
            if (a.num_pushes) a.num_pushes[item] = npush;
            if (a.canon) reinterpret_cast<int16_t*>(a.canon)[item] = static_cast<int16_t>((ckey & 63) | ((ckey >> 6) << 8));
          }
          active = false;
        } else if (pass == 1 && npush != 0) {  // the rows before row y, then the layers once more
          uint64_t run = 0;
          for (int y = 0; y < p.H; y++) {
            PRE[y] = run;
#pragma unroll
            for (int k = 0; k < 4; k++) run += static_cast<uint64_t>(__popcll(PUSH[k * a.rows + y]));
          }
          pass = 2;
          seed();
        } else {
          active = false;
        }
      }
    }
    if (!active) {  // (a group between items plays nothing: no movable, no goal lane)
      p.N = 0;
      is_goal_lane = false;
      xy = 0;
      ot = 0u;
      small = 0ull;
    }

    // ---- one step of every lane group that has a candidate: the agent's slot stands at the candidate ------------------------
    const bool play = active && have;
    const int dx = ai == 0 ? -1 : (ai == 1 ? 1 : 0);
    const int dy = ai == 2 ? -1 : (ai == 3 ? 1 : 0);
    const int sxy = (play && lj == 0) ? ((cx & 0xff) | ((cy & 0xff) << 8)) : xy;
    const LaneSlot s0 = lane_slot(sxy, ot, small);
    const uint32_t moved = group_push_set<GS, false>(p, s0, none, lj, gbase, gmask, play, ai, dx, dy);
    int nxy = sxy;
    if (play && ((moved >> lj) & 1u)) {
      const int x = static_cast<int8_t>(sxy & 0xff) + dx, y = static_cast<int8_t>((sxy >> 8) & 0xff) + dy;
      nxy = (x & 0xff) | ((y & 0xff) << 8);
    }
    const int after = __popcll(__ballot(is_goal_lane && nxy == gxy) & gmask);
    if (play) {
      const uint64_t bit = 1ull << cx;
      if (pass == 1) {
        if (moved == 1u) {
          WALK[ai * a.rows + cy] |= bit;
          discover(cx, cy, ai);
        } else if (moved != 0u) {
          PUSH[ai * a.rows + cy] |= bit;
          npush++;
        }
      } else {
        const uint64_t below = bit - 1ull;
        int64_t k = static_cast<int64_t>(PRE[cy]);
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const uint64_t r = PUSH[q * a.rows + cy];
          k += __popcll(r & below) + ((q < ai && (r & bit)) ? 1 : 0);
        }
        const int64_t row = base + k;
        if (row < a.cap) {
          if (lj == 0) {
            if (a.row_item) a.row_item[row] = item;
            if (a.row_from) reinterpret_cast<int16_t*>(a.row_from)[row] = static_cast<int16_t>(sxy);
            if (a.row_action) a.row_action[row] = static_cast<uint8_t>(ai);
            if (a.row_walk) a.row_walk[row] = d;
            if (a.row_moved) a.row_moved[row] = moved;
            if (a.row_goal) a.row_goal[row] = after == p.G ? 1 : 0;  // (vacuously a goal without goals, trap T8)
          }
          if (a.row_next_pos && lj < a.npad) reinterpret_cast<int16_t*>(a.row_next_pos)[row * a.npad + lj] = static_cast<int16_t>(nxy);
        } else if (lj == 0) {
          n_dropped++;
        }
      }
    }
  }
  if (a.emit && a.dropped && n_dropped) atomicAdd(a.dropped, n_dropped);
}

// the argument checks of both entry points; everything but the last three needs no engine
static int walk_check_args(const PwEngine* e, const int32_t* puzzle_id, int32_t npad, int32_t n, const int64_t* offset,
                           int64_t cap, bool maps, int32_t map_h, int32_t map_w, const char* what) {
  const std::string w = std::string(what) + ": ";
  if (n < 1) return pw_fail(PW_EINVAL, w + "n must be >= 1");
  if (int rc = pw_check_npad(w, npad)) return rc;
  if (!puzzle_id) return pw_fail(PW_EINVAL, w + "null puzzle_id");
  if (!offset) return pw_fail(PW_EINVAL, w + "null offset");
  if (cap < 0) return pw_fail(PW_EINVAL, w + "cap must be >= 0");
  if (maps && (map_h < 1 || map_h > PW_MAX_DIM)) return pw_fail(PW_EINVAL, w + "map_h must be 1 .. PW_MAX_DIM");
  if (maps && (map_w < 1 || map_w > PW_MAX_DIM)) return pw_fail(PW_EINVAL, w + "map_w must be 1 .. PW_MAX_DIM");
  if (!e) return pw_fail(PW_EINVAL, w + "null engine");
  if (npad < e->set->max_n) return pw_fail(PW_EINVAL, w + "npad is smaller than the set's largest number of movables");
  if (maps && map_h < e->set->max_h) return pw_fail(PW_EINVAL, w + "map_h is smaller than the set's largest height");
  if (maps && map_w < e->set->max_w) return pw_fail(PW_EINVAL, w + "map_w is smaller than the set's largest width");
  return PW_OK;
}

static void walk_launch(PwEngine* e, WalkArgs& a, hipStream_t st) {
  a.hdrs = e->set->d_headers;
  a.blob = e->set->d_blob;
  a.ovl = e->d_ovl;
  a.ovl_dir = e->d_ovl_dir;
  a.num_puzzles = e->set->count;
  a.rows = std::min(std::max(e->set->max_h, 1), PW_MAX_DIM);
  // the item counter: the caller's own (pw_push_search.inc), else the next of the replay workspace's
  if (!a.next_item) a.next_item = reinterpret_cast<uint32_t*>(e->d_replay + 64 * (e->replay_seq++ & 63u));
  (void)hipMemsetAsync(a.next_item, 0, 4, st);
  const int tab = e->ovl_puzzles == 0 ? 0 : (e->ovl_puzzles == e->set->count ? 2 : 1);
  const int gs = a.npad <= 8 ? 8 : a.npad;
  // the boards of the wavefront's 64 / GS items: at most 12 * 64 * 8 * 8 = 48 KB
  const size_t lds = static_cast<size_t>(PW_WAVE / gs) * PW_WALK_BOARDS * a.rows * sizeof(uint64_t);
  const int64_t waves = (static_cast<int64_t>(a.n) + (PW_WAVE / gs) - 1) / (PW_WAVE / gs);
  const dim3 grid(static_cast<unsigned>(std::min<int64_t>(waves, 16ll * std::max(e->num_cus, 1)))), block(PW_WAVE);
#define PW_LAUNCH_WALK(GS)                                                                      \
  do {                                                                                          \
    if (tab == 0) hipLaunchKernelGGL((pw_walk_kernel<GS, 0>), grid, block, lds, st, a);         \
    else if (tab == 1) hipLaunchKernelGGL((pw_walk_kernel<GS, 1>), grid, block, lds, st, a);    \
    else hipLaunchKernelGGL((pw_walk_kernel<GS, 2>), grid, block, lds, st, a);                  \
  } while (0)
  if (gs == 8) PW_LAUNCH_WALK(8);
  else if (gs == 16) PW_LAUNCH_WALK(16);
  else PW_LAUNCH_WALK(32);
#undef PW_LAUNCH_WALK
}

extern "C" {

int pw_walk_regions(PwEngine* e, const int32_t* puzzle_id, const int8_t* pos, int32_t npad, const uint8_t* mask, int32_t n,
                    int32_t* region_size, int8_t* canon, int64_t* offset, uint16_t* walk_map, int32_t map_h, int32_t map_w,
                    void* stream) try {
  if (!region_size) return pw_fail(PW_EINVAL, "pw_walk_regions: null region_size");
  if (int rc = walk_check_args(e, puzzle_id, npad, n, offset, 0, walk_map != nullptr, map_h, map_w, "pw_walk_regions")) return rc;
  PwDeviceGuard guard(e->set->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  size_t scan_bytes = 0;
  const size_t count = static_cast<size_t>(n) + 1;
  hipError_t err = rocprim::exclusive_scan(nullptr, scan_bytes, offset, offset, static_cast<int64_t>(0), count,
                                           rocprim::plus<int64_t>(), st);
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string("pw_walk_regions: ") + hipGetErrorString(err));
  scan_bytes = pw_pad256(scan_bytes);
  if (int rc = replay_workspace(e, scan_bytes, "pw_walk_regions")) return rc;
  // every entry of every map: 0xFFFF, the kernel overwrites the positions of the regions
  if (walk_map && hipMemsetAsync(walk_map, 0xff, static_cast<size_t>(n) * map_h * map_w * sizeof(uint16_t), st) != hipSuccess)
    return pw_fail(PW_EDEVICE, "pw_walk_regions: hipMemsetAsync failed");
  WalkArgs a{};
  a.puzzle_id = puzzle_id;
  a.pos = pos;
  a.mask = mask;
  a.n = n;
  a.npad = npad;
  a.emit = 0;
  a.region_size = region_size;
  a.canon = canon;
  a.offset = offset;
  a.walk_map = walk_map;
  a.map_h = map_h;
  a.map_w = map_w;
  walk_launch(e, a, st);
  if (int rc = check_launch("pw_walk_regions")) return rc;
  size_t tmp = e->replay_bytes - kReplayCounterBytes;
  err = rocprim::exclusive_scan(e->d_replay + kReplayCounterBytes, tmp, offset, offset, static_cast<int64_t>(0), count,
                                rocprim::plus<int64_t>(), st);
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string("pw_walk_regions: ") + hipGetErrorString(err));
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_walk_pushes(PwEngine* e, const int32_t* puzzle_id, const int8_t* pos, int32_t npad, const uint8_t* mask, int32_t n,
                   const int64_t* offset, int64_t cap, int32_t* row_item, int8_t* row_from, uint8_t* row_action,
                   int32_t* row_walk, uint32_t* row_moved, uint8_t* row_goal, int8_t* row_next_pos, int64_t* dropped,
                   void* stream) try {
  if (int rc = walk_check_args(e, puzzle_id, npad, n, offset, cap, false, 0, 0, "pw_walk_pushes")) return rc;
  PwDeviceGuard guard(e->set->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (int rc = replay_workspace(e, 0, "pw_walk_pushes")) return rc;
  if (dropped && hipMemsetAsync(dropped, 0, 8, st) != hipSuccess)
    return pw_fail(PW_EDEVICE, "pw_walk_pushes: hipMemsetAsync failed");
  WalkArgs a{};
  a.puzzle_id = puzzle_id;
  a.pos = pos;
  a.mask = mask;
  a.n = n;
  a.npad = npad;
  a.emit = 1;
  a.offset = const_cast<int64_t*>(offset);
  a.cap = cap;
  a.row_item = row_item;
  a.row_from = row_from;
  a.row_action = row_action;
  a.row_walk = row_walk;
  a.row_moved = row_moved;
  a.row_goal = row_goal;
  a.row_next_pos = row_next_pos;
  a.dropped = reinterpret_cast<unsigned long long*>(dropped);
  walk_launch(e, a, st);
  return check_launch("pw_walk_pushes");
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

}  // extern "C"

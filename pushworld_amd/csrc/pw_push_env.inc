// pw_push_env.inc -- K23: a batch of environments stepped by pushes with the push mask and the walk map of the states that are
// left kept per environment (pw_step_push_mask).  Part of the single translation unit pw_kernels.hip (included there after
// pw_push_step.inc: uses K19's status values, the lane-group step helpers and the replay workspace's item counters).
//
// Definitions (include/pushworld_amd.h): the VIEW of an environment is the push mask, the number of push moves, the walk map and
// the region size of one state, with the puzzle id and the positions it was computed for.  It is CURRENT when that id and the
// first N positions are those of the environment.  A current view answers everything pw_step_push floods for: the choice
// (from, a) is valid exactly when a is in 0..3, the map's entry at `from` is not 0xFFFF and bit a of the mask's entry is set;
// dist(from) is the entry's low 12 bits; the agent's position at a max_steps cut is found along the parent actions from `from`.
//
// Per environment, in K15's frame (one wavefront per workgroup, 64 / GS lane groups, one movable per lane, items off a device
// counter, row bitboards in LDS):
//   1. a finished environment under PW_STEP_AUTORESET is reset; otherwise the choice is looked up in the view -- a stale view is
//      rebuilt first by one flood of the state on entry, and the same lookup follows -- and the push is ONE group_push_set, with
//      K19's goal, reward and max_steps rules.  A refused choice changes nothing.
//   2. whenever the state that is left is not the view's, it is flooded (region pass of pw_walk_kernel: every (q, a) verdict is
//      one group_push_set) and the view is written: every entry, none twice by one flood.
//   3. PW_PUSH_END_STUCK truncates an environment that is left without a push move and without a flag.
// In the steady state of a learner -- views current on entry, every choice a push move -- that is one flood per environment and
// call, where pw_step_push followed by pw_push_mask floods twice.
//
// Stores.  Within one flood every address of the view has one writer: the entries of the region are written at discovery by
// the group's first lane, all others when the flood ends, from the visited board, by the lanes in turn.  An item may be
// flooded twice (a stale view on entry, then the state that is left); the two floods write the same addresses from different
// lanes, and the lookup between them reads what the first one wrote: a device-scope fence stands after the first flood (the
// stores have reached L2 and the vector L1 is invalidated before anything that follows).  What is read of the caller's old view
// is read, and waited for, before the item's first store to it.
//
// Seven boards of the set's largest height per item -- visited, current, next, push[4] -- 56 bytes per row, at most
// 7 * 64 * 8 * 8 = 28 KB per workgroup.  Every loop is bounded by the items, the W x H cells of a board times four actions, the
// cells of a map, or dist (at most 4 095: the reward sum and the way back along the parents); every position on that way is
// range-checked, and a link that is 0xFFFF, has a parent outside 0..3 or whose dist does not drop by one makes the view stale
// (it is rebuilt once; nothing the caller hands in can lead to a read out of bounds or an endless loop).  There is no wait on
// another workgroup.

#define PW_PENV_BOARDS 7  // visited, current, next, push[4]

struct PushEnvArgs {
  const PwPuzzleHeader* hdrs;
  const uint8_t* blob;
  const uint64_t* ovl;
  const PwOvlDir* ovl_dir;
  const int32_t* puzzle_id;    // [n]
  const int8_t* push_from;     // [n][2]
  const uint8_t* push_action;  // [n]
  int8_t* pos;                 // [n][npad][2]
  int32_t* steps;
  double* reward;   // or NULL
  int8_t* dgoals;   // or NULL
  uint8_t* term;
  uint8_t* trunc;
  int32_t* moves;   // or NULL
  int8_t* status;   // or NULL
  // the view
  uint8_t* push_mask;    // [n][map_h][map_w]
  int32_t* num_pushes;   // [n]
  uint16_t* walk_map;    // [n][map_h][map_w]
  int32_t* region_size;  // [n]
  int8_t* view_pos;      // [n][npad][2]
  int32_t* view_id;      // [n]
  int32_t map_h, map_w;
  int32_t n, npad, num_puzzles, rows, max_steps;
  uint32_t flags;
  uint32_t* next_item;
  unsigned long long* counters;  // pw_counters' slots
};

template <int GS, int kTab>
__global__ __launch_bounds__(64) void pw_push_env_kernel(PushEnvArgs a) {
  extern __shared__ uint64_t pw_penv_lds[];
  const int lane = threadIdx.x;
  const int lj = lane & (GS - 1);
  const int gbase = lane & ~(GS - 1);
  const unsigned long long gmask = ((1ull << (GS - 1) << 1) - 1ull) << gbase;
  uint64_t* const B = pw_penv_lds + static_cast<size_t>(lane / GS) * PW_PENV_BOARDS * a.rows;
  uint64_t* const VIS = B;
  uint64_t* const CUR = B + a.rows;
  uint64_t* const NXT = B + 2 * a.rows;
  uint64_t* const PUSH = B + 3 * a.rows;  // [4][rows]
  const int cells = a.map_h * a.map_w;

  LanePuzzleT<const uint64_t*, kTab> p;
  const PwPuzzleHeader* h = a.hdrs;
  p.h = h;
  p.wall = p.awall = p.shapes = reinterpret_cast<const uint64_t*>(a.blob + h->base);
  p.pair = nullptr;
  p.wtab = nullptr;
  p.R = p.Hs = 0;
  p.H = p.N = p.G = 0;
  bool active = false, exhausted = false, is_goal_lane = false;
  bool stepped = false;  // the step phase of the item is over: the flood that runs is the one of the state that is left
  bool rebuilt = false;  // the view of the state on entry was rebuilt by this call
  bool f_term = false, f_trunc = false;  // the item's flags as they stand
  int item = 0, spid = 0, xy = 0, gxy = -1;
  int W = 0, aw = 0, ah = 0, q0x = 0, q0y = 0;
  int fx = 0, fy = 0, fa = 0, steps_in = 0;
  // the group's iterator: phase (0 a flood, 1 the push itself), layer, action, row, what is left of the row / of the layer
  int phase = 0, d = 0, ai = 0, cy = 0, dist = 0, rsize = 0, npush = 0;
  uint64_t rowbits = 0, ymask = 0, cur_rows = 0, next_rows = 0;
  uint32_t ot = 0;
  uint64_t small = 0;
  uint32_t c_steps = 0, c_ended = 0, c_solved = 0;  // what this group's items add to pw_counters
  const LaneSlot none = lane_slot(0, 0u, 0ull);

  // a refused choice: the state stays as it was
  auto refuse = [&]() {
    if (lj == 0) {
      if (a.reward) a.reward[item] = 0.0;
      if (a.dgoals) a.dgoals[item] = 0;
      if (a.moves) a.moves[item] = 0;
      if (a.status) a.status[item] = PW_PUSH_REFUSED;
    }
  };
  // the item is done: `np` push moves in the state that is left
  auto finish = [&](int np) {
    if ((a.flags & PW_PUSH_END_STUCK) && np == 0 && !f_term && !f_trunc) {
      if (lj == 0) a.trunc[item] = 1;
      c_ended += 1u;
    }
    active = false;
  };
  // the view of an item that the walk regions skip
  auto skipped_view = [&]() {
    for (int c = lj; c < cells; c += GS) {
      a.push_mask[static_cast<int64_t>(item) * cells + c] = 0;
      a.walk_map[static_cast<int64_t>(item) * cells + c] = 0xFFFFu;
    }
    if (lj < a.npad) reinterpret_cast<int16_t*>(a.view_pos)[static_cast<int64_t>(item) * a.npad + lj] = 0;
    if (lj == 0) {
      a.num_pushes[item] = 0;
      a.region_size[item] = -1;
      a.view_id[item] = -1;
    }
  };
  // a flood of the state in the registers begins: layer 0 is the agent's own position
  auto start_flood = [&]() {
    for (int y = 0; y < p.H; y++) {
      VIS[y] = CUR[y] = NXT[y] = 0ull;
#pragma unroll
      for (int k = 0; k < 4; k++) PUSH[k * a.rows + y] = 0ull;
    }
    VIS[q0y] = CUR[q0y] = 1ull << q0x;
    cur_rows = 1ull << q0y;
    next_rows = 0ull;
    ymask = cur_rows;
    rowbits = 0ull;
    d = 0;
    ai = 0;
    rsize = 1;
    npush = 0;
    phase = 0;
    if (lj == 0) a.walk_map[static_cast<int64_t>(item) * cells + q0y * a.map_w + q0x] = 0;
    active = true;
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
    rsize++;
    if (lj == 0) a.walk_map[static_cast<int64_t>(item) * cells + ny * a.map_w + nx] = static_cast<uint16_t>((d + 1) | (act << 12));
  };
  // the choice looked up in the item's view, which is current: the push itself is next, or the choice is refused
  auto lookup = [&]() {
    const int64_t at = static_cast<int64_t>(item) * cells + fy * a.map_w + fx;
    const uint32_t e = a.walk_map[at];
    const uint32_t m = a.push_mask[at];
    if (e == 0xFFFFu || ((m >> fa) & 1u) == 0u) {
      refuse();
      finish(a.num_pushes[item]);
    } else {
      dist = static_cast<int>(e & 0xFFFu);
      phase = 1;
      active = true;
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
          ot = 0u;
          spid = a.puzzle_id[idx];
          stepped = false;
          rebuilt = false;
          int16_t* prow = reinterpret_cast<int16_t*>(a.pos) + static_cast<int64_t>(idx) * a.npad;
          f_term = a.term[idx] != 0;
          f_trunc = a.trunc[idx] != 0;
          const bool reset = (a.flags & PW_STEP_AUTORESET) && (f_term || f_trunc);
          if (reset) {
            // next-step autoreset, as pw_step_push: this call is the reset() of a finished episode; the choice is not read
            const PwPuzzleHeader* hr = a.hdrs + pw_clamp_pid(spid, a.num_puzzles);
            if (lj < a.npad) prow[lj] = (lj < hr->N) ? reinterpret_cast<const int16_t*>(hr->init)[lj] : static_cast<int16_t>(0);
            if (lj == 0) {
              a.steps[idx] = 0;
              a.term[idx] = 0;
              a.trunc[idx] = 0;
              if (a.reward) a.reward[idx] = 0.0;
              if (a.dgoals) a.dgoals[idx] = 0;
              if (a.moves) a.moves[idx] = 0;
              if (a.status) a.status[idx] = PW_PUSH_RESET;
            }
            f_term = f_trunc = false;
            stepped = true;
          }
          bool skip = spid < 0 || spid >= a.num_puzzles;
          int N = 0;
          if (!skip) {
            h = a.hdrs + spid;
            N = h->N;
            if (lj < N) {  // every movable inside its grid (pw_validate_state's range test); nothing past N is read
              xy = reset ? static_cast<int>(reinterpret_cast<const uint16_t*>(h->init)[lj]) : static_cast<int>(static_cast<uint16_t>(prow[lj]));
              ot = reinterpret_cast<const uint32_t*>(h->objtab)[lj];
            }
            const int x = static_cast<int8_t>(xy & 0xff), y = static_cast<int8_t>((xy >> 8) & 0xff);
            const bool bad = lj < N && (x < 0 || y < 0 || x + static_cast<int>(ot & 0xffu) > h->W ||
                                        y + static_cast<int>((ot >> 8) & 0xffu) > h->H);
            skip = (__ballot(bad) & gmask) != 0ull;
          }
          if (skip) {
            if (!reset) refuse();
            skipped_view();
            finish(0);
          } else {
            const uint8_t* b = a.blob + h->base;
            p.h = h;
            p.wall = reinterpret_cast<const uint64_t*>(b + h->off_wall);
            p.awall = reinterpret_cast<const uint64_t*>(b + h->off_awall);
            p.shapes = reinterpret_cast<const uint64_t*>(b + h->off_shapes);
            lane_tables(p, a.ovl, a.ovl_dir, spid);
            p.H = min(static_cast<int>(h->H), a.rows);  // (a.rows is the set's largest height: never the smaller one)
            p.N = N;
            p.G = h->G;
            W = h->W;
            small = (lj < N) ? reinterpret_cast<const uint64_t*>(b + h->off_small)[lj] : 0ull;
            is_goal_lane = lj >= 1 && lj <= p.G;
            gxy = is_goal_lane ? static_cast<int>(reinterpret_cast<const uint16_t*>(h->goal)[lj - 1]) : -1;
            const int axy = __shfl(xy, gbase, PW_WAVE);
            const uint32_t aot = static_cast<uint32_t>(__shfl(static_cast<int>(ot), gbase, PW_WAVE));
            q0x = axy & 0xff;
            q0y = (axy >> 8) & 0xff;
            aw = static_cast<int>(aot & 0xffu);
            ah = static_cast<int>((aot >> 8) & 0xffu);
            steps_in = reset ? 0 : a.steps[idx];
            // is the view current?  The id, and the first N pairs (nothing beyond N is compared)
            const bool differs = lj < N && static_cast<int>(reinterpret_cast<const uint16_t*>(a.view_pos)[static_cast<int64_t>(idx) * a.npad + lj]) != xy;
            const bool same_pos = (__ballot(differs) & gmask) == 0ull;
            const bool current = same_pos && a.view_id[idx] == spid;
            bool choice = false;
            if (!reset) {
              fx = a.push_from[2 * static_cast<int64_t>(idx)];
              fy = a.push_from[2 * static_cast<int64_t>(idx) + 1];
              fa = a.push_action[idx];
              // an action outside 0..3 or a position at which the agent leaves its grid: no push move
              choice = !(fa > 3 || fx < 0 || fy < 0 || fx + aw > W || fy + ah > p.H || fx >= a.map_w || fy >= a.map_h);
              if (!choice) {
                refuse();
                stepped = true;
              }
            }
            if (!current) start_flood();  // (of the state on entry when a choice waits: the rebuild)
            else if (choice) lookup();
            else finish(a.num_pushes[idx]);
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
        if (next_rows != 0ull) {
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
          continue;
        }
        // the flood is over: the view of the state in the registers.  Every entry outside the region, and the mask everywhere
        // (a lane reads the boards' words it wrote itself: every lane of the group wrote all of them)
        for (int c = lj; c < cells; c += GS) {
          const int y = c / a.map_w, x = c - y * a.map_w;
          uint32_t m = 0u;
          bool in = false;
          if (y < p.H && x < 64) {
            m = static_cast<uint32_t>(((PUSH[y] >> x) & 1ull) | (((PUSH[a.rows + y] >> x) & 1ull) << 1) |
                                      (((PUSH[2 * a.rows + y] >> x) & 1ull) << 2) | (((PUSH[3 * a.rows + y] >> x) & 1ull) << 3));
            in = ((VIS[y] >> x) & 1ull) != 0ull;
          }
          a.push_mask[static_cast<int64_t>(item) * cells + c] = static_cast<uint8_t>(m);
          if (!in) a.walk_map[static_cast<int64_t>(item) * cells + c] = 0xFFFFu;
        }
        if (lj < a.npad) reinterpret_cast<int16_t*>(a.view_pos)[static_cast<int64_t>(item) * a.npad + lj] = (lj < p.N) ? static_cast<int16_t>(xy) : static_cast<int16_t>(0);
        if (lj == 0) {
          a.num_pushes[item] = npush;
          a.region_size[item] = rsize;
          a.view_id[item] = spid;
        }
        if (stepped) {
          finish(npush);
        } else {
          // the rebuilt view of the state on entry: its stores before the lookup's loads, and before the second flood's stores
          rebuilt = true;
          __threadfence();
          lookup();
        }
        break;
      }
      if (active && phase == 1) {
        have = true;
        cx = fx;
        cy = fy;
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
    const int act = (phase == 1 ? fa : ai) & 3;  // (a group that plays nothing may hold a refused action: never an index)
    const int dx = act == 0 ? -1 : (act == 1 ? 1 : 0);
    const int dy = act == 2 ? -1 : (act == 3 ? 1 : 0);
    const int sxy = (play && lj == 0) ? ((cx & 0xff) | ((cy & 0xff) << 8)) : xy;
    const LaneSlot s0 = lane_slot(sxy, ot, small);
    const uint32_t moved = group_push_set<GS, false>(p, s0, none, lj, gbase, gmask, play, act, dx, dy);
    int nxy = sxy;
    if (play && ((moved >> lj) & 1u)) {
      const int x = static_cast<int8_t>(sxy & 0xff) + dx, y = static_cast<int8_t>((sxy >> 8) & 0xff) + dy;
      nxy = (x & 0xff) | ((y & 0xff) << 8);
    }
    // (the agent is no goal lane: `before` is the count of the state on entry and of every state of the walk)
    const int before = __popcll(__ballot(is_goal_lane && xy == gxy) & gmask);
    const int after = __popcll(__ballot(is_goal_lane && nxy == gxy) & gmask);
    if (play && phase == 0) {
      if (moved == 1u) {
        discover(cx, cy, ai);
      } else if (moved != 0u) {
        PUSH[ai * a.rows + cy] |= 1ull << cx;
        npush++;
      }
    } else if (play) {
      if (moved == 0u || moved == 1u) {
        // (a view that is current by id and positions but was not written by this function: the step function decides)
        refuse();
        finish(a.num_pushes[item]);
      } else {
        const int64_t total = static_cast<int64_t>(dist) + 1;
        const int64_t left = static_cast<int64_t>(a.max_steps) - steps_in;
        const int64_t cut = a.max_steps >= 0 ? (left > 1 ? left : 1) : total;  // the first step that returns truncated
        const bool at_goal = before == p.G;  // the first walking step of a goal state returns terminated (vacuously without goals)
        const int n = static_cast<int>((at_goal && dist > 0) ? 1 : (cut < total ? cut : total));
        const bool done = n == total;
        int x = fx, y = fy;  // the ancestor of `from` in layer n, along the parent actions of the map
        bool sound = true;
        if (!done) {
          const uint16_t* map = a.walk_map + static_cast<int64_t>(item) * cells;
          for (int k = dist; k > n; k--) {
            const uint32_t e = map[y * a.map_w + x];
            const int pa = static_cast<int>(e >> 12);
            if (e == 0xFFFFu || static_cast<int>(e & 0xFFFu) != k || pa > 3) {
              sound = false;
              break;
            }
            x -= pa == 0 ? -1 : (pa == 1 ? 1 : 0);
            y -= pa == 2 ? -1 : (pa == 3 ? 1 : 0);
            if (x < 0 || y < 0 || x + aw > W || y + ah > p.H || x >= a.map_w || y >= a.map_h) {
              sound = false;
              break;
            }
          }
          if (sound) {
            const uint32_t e = map[y * a.map_w + x];
            sound = e != 0xFFFFu && static_cast<int>(e & 0xFFFu) == n;
          }
        }
        if (!sound && !rebuilt) {
          start_flood();  // a broken link: the view is stale; the state on entry is flooded and the lookup follows again
        } else if (!sound) {
          refuse();  // (not reached: the map was written by this item's own flood)
          finish(a.num_pushes[item]);
        } else {
          double r = 0.0;  // ((r1 + r2) + r3) + ...: sequential float64 additions in execution order (0.0 + r1 is r1)
          bool term;
          int dg = 0;
          int16_t* prow = reinterpret_cast<int16_t*>(a.pos) + static_cast<int64_t>(item) * a.npad;
          if (done) {
            for (int k = 0; k < dist; k++) r += static_cast<double>(0) - 0.01;
            term = after == p.G;
            dg = after - before;
            r += term ? 10.0 : static_cast<double>(dg) - 0.01;  // gym_env.py:212-221
            if (lj < p.N && ((moved >> lj) & 1u)) {
              prow[lj] = static_cast<int16_t>(nxy);
              xy = nxy;
            }
          } else {
            term = at_goal;
            if (term) r = 10.0;
            else
              for (int k = 0; k < n; k++) r += static_cast<double>(0) - 0.01;
            if (lj == 0) {
              xy = (x & 0xff) | ((y & 0xff) << 8);
              prow[0] = static_cast<int16_t>(xy);
            }
          }
          const int64_t steps_out = static_cast<int64_t>(steps_in) + n;
          const bool trunc = a.max_steps >= 0 && steps_out >= a.max_steps;
          if (lj == 0) {
            a.steps[item] = static_cast<int32_t>(steps_out);
            a.term[item] = term ? 1 : 0;
            a.trunc[item] = trunc ? 1 : 0;
            if (a.reward) a.reward[item] = r;
            if (a.dgoals) a.dgoals[item] = static_cast<int8_t>(dg);
            if (a.moves) a.moves[item] = n;
            if (a.status) a.status[item] = done ? PW_PUSH_DONE : PW_PUSH_CUT;
          }
          c_steps += static_cast<uint32_t>(n);
          c_ended += (term || trunc) ? 1u : 0u;
          c_solved += term ? 1u : 0u;
          f_term = term;
          f_trunc = trunc;
          // the state that is left: the agent moved, so the view is stale
          const int axy = __shfl(xy, gbase, PW_WAVE);
          q0x = axy & 0xff;
          q0y = (axy >> 8) & 0xff;
          stepped = true;
          // a push may carry a movable out of its grid (states with overlaps): the walk regions skip such a state
          const int mx = static_cast<int8_t>(xy & 0xff), my = static_cast<int8_t>((xy >> 8) & 0xff);
          const bool bad = lj < p.N && (mx < 0 || my < 0 || mx + static_cast<int>(ot & 0xffu) > W ||
                                        my + static_cast<int>((ot >> 8) & 0xffu) > p.H);
          if ((__ballot(bad) & gmask) != 0ull) {
            skipped_view();
            finish(0);
          } else {
            // (after a rebuild this is the item's second flood: the fence behind the first one stands between their stores)
            start_flood();
          }
        }
      }
    }
  }
  // pw_counters: what the executed primitive steps would have added (fire and forget, one slot per workgroup)
  if (lj == 0) {
    unsigned long long* slot = a.counters + (blockIdx.x & (PW_COUNTER_SLOTS - 1)) * 8u;
    if (c_steps) atomicAdd(slot, static_cast<unsigned long long>(c_steps));
    if (c_ended) atomicAdd(slot + 1, static_cast<unsigned long long>(c_ended));
    if (c_solved) atomicAdd(slot + 2, static_cast<unsigned long long>(c_solved));
  }
}

extern "C" {

int pw_step_push_mask(PwEngine* e, const int32_t* puzzle_id, const int8_t* push_from, const uint8_t* push_action, int8_t* pos,
                      int32_t* steps, double* reward, int8_t* dgoals, uint8_t* terminated, uint8_t* truncated, int32_t* moves,
                      int8_t* status, uint8_t* push_mask, int32_t* num_pushes, uint16_t* walk_map, int32_t* region_size,
                      int8_t* view_pos, int32_t* view_id, int32_t map_h, int32_t map_w, int32_t batch, uint32_t flags,
                      void* stream) try {
  if (!e) return pw_fail(PW_EINVAL, "pw_step_push_mask: null engine");
  if (!puzzle_id) return pw_fail(PW_EINVAL, "pw_step_push_mask: null puzzle_id");
  if (!push_from) return pw_fail(PW_EINVAL, "pw_step_push_mask: null push_from");
  if (!push_action) return pw_fail(PW_EINVAL, "pw_step_push_mask: null push_action");
  if (!pos) return pw_fail(PW_EINVAL, "pw_step_push_mask: null pos");
  if (!steps) return pw_fail(PW_EINVAL, "pw_step_push_mask: null steps");
  if (!terminated) return pw_fail(PW_EINVAL, "pw_step_push_mask: null terminated");
  if (!truncated) return pw_fail(PW_EINVAL, "pw_step_push_mask: null truncated");
  if (!push_mask) return pw_fail(PW_EINVAL, "pw_step_push_mask: null push_mask");
  if (!num_pushes) return pw_fail(PW_EINVAL, "pw_step_push_mask: null num_pushes");
  if (!walk_map) return pw_fail(PW_EINVAL, "pw_step_push_mask: null walk_map");
  if (!region_size) return pw_fail(PW_EINVAL, "pw_step_push_mask: null region_size");
  if (!view_pos) return pw_fail(PW_EINVAL, "pw_step_push_mask: null view_pos");
  if (!view_id) return pw_fail(PW_EINVAL, "pw_step_push_mask: null view_id");
  if (batch < 1) return pw_fail(PW_EINVAL, "pw_step_push_mask: batch must be >= 1");
  if (map_h < 1 || map_h > PW_MAX_DIM) return pw_fail(PW_EINVAL, "pw_step_push_mask: map_h must be 1 .. PW_MAX_DIM");
  if (map_w < 1 || map_w > PW_MAX_DIM) return pw_fail(PW_EINVAL, "pw_step_push_mask: map_w must be 1 .. PW_MAX_DIM");
  if (e->mailbox)
    return pw_fail(PW_EINVAL, "pw_step_push_mask: this engine has an open mailbox (pw_mailbox_open): its environments live in the resident kernel until pw_mailbox_close");
  const int np = e->np;
  if ((np != 4 && np != 8 && np != 16 && np != 32) || np < e->set->max_n)
    return pw_fail(PW_EINVAL, "pw_step_push_mask: the engine's pos layout holds more than 32 movables");
  if (map_h < e->set->max_h) return pw_fail(PW_EINVAL, "pw_step_push_mask: map_h is smaller than the set's largest height");
  if (map_w < e->set->max_w) return pw_fail(PW_EINVAL, "pw_step_push_mask: map_w is smaller than the set's largest width");
  PwDeviceGuard guard(e->set->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  // the only workspace: the replay workspace's item counters (4 KB, allocated by the first call of any of its users)
  if (int rc = replay_workspace(e, 0, "pw_step_push_mask")) return rc;
  PushEnvArgs a{};
  a.hdrs = e->set->d_headers;
  a.blob = e->set->d_blob;
  a.ovl = e->d_ovl;
  a.ovl_dir = e->d_ovl_dir;
  a.puzzle_id = puzzle_id;
  a.push_from = push_from;
  a.push_action = push_action;
  a.pos = pos;
  a.steps = steps;
  a.reward = reward;
  a.dgoals = dgoals;
  a.term = terminated;
  a.trunc = truncated;
  a.moves = moves;
  a.status = status;
  a.push_mask = push_mask;
  a.num_pushes = num_pushes;
  a.walk_map = walk_map;
  a.region_size = region_size;
  a.view_pos = view_pos;
  a.view_id = view_id;
  a.map_h = map_h;
  a.map_w = map_w;
  a.n = batch;
  a.npad = np;
  a.num_puzzles = e->set->count;
  a.rows = std::min(std::max(e->set->max_h, 1), PW_MAX_DIM);
  a.max_steps = e->cfg.max_steps;
  a.flags = flags;
  a.next_item = reinterpret_cast<uint32_t*>(e->d_replay + 64 * (e->replay_seq++ & 63u));
  a.counters = e->d_counters;
  // (the item counter's four bytes, as pw_step_push: a memset node, not a fill of the view)
  if (hipMemsetAsync(a.next_item, 0, 4, st) != hipSuccess) return pw_fail(PW_EDEVICE, "pw_step_push_mask: hipMemsetAsync failed");
  const int tab = e->ovl_puzzles == 0 ? 0 : (e->ovl_puzzles == e->set->count ? 2 : 1);
  const int gs = np <= 8 ? 8 : np;
  // the boards of the wavefront's 64 / GS items: at most 7 * 64 * 8 * 8 = 28 KB
  const size_t lds = static_cast<size_t>(PW_WAVE / gs) * PW_PENV_BOARDS * a.rows * sizeof(uint64_t);
  const int64_t waves = (static_cast<int64_t>(batch) + (PW_WAVE / gs) - 1) / (PW_WAVE / gs);
  const dim3 grid(static_cast<unsigned>(std::min<int64_t>(waves, 16ll * std::max(e->num_cus, 1)))), block(PW_WAVE);
#define PW_LAUNCH_PENV(GS)                                                                       \
  do {                                                                                           \
    if (tab == 0) hipLaunchKernelGGL((pw_push_env_kernel<GS, 0>), grid, block, lds, st, a);      \
    else if (tab == 1) hipLaunchKernelGGL((pw_push_env_kernel<GS, 1>), grid, block, lds, st, a); \
    else hipLaunchKernelGGL((pw_push_env_kernel<GS, 2>), grid, block, lds, st, a);               \
  } while (0)
  if (gs == 8) PW_LAUNCH_PENV(8);
  else if (gs == 16) PW_LAUNCH_PENV(16);
  else PW_LAUNCH_PENV(32);
#undef PW_LAUNCH_PENV
  return check_launch("pw_step_push_mask");
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

}  // extern "C"

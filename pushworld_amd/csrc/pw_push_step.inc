// pw_push_step.inc -- K19: a batch of environments stepped by pushes (pw_step_push), and the dense push mask (pw_push_mask).
// Part of the single translation unit pw_kernels.hip (included there after pw_walk.inc: uses its frame, its argument checks,
// its launch and the replay workspace's item counters).
//
// Definitions (include/pushworld_amd.h): a choice (from, a) of a live environment is valid when a is in 0..3, from lies in the
// walk region R and (from, a) is a push move.  Its macro step is pw_step applied with the parent actions from the agent's
// position to `from` and then a, without autoreset inside, ended by the first step that returns terminated | truncated.
//
// Walking changes no movable but the agent, so a walking step gives -0.01 and no flag unless the state on entry is a goal state
// (then the first one terminates) or max_steps is reached.  The outputs therefore follow from the state on entry, dist(from),
// the position on the path at the cut and the push's own step: the kernel floods the region layer by layer until `from` is
// discovered (pw_walk_kernel's frame: one wavefront per workgroup, 64 / GS lane groups, one movable per lane, items off a
// device counter, row bitboards in LDS), evaluates (from, a) ONCE with group_push_set and applies the goal, reward and
// max_steps rules.  Every (q, a) verdict of the flood is one group_push_set as well: no second copy of the dynamics.
//
// The path ancestor a cut needs is kept in LDS: two more boards hold the two bits of every discovered cell's parent action
// (the action of its first discovery: layers in order, actions in order inside a layer, so the lowest one).  Five boards of the
// set's largest height per item -- visited, current, next, parent bit 0, parent bit 1 -- 40 bytes per row, at most
// 5 * 64 * 8 * 8 = 20 KB per workgroup; no per-environment workspace in HBM at any batch size.
//
// Every loop is bounded by the items, the W x H cells of a board times four actions, the rows of a board, or the layers of a
// region (at most 4 095: the reward sum and the walk back along the path); there is no wait on another workgroup.

#define PW_PSTEP_BOARDS 5  // visited, current, next, parent bit 0, parent bit 1

struct PushStepArgs {
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
  int32_t n, npad, num_puzzles, rows, max_steps;
  uint32_t flags;
  uint32_t* next_item;
  unsigned long long* counters;  // pw_counters' slots
};

template <int GS, int kTab>
__global__ __launch_bounds__(64) void pw_push_step_kernel(PushStepArgs a) {
  extern __shared__ uint64_t pw_pstep_lds[];
  const int lane = threadIdx.x;
  const int lj = lane & (GS - 1);
  const int gbase = lane & ~(GS - 1);
  const unsigned long long gmask = ((1ull << (GS - 1) << 1) - 1ull) << gbase;
  uint64_t* const B = pw_pstep_lds + static_cast<size_t>(lane / GS) * PW_PSTEP_BOARDS * a.rows;
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
  bool active = false, exhausted = false, is_goal_lane = false;
  int item = 0, xy = 0, gxy = -1;
  int W = 0, aw = 0, ah = 0, q0x = 0, q0y = 0;
  int fx = 0, fy = 0, fa = 0, steps_in = 0;
  // the group's iterator: phase (0 the flood, 1 the push itself), layer, action, row, what is left of the row / of the layer
  int phase = 0, d = 0, ai = 0, cy = 0, dist = 0;
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
          int16_t* prow = reinterpret_cast<int16_t*>(a.pos) + static_cast<int64_t>(idx) * a.npad;
          if ((a.flags & PW_STEP_AUTORESET) && (a.term[idx] | a.trunc[idx]) != 0) {
            // next-step autoreset, as pw_step: this call is the reset() of a finished episode; the choice is not read
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
          } else {
            bool skip = spid < 0 || spid >= a.num_puzzles;
            int N = 0;
            if (!skip) {
              h = a.hdrs + spid;
              N = h->N;
              if (lj < N) {  // every movable inside its grid (pw_validate_state's range test); nothing past N is read
                xy = static_cast<uint16_t>(prow[lj]);
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
              is_goal_lane = lj >= 1 && lj <= p.G;
              gxy = is_goal_lane ? static_cast<int>(reinterpret_cast<const uint16_t*>(h->goal)[lj - 1]) : -1;
              steps_in = a.steps[idx];
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
      if (moved == 1u) discover(cx, cy, ai);
    } else if (play) {
      if (moved == 0u || moved == 1u) {  // a step that displaces nothing, or a walk move
        refuse();
      } else {
        const int64_t total = static_cast<int64_t>(dist) + 1;
        const int64_t left = static_cast<int64_t>(a.max_steps) - steps_in;
        const int64_t cut = a.max_steps >= 0 ? (left > 1 ? left : 1) : total;  // the first step that returns truncated
        const bool at_goal = before == p.G;  // the first walking step of a goal state returns terminated (vacuously without goals)
        const int n = static_cast<int>((at_goal && dist > 0) ? 1 : (cut < total ? cut : total));
        const bool done = n == total;
        double r = 0.0;  // ((r1 + r2) + r3) + ...: sequential float64 additions in execution order (0.0 + r1 is r1)
        bool term;
        int dg = 0;
        int16_t* prow = reinterpret_cast<int16_t*>(a.pos) + static_cast<int64_t>(item) * a.npad;
        if (done) {
          for (int k = 0; k < dist; k++) r += static_cast<double>(0) - 0.01;
          term = after == p.G;
          dg = after - before;
          r += term ? 10.0 : static_cast<double>(dg) - 0.01;  // gym_env.py:212-221
          if (lj < p.N && ((moved >> lj) & 1u)) prow[lj] = static_cast<int16_t>(nxy);
        } else {
          term = at_goal;
          if (term) r = 10.0;
          else
            for (int k = 0; k < n; k++) r += static_cast<double>(0) - 0.01;
          int x = fx, y = fy;  // the ancestor of `from` in layer n, along the parent actions
          for (int k = dist; k > n; k--) {
            const int pa = static_cast<int>((PAR0[y] >> x) & 1ull) | (static_cast<int>((PAR1[y] >> x) & 1ull) << 1);
            x -= pa == 0 ? -1 : (pa == 1 ? 1 : 0);
            y -= pa == 2 ? -1 : (pa == 3 ? 1 : 0);
          }
          if (lj == 0) prow[0] = static_cast<int16_t>((x & 0xff) | ((y & 0xff) << 8));
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
        active = false;
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

int pw_step_push(PwEngine* e, const int32_t* puzzle_id, const int8_t* push_from, const uint8_t* push_action, int8_t* pos,
                 int32_t* steps, double* reward, int8_t* dgoals, uint8_t* terminated, uint8_t* truncated, int32_t* moves,
                 int8_t* status, int32_t batch, uint32_t flags, void* stream) try {
  if (!e) return pw_fail(PW_EINVAL, "pw_step_push: null engine");
  if (!puzzle_id) return pw_fail(PW_EINVAL, "pw_step_push: null puzzle_id");
  if (!push_from) return pw_fail(PW_EINVAL, "pw_step_push: null push_from");
  if (!push_action) return pw_fail(PW_EINVAL, "pw_step_push: null push_action");
  if (!pos) return pw_fail(PW_EINVAL, "pw_step_push: null pos");
  if (!steps) return pw_fail(PW_EINVAL, "pw_step_push: null steps");
  if (!terminated) return pw_fail(PW_EINVAL, "pw_step_push: null terminated");
  if (!truncated) return pw_fail(PW_EINVAL, "pw_step_push: null truncated");
  if (batch < 1) return pw_fail(PW_EINVAL, "pw_step_push: batch must be >= 1");
  if (e->mailbox)
    return pw_fail(PW_EINVAL, "pw_step_push: this engine has an open mailbox (pw_mailbox_open): its environments live in the resident kernel until pw_mailbox_close");
  const int np = e->np;
  if ((np != 4 && np != 8 && np != 16 && np != 32) || np < e->set->max_n)
    return pw_fail(PW_EINVAL, "pw_step_push: the engine's pos layout holds more than 32 movables");
  PwDeviceGuard guard(e->set->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  // the only workspace: the replay workspace's item counters (4 KB, allocated by the first call of any of its users)
  if (int rc = replay_workspace(e, 0, "pw_step_push")) return rc;
  PushStepArgs a{};
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
  a.n = batch;
  a.npad = np;
  a.num_puzzles = e->set->count;
  a.rows = std::min(std::max(e->set->max_h, 1), PW_MAX_DIM);
  a.max_steps = e->cfg.max_steps;
  a.flags = flags;
  a.next_item = reinterpret_cast<uint32_t*>(e->d_replay + 64 * (e->replay_seq++ & 63u));
  a.counters = e->d_counters;
  if (hipMemsetAsync(a.next_item, 0, 4, st) != hipSuccess) return pw_fail(PW_EDEVICE, "pw_step_push: hipMemsetAsync failed");
  const int tab = e->ovl_puzzles == 0 ? 0 : (e->ovl_puzzles == e->set->count ? 2 : 1);
  const int gs = np <= 8 ? 8 : np;
  // the boards of the wavefront's 64 / GS items: at most 5 * 64 * 8 * 8 = 20 KB
  const size_t lds = static_cast<size_t>(PW_WAVE / gs) * PW_PSTEP_BOARDS * a.rows * sizeof(uint64_t);
  const int64_t waves = (static_cast<int64_t>(batch) + (PW_WAVE / gs) - 1) / (PW_WAVE / gs);
  const dim3 grid(static_cast<unsigned>(std::min<int64_t>(waves, 16ll * std::max(e->num_cus, 1)))), block(PW_WAVE);
#define PW_LAUNCH_PSTEP(GS)                                                                        \
  do {                                                                                             \
    if (tab == 0) hipLaunchKernelGGL((pw_push_step_kernel<GS, 0>), grid, block, lds, st, a);       \
    else if (tab == 1) hipLaunchKernelGGL((pw_push_step_kernel<GS, 1>), grid, block, lds, st, a);  \
    else hipLaunchKernelGGL((pw_push_step_kernel<GS, 2>), grid, block, lds, st, a);                \
  } while (0)
  if (gs == 8) PW_LAUNCH_PSTEP(8);
  else if (gs == 16) PW_LAUNCH_PSTEP(16);
  else PW_LAUNCH_PSTEP(32);
#undef PW_LAUNCH_PSTEP
  return check_launch("pw_step_push");
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_push_mask(PwEngine* e, const int32_t* puzzle_id, const int8_t* pos, int32_t npad, const uint8_t* mask, int32_t n,
                 uint8_t* push_mask, int32_t* num_pushes, int32_t map_h, int32_t map_w, void* stream) try {
  if (!push_mask) return pw_fail(PW_EINVAL, "pw_push_mask: null push_mask");
  // (offset is not used here: the checks see a stand-in that is never read)
  if (int rc = walk_check_args(e, puzzle_id, npad, n, reinterpret_cast<const int64_t*>(push_mask), 0, true, map_h, map_w, "pw_push_mask"))
    return rc;
  PwDeviceGuard guard(e->set->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (int rc = replay_workspace(e, 0, "pw_push_mask")) return rc;
  // every entry of every item: 0, the kernel overwrites the positions that have a push move
  if (hipMemsetAsync(push_mask, 0, static_cast<size_t>(n) * map_h * map_w, st) != hipSuccess)
    return pw_fail(PW_EDEVICE, "pw_push_mask: hipMemsetAsync failed");
  WalkArgs a{};
  a.puzzle_id = puzzle_id;
  a.pos = pos;
  a.mask = mask;
  a.n = n;
  a.npad = npad;
  a.emit = 0;
  a.map_h = map_h;
  a.map_w = map_w;
  a.push_mask = push_mask;
  a.num_pushes = num_pushes;
  walk_launch(e, a, st);
  return check_launch("pw_push_mask");
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

}  // extern "C"

// pw_plan_replay.inc -- K11: ragged replay of a batch of plans into verdicts and flat (state, action, reward, done) rows.
// Part of the single translation unit pw_kernels.hip (included there; uses the lane-group step helpers of pw_step_kernels.inc).
//
// The inputs are what pw_plan_batch_run / pw_plan_batch_run_states leave in device memory (plans uint8 [n][plan_cap],
// plan_len int32 [n]) plus the start states in the engine's pos layout.  One wavefront per workgroup holds 64 / GS lane
// groups (GS = 8 / 16 / 32 lanes for N_pad <= 8 / 16 / 32, one movable per lane); every lane group takes items off a device
// counter and replays its item's plan with group_push_set -- the push-set logic of pw_step -- one action after the other.  A
// lane group that finishes its item takes the next one while its neighbours go on with theirs, so a wavefront is busy until
// the counter runs out; plan lengths are ragged (6 .. 421 actions in the human solutions).
//
//   check   verdict / first_goal / final_pos per item, and the rows the item will emit into offset[i]; offset[n] = 0.  An
//           in-place rocPRIM exclusive scan over n + 1 values turns the counts into row offsets (offset[n] = total).
//   emit    row offset[i] + t of every included item i: the state before action t (padding zeroed: pw_render's layout), the
//           action, pw_step's reward and terminated flag of that step, optionally the state after it.  A lane group's
//           2 * N_pad position bytes of a row are one contiguous store of the group's lanes.
//
// Every loop is bounded by the items and their plan_len <= plan_cap; there is no wait on another workgroup.
#include <rocprim/device/device_scan.hpp>

struct ReplayArgs {
  const PwPuzzleHeader* hdrs;
  const uint8_t* blob;
  const uint64_t* ovl;
  const PwOvlDir* ovl_dir;
  const int32_t* puzzle_id;  // [n]
  const int8_t* pos;         // [n][npad][2] or NULL (initial states)
  const uint8_t* plans;      // [n][plan_cap]
  const int32_t* plan_len;   // [n]
  const uint8_t* mask;       // [n] or NULL
  int32_t n, npad, plan_cap, num_puzzles, include, emit;
  uint32_t* next_item;
  // check: written; emit: verdict and offset are read
  int8_t* verdict;
  int32_t* first_goal;
  int8_t* final_pos;
  int64_t* offset;
  // emit
  int64_t cap;
  int32_t* row_item;
  int32_t* row_t;
  int32_t* row_puzzle_id;
  int8_t* row_pos;
  uint8_t* row_action;
  double* row_reward;
  uint8_t* row_done;
  int8_t* row_next_pos;
  unsigned long long* dropped;
};

__device__ __forceinline__ bool replay_included(int verdict, int include) {
  return verdict == PW_REPLAY_VALID ||
         (include == PW_REPLAY_INCLUDE_REPLAYED && (verdict == PW_REPLAY_NOT_GOAL || verdict == PW_REPLAY_EARLY));
}

template <int GS, int kTab>
__global__ __launch_bounds__(64) void pw_plan_replay_kernel(ReplayArgs a) {
  const int lane = threadIdx.x;
  const int lj = lane & (GS - 1);
  const int gbase = lane & ~(GS - 1);
  const unsigned long long gmask = ((1ull << (GS - 1) << 1) - 1ull) << gbase;
  if (!a.emit && blockIdx.x == 0 && lane == 0) a.offset[a.n] = 0;  // the scan's last input: offset[n] becomes the total

  // the lane group's item (all of it group-uniform except xy / ot / small / gxy, which are per movable)
  LanePuzzleT<const uint64_t*, kTab> p;
  const PwPuzzleHeader* h = a.hdrs;
  p.h = h;
  p.wall = p.awall = p.shapes = reinterpret_cast<const uint64_t*>(a.blob + h->base);
  p.pair = nullptr;
  p.wtab = nullptr;
  p.R = p.Hs = 0;
  p.H = p.N = p.G = 0;
  bool active = false, exhausted = false, is_goal_lane = false;
  int item = 0, pid = 0, t = 0, len = 0, first = -1, xy = 0, gxy = -1, chunk = 0;
  uint32_t ot = 0;
  uint64_t small = 0;
  int64_t base = 0;
  const uint8_t* plan = a.plans;
  unsigned long long n_dropped = 0;
  const LaneSlot none = lane_slot(0, 0u, 0ull);

  // what an item leaves behind when its replay ends (or never starts): check only
  auto finish = [&](int verdict, int first_goal, bool replayed) {
    if (a.emit) return;
    if (lj == 0) {
      a.verdict[item] = static_cast<int8_t>(verdict);
      if (a.first_goal) a.first_goal[item] = first_goal;
      a.offset[item] = replay_included(verdict, a.include) ? static_cast<int64_t>(len) : 0;
    }
    if (a.final_pos && lj < a.npad)
      reinterpret_cast<int16_t*>(a.final_pos)[static_cast<int64_t>(item) * a.npad + lj] = static_cast<int16_t>(replayed ? xy : 0);
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
          len = 0;
          xy = 0;
          const int spid = a.puzzle_id[idx];
          bool skip = (a.mask && a.mask[idx] == 0) || spid < 0 || spid >= a.num_puzzles;
          if (a.emit && !skip) skip = !replay_included(a.verdict[idx], a.include);
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
            finish(PW_REPLAY_SKIPPED, -1, false);
          } else {
            const int l = a.plan_len[idx];
            if (l < 0) {
              finish(PW_REPLAY_NONE, -1, false);
            } else if (l > a.plan_cap) {
              finish(PW_REPLAY_CUT, -1, false);
            } else {
              len = l;
              const uint8_t* b = a.blob + h->base;
              p.h = h;
              p.wall = reinterpret_cast<const uint64_t*>(b + h->off_wall);
              p.awall = reinterpret_cast<const uint64_t*>(b + h->off_awall);
              p.shapes = reinterpret_cast<const uint64_t*>(b + h->off_shapes);
              lane_tables(p, a.ovl, a.ovl_dir, pid);
              p.H = h->H;
              p.N = N;
              p.G = h->G;
              if (lj >= N) ot = 0u;
              small = (lj < N) ? reinterpret_cast<const uint64_t*>(b + h->off_small)[lj] : 0ull;
              is_goal_lane = lj >= 1 && lj <= p.G;
              gxy = is_goal_lane ? static_cast<int>(reinterpret_cast<const uint16_t*>(h->goal)[lj - 1]) : -1;
              const int at_goal = __popcll(__ballot(is_goal_lane && xy == gxy) & gmask);
              first = at_goal == p.G ? 0 : -1;  // (vacuously a goal without goals, trap T8)
              plan = a.plans + static_cast<int64_t>(idx) * a.plan_cap;
              base = a.emit ? a.offset[idx] : 0;
              t = 0;
              if (len == 0) finish(first == 0 ? PW_REPLAY_VALID : PW_REPLAY_NOT_GOAL, first, true);  // puzzle.py:413-424 on no action
              else active = true;
            }
          }
        }
      }
    }
    if (__ballot(active) == 0ull) {
      if (__ballot(!exhausted) == 0ull) break;
      continue;
    }
    if (!active) {  // (a group between items plays nothing: no movable, no goal lane)
      p.N = 0;
      is_goal_lane = false;
      xy = 0;
      ot = 0u;
      small = 0ull;
    }

    // ---- one action of every active lane group ---------------------------------------------------------------------------
    // GS plan bytes per load: lane lj holds action t - (t mod GS) + lj
    if (active && (t & (GS - 1)) == 0) chunk = (t + lj < len) ? static_cast<int>(plan[t + lj]) : 0;
    const int act = __shfl(chunk, gbase + (t & (GS - 1)), PW_WAVE);
    const bool bad_act = active && act > 3;
    const bool play = active && !bad_act;
    const int am = act & 3;
    const int dx = am == 0 ? -1 : (am == 1 ? 1 : 0);
    const int dy = am == 2 ? -1 : (am == 3 ? 1 : 0);
    const LaneSlot s0 = lane_slot(xy, ot, small);
    const uint32_t moved = group_push_set<GS, false>(p, s0, none, lj, gbase, gmask, play, am, dx, dy);

    // displaced state + goal bookkeeping (puzzle.py:384-411), as step_group_body
    int nxy = xy;
    if (play && ((moved >> lj) & 1u)) {
      const int x = static_cast<int8_t>(xy & 0xff) + dx, y = static_cast<int8_t>((xy >> 8) & 0xff) + dy;
      nxy = (x & 0xff) | ((y & 0xff) << 8);
    }
    const int before = __popcll(__ballot(is_goal_lane && xy == gxy) & gmask);
    const int after = __popcll(__ballot(is_goal_lane && nxy == gxy) & gmask);
    if (play) {
      const bool terminated = after == p.G;
      if (a.emit) {
        const int64_t row = base + t;
        if (row < a.cap) {
          if (lj == 0) {
            if (a.row_item) a.row_item[row] = item;
            if (a.row_t) a.row_t[row] = t;
            if (a.row_puzzle_id) a.row_puzzle_id[row] = pid;
            if (a.row_action) a.row_action[row] = static_cast<uint8_t>(act);
            if (a.row_reward) a.row_reward[row] = terminated ? 10.0 : static_cast<double>(after - before) - 0.01;  // gym_env.py:212-221
            if (a.row_done) a.row_done[row] = terminated ? 1 : 0;
          }
          if (lj < a.npad) {
            if (a.row_pos) reinterpret_cast<int16_t*>(a.row_pos)[row * a.npad + lj] = static_cast<int16_t>(xy);
            if (a.row_next_pos) reinterpret_cast<int16_t*>(a.row_next_pos)[row * a.npad + lj] = static_cast<int16_t>(nxy);
          }
        } else if (lj == 0) {
          n_dropped++;
        }
      }
      xy = nxy;
      if (terminated && first < 0) first = t + 1;
      t++;
      if (t == len) {
        finish(first == len ? PW_REPLAY_VALID : (first < 0 ? PW_REPLAY_NOT_GOAL : PW_REPLAY_EARLY), first, true);
        active = false;
      }
    } else if (bad_act) {  // a byte outside 0..3: the item is not a plan (emit: never reached after a check of the same data)
      finish(PW_REPLAY_SKIPPED, -1, false);
      active = false;
    }
  }
  if (a.emit && a.dropped && n_dropped) atomicAdd(a.dropped, n_dropped);
}

// the engine-owned workspace: 64 work counters (64 bytes apart, one per launch in turn) + the scan's temporary storage
static const size_t kReplayCounterBytes = 64 * 64;

static int replay_workspace(PwEngine* e, size_t scan_bytes, const char* what) {
  const size_t want = kReplayCounterBytes + scan_bytes;
  if (e->d_replay && e->replay_bytes >= want) return PW_OK;
  uint8_t* fresh = nullptr;
  if (hipMalloc(reinterpret_cast<void**>(&fresh), want) != hipSuccess) {
    (void)hipGetLastError();
    return pw_fail(PW_ENOMEM, std::string(what) + ": cannot allocate the replay workspace");
  }
  if (e->d_replay) {  // (a launch in flight on any stream still uses the old one)
    (void)hipDeviceSynchronize();
    (void)hipFree(e->d_replay);
  }
  e->d_replay = fresh;
  e->replay_bytes = want;
  return PW_OK;
}

// the argument checks of both entry points; everything but the last two needs no engine
static int replay_check_args(const PwEngine* e, const int32_t* puzzle_id, int32_t npad, const uint8_t* plans,
                             const int32_t* plan_len, int32_t plan_cap, int32_t n, int32_t include, const int8_t* verdict,
                             const int64_t* offset, int64_t cap, const char* what) {
  const std::string w = std::string(what) + ": ";
  if (n < 1) return pw_fail(PW_EINVAL, w + "n must be >= 1");
  if (int rc = pw_check_npad(w, npad)) return rc;
  if (!puzzle_id) return pw_fail(PW_EINVAL, w + "null puzzle_id");
  if (!plans) return pw_fail(PW_EINVAL, w + "null plans");
  if (!plan_len) return pw_fail(PW_EINVAL, w + "null plan_len");
  if (!verdict) return pw_fail(PW_EINVAL, w + "null verdict");
  if (!offset) return pw_fail(PW_EINVAL, w + "null offset");
  if (plan_cap < 1 || plan_cap > PW_PLAN_MAX_ACTIONS) return pw_fail(PW_EINVAL, w + "plan_cap must be 1 .. PW_PLAN_MAX_ACTIONS");
  if (include != PW_REPLAY_INCLUDE_VALID && include != PW_REPLAY_INCLUDE_REPLAYED)
    return pw_fail(PW_EINVAL, w + "include must be PW_REPLAY_INCLUDE_VALID or PW_REPLAY_INCLUDE_REPLAYED");
  if (cap < 0) return pw_fail(PW_EINVAL, w + "cap must be >= 0");
  if (!e) return pw_fail(PW_EINVAL, w + "null engine");
  if (npad < e->set->max_n) return pw_fail(PW_EINVAL, w + "npad is smaller than the set's largest number of movables");
  return PW_OK;
}

static void replay_launch(PwEngine* e, ReplayArgs& a, hipStream_t st) {
  a.hdrs = e->set->d_headers;
  a.blob = e->set->d_blob;
  a.ovl = e->d_ovl;
  a.ovl_dir = e->d_ovl_dir;
  a.num_puzzles = e->set->count;
  a.next_item = reinterpret_cast<uint32_t*>(e->d_replay + 64 * (e->replay_seq++ & 63u));
  (void)hipMemsetAsync(a.next_item, 0, 4, st);
  const int tab = e->ovl_puzzles == 0 ? 0 : (e->ovl_puzzles == e->set->count ? 2 : 1);
  const int gs = a.npad <= 8 ? 8 : a.npad;
  // a wavefront per workgroup, 64 / GS items at a time; the chains are latency bound: up to 16 wavefronts per CU
  const int64_t waves = (static_cast<int64_t>(a.n) + (PW_WAVE / gs) - 1) / (PW_WAVE / gs);
  const dim3 grid(static_cast<unsigned>(std::min<int64_t>(waves, 16ll * std::max(e->num_cus, 1)))), block(PW_WAVE);
#define PW_LAUNCH_REPLAY(GS)                                                                          \
  do {                                                                                                \
    if (tab == 0) hipLaunchKernelGGL((pw_plan_replay_kernel<GS, 0>), grid, block, 0, st, a);          \
    else if (tab == 1) hipLaunchKernelGGL((pw_plan_replay_kernel<GS, 1>), grid, block, 0, st, a);     \
    else hipLaunchKernelGGL((pw_plan_replay_kernel<GS, 2>), grid, block, 0, st, a);                   \
  } while (0)
  if (gs == 8) PW_LAUNCH_REPLAY(8);
  else if (gs == 16) PW_LAUNCH_REPLAY(16);
  else PW_LAUNCH_REPLAY(32);
#undef PW_LAUNCH_REPLAY
}

extern "C" {

int pw_plan_replay_check(PwEngine* e, const int32_t* puzzle_id, const int8_t* pos, int32_t npad, const uint8_t* plans,
                         const int32_t* plan_len, int32_t plan_cap, const uint8_t* mask, int32_t n, int32_t include,
                         int8_t* verdict, int32_t* first_goal, int8_t* final_pos, int64_t* offset, void* stream) try {
  if (int rc = replay_check_args(e, puzzle_id, npad, plans, plan_len, plan_cap, n, include, verdict, offset, 0,
                                 "pw_plan_replay_check"))
    return rc;
  PwDeviceGuard guard(e->set->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  size_t scan_bytes = 0;
  const size_t count = static_cast<size_t>(n) + 1;
  hipError_t err = rocprim::exclusive_scan(nullptr, scan_bytes, offset, offset, static_cast<int64_t>(0), count,
                                           rocprim::plus<int64_t>(), st);
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string("pw_plan_replay_check: ") + hipGetErrorString(err));
  scan_bytes = pw_pad256(scan_bytes);
  if (int rc = replay_workspace(e, scan_bytes, "pw_plan_replay_check")) return rc;
  ReplayArgs a{};
  a.puzzle_id = puzzle_id;
  a.pos = pos;
  a.plans = plans;
  a.plan_len = plan_len;
  a.mask = mask;
  a.n = n;
  a.npad = npad;
  a.plan_cap = plan_cap;
  a.include = include;
  a.emit = 0;
  a.verdict = verdict;
  a.first_goal = first_goal;
  a.final_pos = final_pos;
  a.offset = offset;
  replay_launch(e, a, st);
  if (int rc = check_launch("pw_plan_replay_check")) return rc;
  size_t tmp = e->replay_bytes - kReplayCounterBytes;
  err = rocprim::exclusive_scan(e->d_replay + kReplayCounterBytes, tmp, offset, offset, static_cast<int64_t>(0), count,
                                rocprim::plus<int64_t>(), st);
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string("pw_plan_replay_check: ") + hipGetErrorString(err));
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_plan_replay_emit(PwEngine* e, const int32_t* puzzle_id, const int8_t* pos, int32_t npad, const uint8_t* plans,
                        const int32_t* plan_len, int32_t plan_cap, const uint8_t* mask, int32_t n, int32_t include,
                        const int8_t* verdict, const int64_t* offset, int64_t cap, int32_t* row_item, int32_t* row_t,
                        int32_t* row_puzzle_id, int8_t* row_pos, uint8_t* row_action, double* row_reward, uint8_t* row_done,
                        int8_t* row_next_pos, int64_t* dropped, void* stream) try {
  if (int rc = replay_check_args(e, puzzle_id, npad, plans, plan_len, plan_cap, n, include, verdict, offset, cap,
                                 "pw_plan_replay_emit"))
    return rc;
  PwDeviceGuard guard(e->set->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (int rc = replay_workspace(e, 0, "pw_plan_replay_emit")) return rc;
  if (dropped && hipMemsetAsync(dropped, 0, 8, st) != hipSuccess)
    return pw_fail(PW_EDEVICE, "pw_plan_replay_emit: hipMemsetAsync failed");
  ReplayArgs a{};
  a.puzzle_id = puzzle_id;
  a.pos = pos;
  a.plans = plans;
  a.plan_len = plan_len;
  a.mask = mask;
  a.n = n;
  a.npad = npad;
  a.plan_cap = plan_cap;
  a.include = include;
  a.emit = 1;
  a.verdict = const_cast<int8_t*>(verdict);
  a.offset = const_cast<int64_t*>(offset);
  a.cap = cap;
  a.row_item = row_item;
  a.row_t = row_t;
  a.row_puzzle_id = row_puzzle_id;
  a.row_pos = row_pos;
  a.row_action = row_action;
  a.row_reward = row_reward;
  a.row_done = row_done;
  a.row_next_pos = row_next_pos;
  a.dropped = reinterpret_cast<unsigned long long*>(dropped);
  replay_launch(e, a, st);
  return check_launch("pw_plan_replay_emit");
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

}  // extern "C"

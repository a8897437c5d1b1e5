// pw_step_kernels.inc -- reset, episode turnover, the step formulations, rollout (the resident step kernel: pw_mailbox_kernels.inc; planner expansion: pw_expand_kernels.inc).
// Part of the single translation unit pw_kernels.hip (included there; uses its helpers).

// ------------------------------------------------------------------------------------
// K0 reset  (gym_env.py:150-186)
// ------------------------------------------------------------------------------------
// Puzzle ids come from the caller and index the header array: clamped into the set (one v_min_u32), so that no kernel of the
// step / render path reads outside the engine's tables whatever it is given (positions are range-checked where they index:
// rows, table rows, bit positions).  A wrong id then plays the wrong puzzle -- pw_validate_state finds it -- but touches nothing
// it should not.
__device__ __forceinline__ int pw_clamp_pid(int pid, int num_puzzles) {
  return static_cast<int>(min(static_cast<unsigned>(pid), static_cast<unsigned>(num_puzzles - 1)));
}

struct ResetArgs {
  const PwPuzzleHeader* hdrs;
  const uint8_t* blob;
  const int32_t* puzzle_id;
  const uint8_t* mask;
  int8_t* pos;
  int32_t* steps;
  uint8_t* term;
  uint8_t* trunc;
  int32_t batch;
  int32_t np;
  int32_t num_puzzles;
};

__global__ __launch_bounds__(256) void pw_reset_kernel(ResetArgs a) {
  // one thread per (env, object slot): coalesced int16 stores of the position rows
  const int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  const int env = static_cast<int>(t / a.np);
  const int j = static_cast<int>(t - static_cast<int64_t>(env) * a.np);
  if (env >= a.batch) return;
  if (a.mask && !a.mask[env]) return;
  const PwPuzzleHeader& h = a.hdrs[pw_clamp_pid(a.puzzle_id[env], a.num_puzzles)];
  int16_t v = 0;
  if (j < h.N) v = reinterpret_cast<const int16_t*>(h.init)[j];
  reinterpret_cast<int16_t*>(a.pos)[static_cast<int64_t>(env) * a.np + j] = v;
  if (j == 0) {
    a.steps[env] = 0;
    if (a.term) a.term[env] = 0;
    if (a.trunc) a.trunc[env] = 0;
  }
}

// ------------------------------------------------------------------------------------
// pw_validate_state: the preconditions the step / render kernels rely on without checking -- puzzle ids inside
// the set, every movable inside its puzzle's grid (DESIGN.md section 2), zero padding beyond N.
// ------------------------------------------------------------------------------------
struct ValidateArgs {
  const PwPuzzleHeader* hdrs;
  const int32_t* puzzle_id;
  const int8_t* pos;  // may be NULL: ids only
  uint32_t* out;      // [0] number of bad environments, [1] lowest bad environment index
  int32_t batch;
  int32_t np;
  int32_t num_puzzles;
};

__global__ __launch_bounds__(256) void pw_validate_kernel(ValidateArgs a) {
  const int env = blockIdx.x * 256 + threadIdx.x;
  if (env >= a.batch) return;
  const int pid = a.puzzle_id[env];
  bool bad = pid < 0 || pid >= a.num_puzzles;
  if (!bad && a.pos) {
    const PwPuzzleHeader& h = a.hdrs[pid];
    const int8_t* row = a.pos + static_cast<int64_t>(env) * a.np * 2;
    for (int j = 0; j < a.np; j++) {
      const int x = row[2 * j], y = row[2 * j + 1];
      if (j < h.N) bad = bad || x < 0 || y < 0 || x + h.objtab[j].w > h.W || y + h.objtab[j].h > h.H;
      else bad = bad || x != 0 || y != 0;
    }
  }
  if (bad) {
    atomicAdd(&a.out[0], 1u);
    atomicMin(&a.out[1], static_cast<uint32_t>(env));
  }
}

// ------------------------------------------------------------------------------------
// K1 step  (gym_env.py:188-226 minus the observation)
// ------------------------------------------------------------------------------------
// ------------------------------------------------------------------------------------
// Episode management (SURVEY 8-f1): environments whose episode has ended draw the puzzle of their
// next episode on the device.  The reference draws with the host's Mersenne Twister
// (gym_env.py:172 random.choice); a batch has no sequential stream to share, so the draw is a
// counter-based hash of (seed, environment, episode number): reproducible, order independent.
// ------------------------------------------------------------------------------------
struct ResampleArgs {
  int32_t* puzzle_id;
  const uint8_t* term;
  const uint8_t* trunc;
  const int32_t* table;
  uint32_t* episode;
  uint64_t seed;
  int32_t table_len;
  int32_t batch;
};

// splitmix64 finaliser over the three counters (also restated in numpy by the tests)
__host__ __device__ __forceinline__ uint64_t mix64(uint64_t seed, uint64_t env, uint64_t episode) {
  uint64_t z = seed + 0x9E3779B97F4A7C15ull * (env + 1ull) + 0xD1B54A32D192ED03ull * episode;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__global__ __launch_bounds__(256) void pw_resample_kernel(ResampleArgs a) {
  const int env = blockIdx.x * 256 + threadIdx.x;
  if (env >= a.batch) return;
  const bool done = (!a.term && !a.trunc) || (a.term && a.term[env]) || (a.trunc && a.trunc[env]);
  if (!done) return;
  const uint32_t ep = a.episode[env] + 1u;
  a.episode[env] = ep;
  const uint64_t r = mix64(a.seed, static_cast<uint64_t>(env), ep);
  // floor(r * n / 2^64): unbiased to 2^-32 for n < 2^31
  const uint32_t idx = static_cast<uint32_t>(__umul64hi(r, static_cast<uint64_t>(a.table_len)));
  a.puzzle_id[env] = a.table ? a.table[idx] : static_cast<int32_t>(idx);
}

struct PwSegDir;
struct PwSegDesc;
struct StepArgs {
  const PwPuzzleHeader* hdrs;
  const uint8_t* blob;
  const int32_t* puzzle_id;
  const uint8_t* actions;
  int8_t* pos;
  int32_t* steps;
  double* reward;
  int8_t* dgoals;
  uint8_t* term;
  uint8_t* trunc;
  int32_t batch;
  int32_t max_steps;
  uint32_t flags;
  int32_t np;
  uint32_t* dirty;  // optional [batch]: cell rows the step changed, lo | hi << 8 | puzzle height << 16
                    // (lo = hi = 0: none); group kernel only
  uint32_t* bad_actions;  // engine-owned sticky counter of actions outside 0..3 (pw_engine_bad_actions)
  PageRec* rec;           // optional [batch]: page records of the NEW state for the page-ordered render; group kernel only
  const uint64_t* ovl;      // overlap tables (PwOvlDir), or NULL; lane-group kernels only
  const PwOvlDir* ovl_dir;  // [set size]
  int32_t reverse;          // lane-group kernels: pw_block_order -- bit 0: workgroup b takes the environments of workgroup gridDim - 1 - b
                            // (PW_OPT_STEP_BLOCK_ORDER: the expensive end of a batch sorted by puzzle starts first)
  int32_t num_puzzles;      // puzzle ids are clamped to 0 .. num_puzzles - 1 (pw_clamp_pid)
  const uint64_t* boards;   // [set size][2] whole-grid wall / wall + agent-wall boards of sets whose puzzles all fit 8 x 8
                            // (pw_step_board_kernel), or NULL
  unsigned long long* counters;  // engine-owned throughput counters (pw_counters): PW_COUNTER_SLOTS slots of 8 uint64 (a 64-byte
                                 // line each): [0] env-steps, [1] episodes ended, [2] episodes solved
  const uint8_t* qdesc;          // [set size] PwQuadDesc records (step_quad16_body), or NULL (PW_OPT_STEP_QUAD16 never / no tables)
  // a BOUND batch (pw_batch_bind, pw_seg_kernels.inc); all NULL / 0 otherwise
  const PwSegDesc* segs;         // segment descriptors: one workgroup of the segment role each
  const int32_t* bind_meta;      // [0] = number of segments
  const int32_t* perm;           // environment indices of the segments whose environments are not consecutive
  const int32_t* mlist;          // (environment, puzzle) pairs of pw_step_mseg_kernel: bind_meta[5] of them
  const uint8_t* bound;          // [batch]: 1 = the environment belongs to a segment (the lane-group role skips it)
  const PwSegDir* seg_dir;       // [set size]
  uint32_t* bind_mismatch;       // engine-owned: environments whose puzzle id no longer is the one they were bound to
  int32_t seg_grid;              // workgroups of the segment role at the front of a fused launch (>= the number of segments)
  int32_t mseg_spread;           // pw_step_mseg_kernel / the lane role of pw_step_segm_kernel: 64 >> this environments per wavefront
  // PW_OPT_OBS_CHANGED_PAGES (looked at only where `rec` is written; both NULL otherwise): the positions the retained observation
  // buffer shows, laid out like pos, and per environment the grid rows in which the new state differs from them (pw_shown_rows)
  int8_t* shown;
  uint64_t* changed;
};

// Grid rows whose pixels may differ between a movable of height h at the packed position `was` (x | y << 8, int8 each) and the
// same movable at `now`: its rows before and after; every row when a position lies outside the 64 rows a mask can name (any
// position is accepted from a caller, include/pushworld_amd.h pw_validate_state).  Zero when the two are equal.
__device__ __forceinline__ uint64_t pw_shown_rows(uint32_t was, uint32_t now, int h) {
  if (((was ^ now) & 0xffffu) == 0u) return 0ull;
  const int y0 = static_cast<int8_t>((was >> 8) & 0xffu), y1 = static_cast<int8_t>((now >> 8) & 0xffu);
  if (static_cast<unsigned>(y0) >= 64u || static_cast<unsigned>(y1) >= 64u) return ~0ull;
  const uint64_t m = h >= 64 ? ~0ull : ((1ull << h) - 1ull);
  return (m << y0) | (m << y1);
}

// The record writers' part of PW_OPT_OBS_CHANGED_PAGES for a lane that owns a whole environment and has stored its new state:
// `pos` / `shown` = the environment's rows of np int8 pairs, `height(j)` = height of movable j in cells (j < n <= np).  Leaves
// the rows that differ from what the retained buffer shows in *changed and, when there are any, the new positions in `shown`.
// Everything is loaded here, after the step: nothing of it is live across the step.  (The slots beyond n are never compared.)
template <typename Height>
__device__ __forceinline__ void pw_shown_update(const int8_t* pos, int8_t* shown, uint64_t* changed, int n, Height height) {
  const uint32_t* prow = reinterpret_cast<const uint32_t*>(pos);
  uint32_t* srow = reinterpret_cast<uint32_t*>(shown);
  uint64_t m = 0;
  for (int k = 0; 2 * k < n; k++) {
    const uint32_t s = srow[k], p = prow[k];
    if (s != p) {
      m |= pw_shown_rows(s, p, height(2 * k));
      if (2 * k + 1 < n) m |= pw_shown_rows(s >> 16, p >> 16, height(2 * k + 1));
    }
  }
  *changed = m;
  if (m)
    for (int k = 0; 2 * k < n; k++) srow[k] = prow[k];
}

// Throughput counters (pw_counters): every wavefront adds what its environments did to ONE of 64 slots (64 bytes apart, so
// the atomics of a launch spread over 64 L2 lines instead of queueing on one address); env-steps always, the other two
// only when non-zero (a few percent of the wavefronts).  No return value is used: the atomics are fire and forget.
#define PW_COUNTER_SLOTS 64
__device__ __forceinline__ void pw_count_add(unsigned long long* counters, uint32_t steps, uint32_t ended, uint32_t solved) {
  // (wave-uniform arguments; one lane of the wavefront adds)
  const unsigned long long active = __ballot(true);
  if (static_cast<int>(threadIdx.x & (PW_WAVE - 1)) != __ffsll(active) - 1) return;
  unsigned long long* slot = counters + ((blockIdx.x * 4u + (threadIdx.x >> 6)) & (PW_COUNTER_SLOTS - 1)) * 8u;
  if (steps) atomicAdd(slot, static_cast<unsigned long long>(steps));
  if (ended) atomicAdd(slot + 1, static_cast<unsigned long long>(ended));
  if (solved) atomicAdd(slot + 2, static_cast<unsigned long long>(solved));
}
// One step of the calling lanes' environments: `stepped` lanes each stand for one (environment, step), with the flags the
// step returned (0 / 1; 0xFF = refused action, counted as a step only).
__device__ __forceinline__ void pw_count_step(unsigned long long* counters, bool stepped, int term, int trunc) {
  const bool fin = stepped && term != 0xFF;
  const uint32_t n = static_cast<uint32_t>(__popcll(__ballot(stepped)));
  const uint32_t e = static_cast<uint32_t>(__popcll(__ballot(fin && (term | trunc) != 0)));
  const uint32_t v = static_cast<uint32_t>(__popcll(__ballot(fin && term != 0)));
  pw_count_add(counters, n, e, v);
}

// One wavefront advances one environment (all lanes of the wave must call this).
//   xy_out     lane j = packed (x | y << 8) of object j after the call
//   legal_out  true when the resulting state is known to be overlap-free (legal play keeps it
//              so: pushed objects move rigidly into free cells); false = unknown
__device__ __forceinline__ void step_one_env(const StepArgs& a, int env, int lane, const PuzzleView& pv, int& xy_out,
                                             bool& legal_out) {
  const int NP = a.np;
  // first-level loads, all independent
  const int act = __builtin_amdgcn_readfirstlane(static_cast<int>(a.actions[env]));
  const int was_done = __builtin_amdgcn_readfirstlane(static_cast<int>(a.term[env] | a.trunc[env]));
  const int steps_in = __builtin_amdgcn_readfirstlane(a.steps[env]);
  int16_t* prow = reinterpret_cast<int16_t*>(a.pos) + static_cast<int64_t>(env) * NP;
  int xy = 0;  // coalesced load of the packed (x, y) int8 pairs: lane j holds object j
  if (lane < NP) xy = static_cast<uint16_t>(prow[lane]);
  legal_out = false;

  if ((a.flags & PW_STEP_AUTORESET) && was_done) {
    // next-step autoreset: this call is the reset() of a finished episode
    xy = (lane < pv.N) ? static_cast<int>(reinterpret_cast<const uint16_t*>(pv.h->init)[lane]) : 0;
    if (lane < NP) prow[lane] = static_cast<int16_t>(xy);
    if (lane == 0) {
      a.steps[env] = 0;
      a.term[env] = 0;
      a.trunc[env] = 0;
      if (a.reward) a.reward[env] = 0.0;
      if (a.dgoals) a.dgoals[env] = 0;
    }
    xy_out = xy;
    pw_count_add(a.counters, 1u, 0u, 0u);
    return;
  }
  if (act > 3) {  // not in Discrete(4): flag and leave the env untouched (gym_env.py:195-196)
    if (lane == 0) {
      a.term[env] = 0xFF;
      a.trunc[env] = 0xFF;
      atomicAdd(a.bad_actions, 1u);
    }
    xy_out = xy;
    pw_count_add(a.counters, 1u, 0u, 0u);
    return;
  }

  const EnvBoards b = load_boards(pv, xy, lane);
  const uint32_t pushed = push_closure(pv, b, xy, act, lane);

  // displaced state (puzzle.py:384-394) + goal bookkeeping (puzzle.py:396-411)
  const int dx = act == 0 ? -1 : (act == 1 ? 1 : 0);
  const int dy = act == 2 ? -1 : (act == 3 ? 1 : 0);
  int x = static_cast<int8_t>(xy & 0xff), y = static_cast<int8_t>((xy >> 8) & 0xff);
  const bool is_goal_lane = lane >= 1 && lane <= pv.G;
  int gxy = 0;
  if (is_goal_lane) gxy = reinterpret_cast<const uint16_t*>(pv.h->goal)[lane - 1];
  const int before = __popcll(__ballot(is_goal_lane && (xy & 0xffff) == gxy));
  if ((pushed >> lane) & 1u) {
    x += dx;
    y += dy;
  }
  const int nxy = (x & 0xff) | ((y & 0xff) << 8);
  const int after = __popcll(__ballot(is_goal_lane && nxy == gxy));
  if (pushed && lane < pv.N) prow[lane] = static_cast<int16_t>(nxy);

  const bool terminated = after == pv.G;  // vacuously true without goals (trap T8)
  const bool truncated = a.max_steps >= 0 && steps_in + 1 >= a.max_steps;
  if (lane == 0) {
    a.steps[env] = steps_in + 1;
    a.term[env] = terminated ? 1 : 0;
    a.trunc[env] = truncated ? 1 : 0;
    // gym_env.py:212-221: python float arithmetic == IEEE double here
    if (a.reward) a.reward[env] = terminated ? 10.0 : static_cast<double>(after - before) - 0.01;
    if (a.dgoals) a.dgoals[env] = static_cast<int8_t>(after - before);
  }
  pw_count_add(a.counters, 1u, (terminated || truncated) ? 1u : 0u, terminated ? 1u : 0u);
  xy_out = lane < pv.N ? nxy : 0;
  legal_out = b.legal;
}

__global__ __launch_bounds__(256) void pw_step_kernel(StepArgs a) {
  const int lane = threadIdx.x & (PW_WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
  const int env = blockIdx.x * (256 / PW_WAVE) + wave;
  if (env >= a.batch) return;
  const int pid = __builtin_amdgcn_readfirstlane(pw_clamp_pid(a.puzzle_id[env], a.num_puzzles));
  const PuzzleView pv = view_of(a.hdrs, a.blob, pid);
  int xy;
  bool legal;
  step_one_env(a, env, lane, pv, xy, legal);
}

// ------------------------------------------------------------------------------------
// K1s single state, latency path (pw_next_state / pw_plan_states: PushWorldPuzzle.get_next_state, is_valid_plan,
// render_plan of puzzle.py:348-394, :413-424, :471-506).  ONE wavefront; the start state arrives in the kernel
// arguments, every state it reaches is written straight into pinned host memory mapped into the device (and, on request, into
// a device buffer in the pos layout for one batched render of the plan); the last store is the completion word the calling
// host thread polls -- a system-scope release, so every earlier store of the wavefront has landed.
// ------------------------------------------------------------------------------------
struct PlanArgs {
  const PwPuzzleHeader* hdrs;
  const uint8_t* blob;
  int32_t puzzle;
  int32_t num_actions;
  int32_t action;           // the action when there is exactly one and no action array (pw_next_state)
  uint8_t* out;             // host memory as the device sees it: [0] completion word, [16] int32 info[4], then the sections below
  uint32_t off_actions;     // uint8 [num_actions] (read 64 at a time: one PCIe round trip per 64 steps)
  uint32_t off_states;      // int8 [num_actions + 1][N][2]
  uint32_t off_goals;       // uint8 [num_actions + 1]
  uint16_t* dev_states;     // optional device buffer [num_actions + 1][np] of packed (x, y)
  int32_t np;
  uint32_t seq;
  uint16_t xy[32];          // the start state, x | y << 8
};

__global__ __launch_bounds__(64) void pw_plan_kernel(PlanArgs a) {
  const int lane = threadIdx.x;
  const PuzzleView pv = view_of(a.hdrs, a.blob, a.puzzle);
  const int N = pv.N;
  int xy = lane < 32 ? static_cast<int>(a.xy[lane & 31]) : 0;
  if (lane >= N) xy = 0;
  uint16_t* states = reinterpret_cast<uint16_t*>(a.out + a.off_states);
  uint8_t* goals = a.out + a.off_goals;
  const bool is_goal_lane = lane >= 1 && lane <= pv.G;
  const int gxy = is_goal_lane ? static_cast<int>(reinterpret_cast<const uint16_t*>(pv.h->goal)[lane - 1]) : -1;
  int at_goal = __popcll(__ballot(is_goal_lane && xy == gxy));
  if (lane < N) states[lane] = static_cast<uint16_t>(xy);
  if (a.dev_states && lane < a.np) a.dev_states[lane] = static_cast<uint16_t>(xy);
  if (lane == 0) goals[0] = at_goal == pv.G ? 1 : 0;
  int chunk = 0;
  uint32_t pushed = 0;
  int before = at_goal;
  for (int t = 0; t < a.num_actions; t++) {
    if (a.action < 0 && (t & 63) == 0) chunk = (t + lane < a.num_actions) ? static_cast<int>(a.out[a.off_actions + t + lane]) : 0;
    const int act = a.action >= 0 ? a.action : __builtin_amdgcn_readlane(chunk, t & 63);
    const EnvBoards b = load_boards(pv, xy, lane);
    pushed = push_closure(pv, b, xy, act & 3, lane);
    if ((pushed >> lane) & 1u) {
      const int dx = act == 0 ? -1 : (act == 1 ? 1 : 0), dy = act == 2 ? -1 : (act == 3 ? 1 : 0);
      const int x = static_cast<int8_t>(xy & 0xff) + dx, y = static_cast<int8_t>((xy >> 8) & 0xff) + dy;
      xy = (x & 0xff) | ((y & 0xff) << 8);
    }
    before = at_goal;
    at_goal = __popcll(__ballot(is_goal_lane && xy == gxy));
    const int64_t o = static_cast<int64_t>(t) + 1;
    if (lane < N) states[o * N + lane] = static_cast<uint16_t>(xy);
    if (a.dev_states && lane < a.np) a.dev_states[o * a.np + lane] = static_cast<uint16_t>(xy);
    if (lane == 0) goals[o] = at_goal == pv.G ? 1 : 0;
  }
  if (lane < 4) {
    const int v = lane == 0 ? static_cast<int>(pushed) : (lane == 1 ? before : (lane == 2 ? at_goal : (at_goal == pv.G ? 1 : 0)));
    reinterpret_cast<int32_t*>(a.out + 16)[lane] = v;
  }
  // every store above has been issued by this wavefront; the release makes them visible to the host before the word
  if (lane == 0) __hip_atomic_store(reinterpret_cast<uint32_t*>(a.out), a.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ------------------------------------------------------------------------------------
// K1b step, one LANE per environment (state-only batches: configs C2 / C4)
//
// Same predicate as the wavefront kernel, evaluated by a single lane on the few rows where two
// bounding boxes can meet: object rows are fetched from the packed shape rows (L1 hits, the
// lanes of a wave mostly share a puzzle) instead of being spread over a wave.  64x less
// ALU work and coalesced per-env outputs.  These row helpers are what the lane-group kernels further down
// (pw_step / pw_rollout default, pw_expand4, pw_search) are built from; only the fused step+render launch
// keeps the wavefront formulation.
// ------------------------------------------------------------------------------------
// RowPtr: where the row bitboards live -- global memory (read through L1, the default) or LDS (address space 3,
// the staged variant, profiles/r02_step_ab.txt)
// kTabMode: what the code that uses the view is compiled for -- 0: no overlap tables anywhere (no table code),
// 1: some puzzles have tables (pair / wtab are NULL for the others: both paths), 2: every puzzle the kernel meets has
// tables (no row loops at all: the instance the engine launches for sets that carry tables for all their puzzles).
template <typename RowPtr, int kTabMode = 0>
struct LanePuzzleT {
  static constexpr int kTables = kTabMode;
  const PwPuzzleHeader* h;
  RowPtr wall;
  RowPtr awall;
  RowPtr shapes;
  int H, N, G;
  // overlap tables of the puzzle (PwOvlDir; always global memory), NULL without
  const uint64_t* pair;
  const uint64_t* wtab;
  int R, Hs;
};

// the puzzle's overlap tables, if the engine built any (one 16-byte load, independent of the header's)
template <typename P>
__device__ __forceinline__ void lane_tables(P& p, const uint64_t* ovl, const PwOvlDir* dir, int pid) {
  p.pair = nullptr;
  p.wtab = nullptr;
  p.R = 0;
  p.Hs = 0;
  if constexpr (P::kTables != 0) {
    const uint4 d = *reinterpret_cast<const uint4*>(dir + pid);
    if (P::kTables == 2 || d.x) {
      p.pair = ovl + d.x;
      p.wtab = ovl + d.y;
      p.R = static_cast<int>(d.z & 0xffffu);
      p.Hs = static_cast<int>(d.z >> 16);
    }
  }
}
typedef LanePuzzleT<const uint64_t*> LanePuzzle;
typedef const uint64_t __attribute__((address_space(3)))* PwLdsRows;

struct LaneObj {
  int x, y, w, h, off;
};

// ot = packed PwObjEntry (w | h << 8 | row_off << 16)
__device__ __forceinline__ LaneObj lane_obj(uint32_t ot, int xy) {
  LaneObj o;
  o.x = static_cast<int8_t>(xy & 0xff);
  o.y = static_cast<int8_t>((xy >> 8) & 0xff);
  o.w = static_cast<int>(ot & 0xffu);
  o.h = static_cast<int>((ot >> 8) & 0xffu);
  o.off = static_cast<int>(ot >> 16);
  return o;
}

// The agent's wall test with every load issued up front (one memory latency instead of one per
// row): window of 8 grid rows around the agent; taller agents use the generic loop.
template <typename P>
__device__ __forceinline__ bool lane_agent_blocked(const P& p, const LaneObj& o, int act);

// row yy of the board that holds only object o (same conventions as object_row())
template <typename P>
__device__ __forceinline__ uint64_t lane_row(const P& p, const LaneObj& o, int yy) {
  const int rr = yy - o.y;
  uint64_t r = 0;
  if (static_cast<unsigned>(rr) < static_cast<unsigned>(o.h) && static_cast<unsigned>(yy) < 64u) r = p.shapes[o.off + rr];
  return (static_cast<unsigned>(o.x) < 64u) ? (r << o.x) : 0ull;
}

// row yy of the board of object o displaced by the action (cf. shift_rows())
template <typename P>
__device__ __forceinline__ uint64_t lane_row_shifted(const P& p, const LaneObj& o, int yy, int act) {
  // ONE load whatever the action (the lane groups of a wavefront play different actions: a branch per action costs a
  // memory latency per branch); UP: the new row yy holds the old row yy + 1, DOWN: yy - 1; rows outside 0..63 are
  // empty in lane_row
  const uint64_t r = lane_row(p, o, act == 2 ? yy + 1 : (act == 3 ? yy - 1 : yy));
  return act == 0 ? r >> 1 : (act == 1 ? r << 1 : r);
}

// the object lies entirely inside its grid: only there can a wall stop it (the bounds clause, puzzle.py:557-561 -- the
// reference's wall tables hold in-bounds positions only).  The row tests below place an object's rows at its grid column,
// which they can do for an object inside the grid alone.
template <typename P>
__device__ __forceinline__ bool lane_inside(const P& p, const LaneObj& o) {
  return o.x >= 0 && o.y >= 0 && o.x + o.w <= static_cast<int>(p.h->W) && o.y + o.h <= static_cast<int>(p.h->H);
}

// row yy of object o in the frame whose column 0 is grid column x0, wherever on or around the grid the object lies
// (cells left of x0 or 64 and more columns right of it vanish)
template <typename P>
__device__ __forceinline__ uint64_t lane_row_rel(const P& p, const LaneObj& o, int yy, int x0) {
  const int rr = yy - o.y, sh = o.x - x0;
  uint64_t r = 0;
  if (static_cast<unsigned>(rr) < static_cast<unsigned>(o.h)) r = p.shapes[o.off + rr];
  return sh >= 0 ? (sh < 64 ? r << sh : 0ull) : (sh > -64 ? r >> -sh : 0ull);
}

// moving o collides with the static rows and o does not overlap them now (puzzle.py:522-564)
template <typename P, typename Rows>
__device__ __forceinline__ bool lane_blocked(const P& p, const LaneObj& o, Rows rows, int act) {
  if (!lane_inside(p, o)) return false;
  uint64_t hit = 0, now = 0;
  const int dyy = act == 2 ? -1 : (act == 3 ? 1 : 0);  // rows of the object now and after the move
  for (int yy = o.y + min(dyy, 0); yy < o.y + o.h + max(dyy, 0); yy++) {
    if (static_cast<unsigned>(yy) >= static_cast<unsigned>(p.H)) continue;
    const uint64_t g = rows[yy];
    hit |= lane_row_shifted(p, o, yy, act) & g;
    now |= lane_row(p, o, yy) & g;
  }
  return hit != 0 && now == 0;
}

// moving a pushes b: they overlap after the move and do not overlap now (puzzle.py:567-593)
template <typename P>
__device__ __forceinline__ bool lane_pushes(const P& p, const LaneObj& a, const LaneObj& b, int act, int dx, int dy) {
  // bounding boxes of the displaced pusher and of the pushee must meet
  if (a.x + dx >= b.x + b.w || b.x >= a.x + dx + a.w || a.y + dy >= b.y + b.h || b.y >= a.y + dy + a.h) return false;
  uint64_t hit = 0, now = 0;
  // only the rows that hold cells of b AND of the pusher (where it is or where it goes): a one-row agent against a
  // 27-row object is two iterations, not 27
  // (in b's frame, so that the verdict does not depend on where the pair lies: a movable one cell beyond the grid, at
  // x = -1 or y = -1, pushes and is pushed like any other)
  const int y0 = max(b.y, a.y + min(dy, 0)), y1 = min(b.y + b.h, a.y + a.h + max(dy, 0));
  for (int yy = y0; yy < y1; yy++) {
    const uint64_t rb = p.shapes[b.off + yy - b.y];
    hit |= lane_row_rel(p, a, yy - dy, b.x - dx) & rb;
    now |= lane_row_rel(p, a, yy, b.x) & rb;
  }
  return hit != 0 && now == 0;
}

// ---- movables that fit into 8 x 8 cells (all but a few dozen objects of the benchmark): their shape is ONE
// uint64 (PwPuzzleHeader::off_small, bit 8 * row + column), the push test between two of them is two shifts and
// two ANDs without a load or a loop, their wall test reads only the wall rows.  Same verdicts as lane_pushes /
// lane_blocked (tests/test_gpu_parity.py runs every shipped puzzle through both).
// the board with every cell moved by (ox, oy); cells that leave the 8 x 8 window vanish
__device__ __forceinline__ uint64_t small_moved(uint64_t s, int ox, int oy) {
  if (static_cast<unsigned>(ox + 7) > 14u || static_cast<unsigned>(oy + 7) > 14u) return 0ull;
  const int sh = 8 * oy + ox;
  const uint64_t r = sh >= 0 ? s << sh : s >> -sh;
  uint32_t m = ox >= 0 ? (0xffu << ox) & 0xffu : 0xffu >> -ox;  // columns that did not wrap into a neighbouring row
  m |= m << 8;
  m |= m << 16;
  return r & ((static_cast<uint64_t>(m) << 32) | m);
}

// row r of a small board placed at column x of the grid (0 outside the board)
__device__ __forceinline__ uint64_t small_row(uint64_t s, int r, int x) {
  const uint64_t b = (static_cast<unsigned>(r) < 8u) ? (s >> (8 * r)) & 0xffull : 0ull;
  return (static_cast<unsigned>(x) < 64u) ? b << x : 0ull;
}

// lane_pushes for two small objects with boards sa (pusher) and sb
__device__ __forceinline__ bool small_pushes(uint64_t sa, const LaneObj& a, uint64_t sb, const LaneObj& b, int dx, int dy) {
  if (a.x + dx >= b.x + b.w || b.x >= a.x + dx + a.w || a.y + dy >= b.y + b.h || b.y >= a.y + dy + a.h) return false;
  const int ox = b.x - a.x, oy = b.y - a.y;  // b in the pusher's frame
  return (sa & small_moved(sb, ox - dx, oy - dy)) != 0ull && (sa & small_moved(sb, ox, oy)) == 0ull;
}

// lane_blocked for a small object with board s
template <typename P, typename Rows>
__device__ __forceinline__ bool small_blocked(const P& p, uint64_t s, const LaneObj& o, Rows rows, int dx, int dy) {
  if (!lane_inside(p, o)) return false;
  uint64_t hit = 0, now = 0;
  for (int rr = 0; rr < o.h; rr++) {
    const int yy = o.y + rr, yh = yy + dy;
    const uint64_t m = (static_cast<unsigned>(o.x) < 64u) ? ((s >> (8 * rr)) & 0xffull) << o.x : 0ull;
    const uint64_t wn = (static_cast<unsigned>(yy) < static_cast<unsigned>(p.H)) ? rows[yy] : 0ull;
    const uint64_t wh = (dy != 0 && static_cast<unsigned>(yh) < static_cast<unsigned>(p.H)) ? rows[yh] : 0ull;
    now |= wn & m;
    hit |= dy != 0 ? (wh & m) : (wn & (dx < 0 ? m >> 1 : m << 1));
  }
  return hit != 0ull && now == 0ull;
}

// ---- the same two verdicts from the puzzle's overlap tables (PwOvlDir): no loop, one or two 8-byte loads
// movable i (geometry a) pushes movable j (geometry b)
template <typename P>
__device__ __forceinline__ bool table_pushes(const P& p, int i, const LaneObj& a, int j, const LaneObj& b, int dx, int dy) {
  if (a.x + dx >= b.x + b.w || b.x >= a.x + dx + a.w || a.y + dy >= b.y + b.h || b.y >= a.y + dy + a.h) return false;
  const uint64_t* t = p.pair + static_cast<size_t>(i * p.N + j) * static_cast<size_t>(p.R);
  const int row = a.y - b.y + a.h - 1, bit = a.x - b.x + a.w - 1;  // the pair's rows beyond h_i + h_j - 1 are zero
  const int rh = row + dy, bh = bit + dx;
  // (the bounding boxes meet after the move, so rh / bh are inside the table)
  const uint64_t th = (static_cast<unsigned>(rh) < static_cast<unsigned>(p.R)) ? t[rh] : 0ull;
  const uint64_t tn = dy == 0 ? th : ((static_cast<unsigned>(row) < static_cast<unsigned>(p.R)) ? t[row] : 0ull);
  const bool hit = static_cast<unsigned>(bh) < 64u && ((th >> bh) & 1ull) != 0ull;
  const bool now = static_cast<unsigned>(bit) < 64u && ((tn >> bit) & 1ull) != 0ull;
  return hit && !now;
}

// table_pushes without a branch around the loads (clamped rows, verdict masked afterwards): in the lane-per-environment
// kernels the tests of one pusher against all other movables are independent of each other, and a load inside a divergent
// branch would wait for its result before the next test starts.  j may be >= N (verdict false).
template <typename P>
__device__ __forceinline__ bool table_pushes_flat(const P& p, int i, const LaneObj& a, int j, const LaneObj& b, int dx, int dy) {
  const bool meet = j < p.N && !(a.x + dx >= b.x + b.w || b.x >= a.x + dx + a.w || a.y + dy >= b.y + b.h || b.y >= a.y + dy + a.h);
  const uint64_t* t = p.pair + static_cast<size_t>(i * p.N + min(j, p.N - 1)) * static_cast<size_t>(p.R);
  const int row = a.y - b.y + a.h - 1, bit = a.x - b.x + a.w - 1;
  const int rh = row + dy, bh = bit + dx;
  const uint64_t th = t[min(max(rh, 0), p.R - 1)];
  const uint64_t tn = t[min(max(row, 0), p.R - 1)];
  const bool hit = static_cast<unsigned>(rh) < static_cast<unsigned>(p.R) && static_cast<unsigned>(bh) < 64u && ((th >> (bh & 63)) & 1ull) != 0ull;
  const bool now = static_cast<unsigned>(row) < static_cast<unsigned>(p.R) && static_cast<unsigned>(bit) < 64u && ((tn >> (bit & 63)) & 1ull) != 0ull;
  return meet && hit && !now;
}

// movable j (geometry o) is stopped by a wall (the agent: wall or agent wall)
template <typename P>
__device__ __forceinline__ bool table_blocked(const P& p, int j, const LaneObj& o, int dx, int dy) {
  const uint64_t* t = p.wtab + static_cast<size_t>(j) * static_cast<size_t>(p.Hs);
  const int row = o.y + 1, bit = o.x + 1, rh = row + dy, bh = bit + dx;
  const uint64_t th = (static_cast<unsigned>(rh) < static_cast<unsigned>(p.Hs)) ? t[rh] : 0ull;
  const uint64_t tn = dy == 0 ? th : ((static_cast<unsigned>(row) < static_cast<unsigned>(p.Hs)) ? t[row] : 0ull);
  const bool hit = static_cast<unsigned>(bh) < 64u && ((th >> bh) & 1ull) != 0ull;
  const bool now = static_cast<unsigned>(bit) < 64u && ((tn >> bit) & 1ull) != 0ull;
  return hit && !now;
}

template <typename P>
__device__ __forceinline__ bool lane_agent_blocked(const P& p, const LaneObj& o, int act) {
  if (o.h > 6) return lane_blocked(p, o, p.awall, act);
  if (!lane_inside(p, o)) return false;
  uint64_t g[8], sh[8];
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const int yy = o.y - 1 + k;
    g[k] = (static_cast<unsigned>(yy) < static_cast<unsigned>(p.H)) ? p.awall[yy] : 0ull;
    // sh[k] = board row yy of the agent (k = 0 and k = 7 are outside for h <= 6)
    const int rr = k - 1;
    uint64_t r = 0;
    if (static_cast<unsigned>(rr) < static_cast<unsigned>(o.h) && static_cast<unsigned>(yy) < 64u) r = p.shapes[o.off + rr];
    sh[k] = (static_cast<unsigned>(o.x) < 64u) ? (r << o.x) : 0ull;
  }
  uint64_t hit = 0, now = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const int yy = o.y - 1 + k;
    uint64_t moved;
    if (act == 0) moved = sh[k] >> 1;
    else if (act == 1) moved = sh[k] << 1;
    else if (act == 2) moved = (k < 7 && yy != 63) ? sh[k + 1] : 0ull;
    else moved = (k > 0 && yy != 0) ? sh[k - 1] : 0ull;
    hit |= moved & g[k];
    now |= sh[k] & g[k];
  }
  return hit != 0 && now == 0;
}

template <int NP>
__device__ __forceinline__ int lane_pos(const uint32_t (&P)[NP / 2], int j) {
  uint32_t v = 0;
#pragma unroll
  for (int k = 0; k < NP / 2; k++) v = (k == (j >> 1)) ? P[k] : v;
  return static_cast<int>((v >> (16 * (j & 1))) & 0xffffu);
}

// Per-lane environment state kept in registers between the steps of a rollout.
template <int NP>
struct LaneEnv {
  uint32_t P[NP / 2];  // packed (x, y) int8 pairs, two objects per dword
  int steps;
  int term, trunc;     // flags of the last step (0 / 1 / 0xFF)
  double reward;
  int dgoals;
};

template <int NP>
__device__ __forceinline__ void lane_load(const StepArgs& a, int env, LaneEnv<NP>& s) {
  const uint32_t* prow = reinterpret_cast<const uint32_t*>(a.pos) + static_cast<int64_t>(env) * (NP / 2);
  if (NP == 4) {
    const uint2 v = *reinterpret_cast<const uint2*>(prow);
    s.P[0] = v.x;
    s.P[1] = v.y;
  } else {
#pragma unroll
    for (int k = 0; k < NP / 8; k++) {
      const uint4 v = reinterpret_cast<const uint4*>(prow)[k];
      s.P[4 * k + 0] = v.x;
      s.P[4 * k + 1] = v.y;
      s.P[4 * k + 2] = v.z;
      s.P[4 * k + 3] = v.w;
    }
  }
  s.steps = a.steps[env];
  s.term = a.term[env];
  s.trunc = a.trunc[env];
  s.reward = 0.0;
  s.dgoals = 0;
}

template <int NP>
__device__ __forceinline__ void lane_store_pos(const StepArgs& a, int env, const LaneEnv<NP>& s) {
  uint32_t* prow = reinterpret_cast<uint32_t*>(a.pos) + static_cast<int64_t>(env) * (NP / 2);
  if (NP == 4) {
    *reinterpret_cast<uint2*>(prow) = make_uint2(s.P[0], s.P[1]);
  } else {
#pragma unroll
    for (int k = 0; k < NP / 8; k++)
      reinterpret_cast<uint4*>(prow)[k] = make_uint4(s.P[4 * k], s.P[4 * k + 1], s.P[4 * k + 2], s.P[4 * k + 3]);
  }
}

// One pw_step of one environment on one lane (gym_env.py:188-226 minus the observation).
// Returns true when the positions changed.
// P::kTables == 2: every verdict from the puzzle's overlap tables (no loop, one or two 8-byte loads each); otherwise the
// row loops (the independent formulation the parity tests compare the table kernels with).
template <int NP, typename P>
__device__ __forceinline__ bool lane_step(const P& p, const PwPuzzleHeader* h, const uint32_t (&OT)[NP],
                                          LaneEnv<NP>& s, int act, uint32_t flags, int max_steps) {
  constexpr bool kT = P::kTables == 2;
  if ((flags & PW_STEP_AUTORESET) && (s.term | s.trunc)) {
    // next-step autoreset: this step is the reset() of a finished episode
#pragma unroll
    for (int k = 0; k < NP / 2; k++) s.P[k] = reinterpret_cast<const uint32_t*>(h->init)[k];
    s.steps = 0;
    s.term = 0;
    s.trunc = 0;
    s.reward = 0.0;
    s.dgoals = 0;
    return true;
  }
  if (act > 3) {  // not in Discrete(4): flag and leave the env untouched (gym_env.py:195-196)
    s.term = 0xFF;
    s.trunc = 0xFF;
    return false;
  }
  const int dx = act == 0 ? -1 : (act == 1 ? 1 : 0);
  const int dy = act == 2 ? -1 : (act == 3 ? 1 : 0);

  uint32_t pushed = 0;
  const LaneObj agent = lane_obj(OT[0], static_cast<int>(s.P[0] & 0xffffu));
  if constexpr (kT) {
    // Table form, in phases whose loads do not depend on each other: every push test of a pusher first, then the wall
    // tests of what it pushes.  The push set is a fixed point of the CURRENT positions, so "some member is stopped by a
    // wall" does not depend on the order of discovery (puzzle.py:361-382 aborts at the first one it meets).
    if (!table_blocked(p, 0, agent, dx, dy)) {
      uint32_t hits = 0;
#pragma unroll
      for (int j = 1; j < NP; j++) {
        if (__ballot(j < p.N) == 0ull) break;  // (wave-uniform: sets padded to NP hold many smaller puzzles)
        const LaneObj oj = lane_obj(OT[j], static_cast<int>((s.P[j >> 1] >> (16 * (j & 1))) & 0xffffu));
        if (table_pushes_flat(p, 0, agent, j, oj, dx, dy)) hits |= 1u << j;
      }
      bool blocked = false;
      pushed = 1u | hits;
      uint32_t frontier = hits;
      while (frontier && !blocked) {  // (one round per step in all but ~0.1 % of them)
        uint32_t next = 0;
        for (uint32_t f = frontier; f; f &= f - 1) {
          const int i = __ffs(f) - 1;
          const LaneObj oi = lane_obj(reinterpret_cast<const uint32_t*>(h->objtab)[i], lane_pos<NP>(s.P, i));
          blocked = blocked || table_blocked(p, i, oi, dx, dy);
          for (int j = 1; j < p.N; j++) {
            if (((pushed | next) >> j) & 1u) continue;
            const LaneObj oj = lane_obj(reinterpret_cast<const uint32_t*>(h->objtab)[j], lane_pos<NP>(s.P, j));
            if (table_pushes(p, i, oi, j, oj, dx, dy)) next |= 1u << j;
          }
        }
        pushed |= next;
        frontier = next;
      }
      if (blocked) pushed = 0;
    }
  } else if (!lane_agent_blocked(p, agent, act)) {  // puzzle.py:353
    pushed = 1u;
    uint32_t frontier = 0;
    bool blocked = false;
    // sweep of the agent over all other movables (positions in registers, static indices)
#pragma unroll
    for (int j = 1; j < NP; j++) {
      if (j < p.N && !blocked) {
        const LaneObj oj = lane_obj(OT[j], static_cast<int>((s.P[j >> 1] >> (16 * (j & 1))) & 0xffffu));
        if (lane_pushes(p, agent, oj, act, dx, dy)) {
          if (lane_blocked(p, oj, p.wall, act)) {
            blocked = true;  // transitive stopping
          } else {
            pushed |= 1u << j;
            frontier |= 1u << j;
          }
        }
      }
    }
    // pushed objects push further objects (about 0.1 % of steps)
    while (frontier && !blocked) {
      const int i = __ffs(frontier) - 1;
      frontier &= frontier - 1;
      const LaneObj oi = lane_obj(reinterpret_cast<const uint32_t*>(h->objtab)[i], lane_pos<NP>(s.P, i));
      for (int j = 1; j < p.N && !blocked; j++) {
        if ((pushed >> j) & 1u) continue;
        const LaneObj oj = lane_obj(reinterpret_cast<const uint32_t*>(h->objtab)[j], lane_pos<NP>(s.P, j));
        if (lane_pushes(p, oi, oj, act, dx, dy)) {
          if (lane_blocked(p, oj, p.wall, act)) {
            blocked = true;
          } else {
            pushed |= 1u << j;
            frontier |= 1u << j;
          }
        }
      }
    }
    if (blocked) pushed = 0;
  }

  // displaced state + goal bookkeeping (puzzle.py:384-411)
  int before = 0, after = 0;
#pragma unroll
  for (int j = 0; j < NP; j++) {
    const uint32_t sh = 16 * (j & 1);
    const uint32_t cur = (s.P[j >> 1] >> sh) & 0xffffu;
    uint32_t nxt = cur;
    if ((pushed >> j) & 1u) {
      const int x = static_cast<int8_t>(cur & 0xff) + dx, y = static_cast<int8_t>((cur >> 8) & 0xff) + dy;
      nxt = static_cast<uint32_t>(x & 0xff) | (static_cast<uint32_t>(y & 0xff) << 8);
      s.P[j >> 1] = (s.P[j >> 1] & ~(0xffffu << sh)) | (nxt << sh);
    }
    if (j >= 1 && j <= p.G) {
      const uint32_t g = reinterpret_cast<const uint16_t*>(h->goal)[j - 1];
      before += cur == g;
      after += nxt == g;
    }
  }
  const bool terminated = after == p.G;  // vacuously true without goals (trap T8)
  s.steps += 1;
  s.term = terminated ? 1 : 0;
  s.trunc = (max_steps >= 0 && s.steps >= max_steps) ? 1 : 0;
  // gym_env.py:212-221: python float arithmetic == IEEE double here
  s.reward = terminated ? 10.0 : static_cast<double>(after - before) - 0.01;
  s.dgoals = after - before;
  return pushed != 0;
}

template <int NP, typename P>
__device__ __forceinline__ void lane_puzzle(const StepArgs& a, int pid, P& p, uint32_t (&OT)[NP]) {
  const PwPuzzleHeader* h = a.hdrs + pid;
  p.h = h;
  const uint8_t* b = a.blob + h->base;
  p.wall = reinterpret_cast<const uint64_t*>(b + h->off_wall);
  p.awall = reinterpret_cast<const uint64_t*>(b + h->off_awall);
  p.shapes = reinterpret_cast<const uint64_t*>(b + h->off_shapes);
  p.H = h->H;
  p.N = h->N;
  p.G = h->G;
  lane_tables(p, a.ovl, a.ovl_dir, pid);  // (nothing without P::kTables)
  // the whole object table (bounding boxes + shape-row offsets) with wide loads
#pragma unroll
  for (int k = 0; k < NP / 4; k++) {
    const uint4 v = reinterpret_cast<const uint4*>(h->objtab)[k];
    OT[4 * k + 0] = v.x;
    OT[4 * k + 1] = v.y;
    OT[4 * k + 2] = v.z;
    OT[4 * k + 3] = v.w;
  }
}

// kTab: 0 row loops, 2 overlap tables only (the engine has tables for every puzzle of the set)
template <int NP, int kTab = 0>
__global__ __launch_bounds__(256) void pw_step_lane_kernel(StepArgs a) {
  const int env = blockIdx.x * 256 + threadIdx.x;
  if (env >= a.batch) return;
  const int act = a.actions[env];
  LaneEnv<NP> s;
  lane_load<NP>(a, env, s);
  LanePuzzleT<const uint64_t*, kTab> p;
  uint32_t OT[NP];
  lane_puzzle<NP>(a, pw_clamp_pid(a.puzzle_id[env], a.num_puzzles), p, OT);
  const int t0 = s.term, u0 = s.trunc;
  const bool changed = lane_step<NP>(p, p.h, OT, s, act, a.flags, a.max_steps);
  pw_count_step(a.counters, true, s.term, s.trunc);
  if (changed) lane_store_pos<NP>(a, env, s);
  if (act > 3 && !((a.flags & PW_STEP_AUTORESET) && (t0 | u0))) {
    a.term[env] = 0xFF;
    a.trunc[env] = 0xFF;
    atomicAdd(a.bad_actions, 1u);
    return;
  }
  a.steps[env] = s.steps;
  a.term[env] = static_cast<uint8_t>(s.term);
  a.trunc[env] = static_cast<uint8_t>(s.trunc);
  if (a.reward) a.reward[env] = s.reward;
  if (a.dgoals) a.dgoals[env] = static_cast<int8_t>(s.dgoals);
}

// K1c rollout: T consecutive steps of every environment in ONE launch.  The environment lives in
// registers between steps; puzzle tables are L1 hits after the first step.
struct RolloutArgs {
  StepArgs s;              // actions = uint8 [T][B]
  int32_t num_steps;
  double* reward_hist;     // optional [T][B]
  uint8_t* term_hist;      // optional [T][B]
  uint8_t* trunc_hist;     // optional [T][B]
};

template <int NP, int kTab = 0>
__global__ __launch_bounds__(256) void pw_rollout_lane_kernel(RolloutArgs r) {
  const StepArgs& a = r.s;
  const int env = blockIdx.x * 256 + threadIdx.x;
  if (env >= a.batch) return;
  LaneEnv<NP> s;
  lane_load<NP>(a, env, s);
  LanePuzzleT<const uint64_t*, kTab> p;
  uint32_t OT[NP];
  lane_puzzle<NP>(a, pw_clamp_pid(a.puzzle_id[env], a.num_puzzles), p, OT);
  bool changed = false;
  uint32_t n_ended = 0, n_solved = 0;  // wave-uniform: summed over the wavefront's environments step by step
  for (int t = 0; t < r.num_steps; t++) {
    const int64_t o = static_cast<int64_t>(t) * a.batch + env;
    // (no prefetch of the next steps' actions as in the lane-group kernel: this kernel runs where the batch fills the chip
    // with wavefronts that hide the load, and the extra registers cost more -- C3 x 4: 533 vs 649 us per 64 steps)
    const int act = a.actions[o];
    if (act > 3 && !((a.flags & PW_STEP_AUTORESET) && (s.term | s.trunc))) atomicAdd(a.bad_actions, 1u);
    changed = lane_step<NP>(p, p.h, OT, s, act, a.flags, a.max_steps) || changed;
    n_ended += static_cast<uint32_t>(__popcll(__ballot(s.term != 0xFF && (s.term | s.trunc) != 0)));
    n_solved += static_cast<uint32_t>(__popcll(__ballot(s.term != 0xFF && s.term != 0)));
    if (r.reward_hist) r.reward_hist[o] = s.reward;
    if (r.term_hist) r.term_hist[o] = static_cast<uint8_t>(s.term);
    if (r.trunc_hist) r.trunc_hist[o] = static_cast<uint8_t>(s.trunc);
  }
  pw_count_add(a.counters, static_cast<uint32_t>(__popcll(__ballot(true))) * static_cast<uint32_t>(r.num_steps), n_ended, n_solved);
  if (changed) lane_store_pos<NP>(a, env, s);
  a.steps[env] = s.steps;
  a.term[env] = static_cast<uint8_t>(s.term);
  a.trunc[env] = static_cast<uint8_t>(s.trunc);
  if (a.reward) a.reward[env] = s.reward;
  if (a.dgoals) a.dgoals[env] = static_cast<int8_t>(s.dgoals);
}

// K1d: sets whose puzzles ALL fit into 8 x 8 cells (grid incl. its border walls; the Level-0 families of 5 x 5 puzzles: C2) and
// have at most 8 movables.  The whole grid is one uint64 (bit 8 y + x), a movable at its position is its 8 x 8 shape board
// shifted there: "i pushes j", "j is stopped by a wall" are two ANDs on registers each -- no table, no load after the
// puzzle's three or four boards, no ballot.  One LANE per environment; the environment lives in registers between the steps
// of a rollout.  Same verdicts as the other formulations (puzzle.py:348-394; cells shifted out of the 8 x 8 window are
// outside the grid, where there is neither wall nor movable).
// an 8 x 8 shape board placed at (x, y) of the grid window (cells outside the window vanish); small_moved() without branches
__device__ __forceinline__ uint64_t board_place(uint64_t s, int x, int y) {
  const bool in = static_cast<unsigned>(x + 7) <= 14u && static_cast<unsigned>(y + 7) <= 14u;
  const int sh = 8 * y + x;
  const uint64_t up = s << (sh & 63), down = s >> ((-sh) & 63);
  const uint32_t m8 = x >= 0 ? (0xffu << (x & 7)) & 0xffu : 0xffu >> ((-x) & 7);  // columns that did not wrap into a neighbouring row
  const uint32_t m32 = m8 * 0x01010101u;
  const uint64_t r = (sh >= 0 ? up : down) & ((static_cast<uint64_t>(m32) << 32) | m32);
  return in ? r : 0ull;
}

template <int NP>
__device__ __forceinline__ bool board_step(const PwPuzzleHeader* h, int N, int G, uint64_t wb, uint64_t awb, const uint64_t (&S)[NP],
                                           const uint32_t (&GL)[NP], uint64_t (&B)[NP], uint32_t& stale, uint32_t& partial,
                                           LaneEnv<NP>& s, int act, uint32_t flags, int max_steps) {
  if ((flags & PW_STEP_AUTORESET) && (s.term | s.trunc)) {  // next-step autoreset: this step is the reset() of a finished episode
#pragma unroll
    for (int k = 0; k < NP / 2; k++) s.P[k] = reinterpret_cast<const uint32_t*>(h->init)[k];
    stale = ~0u;
    s.steps = 0;
    s.term = 0;
    s.trunc = 0;
    s.reward = 0.0;
    s.dgoals = 0;
    return true;
  }
  if (act > 3) {  // not in Discrete(4): flag and leave the env untouched (gym_env.py:195-196)
    s.term = 0xFF;
    s.trunc = 0xFF;
    return false;
  }
  const int dx = act == 0 ? -1 : (act == 1 ? 1 : 0);
  const int dy = act == 2 ? -1 : (act == 3 ? 1 : 0);
  // Branch-free where it can be: with one wavefront per SIMD (C2: 64 wavefronts on the chip) nothing hides the bubble of a
  // taken branch, and small_moved() has two per board.
  // The boards live in registers from step to step: a moved one is its old board shifted by one cell (B is replaced by M
  // below).  Only after a (re)start, or when a movable is not entirely inside the 8 x 8 window before or after a move -- it
  // left the grid, from a state that overlapped a border wall --, its board is placed from its position again (`partial`:
  // boards that lost cells at their placement; `leaves` below: boards about to lose some).
  if (stale) {
#pragma unroll
    for (int j = 0; j < NP; j++) {
      const uint32_t xy = (s.P[j >> 1] >> (16 * (j & 1))) & 0xffffu;
      if ((stale >> j) & 1u) {  // (S[j] = 0 beyond N: empty boards push nothing and are never pushed)
        B[j] = board_place(S[j], static_cast<int8_t>(xy & 0xff), static_cast<int8_t>((xy >> 8) & 0xff));
        partial = (partial & ~(1u << j)) | ((__popcll(B[j]) != __popcll(S[j]) ? 1u : 0u) << j);
      }
    }
    stale = 0;
  }
  const int up = act == 1 ? 1 : (act == 3 ? 8 : 0), down = act == 0 ? 1 : (act == 2 ? 8 : 0);
  const uint64_t keep = act == 0 ? ~0x8080808080808080ull : (act == 1 ? ~0x0101010101010101ull : ~0ull);  // no wrap into the next row
  const uint64_t edge = act == 0 ? 0x0101010101010101ull
                                 : (act == 1 ? 0x8080808080808080ull : (act == 2 ? 0x00000000000000ffull : 0xff00000000000000ull));
  uint64_t M[NP];         // every movable where the action would take it
  uint32_t stopped = 0;   // bit j: movable j would move into a wall it does not overlap now (the agent: wall or agent wall)
  uint32_t leaves = 0;    // bit j: the move would take cells of j out of the window
#pragma unroll
  for (int j = 0; j < NP; j++) M[j] = ((B[j] << up) >> down) & keep;
  if (partial) {  // (never in play that started inside the grid) cells may ENTER the window: place the moved boards
#pragma unroll
    for (int j = 0; j < NP; j++) {
      const uint32_t xy = (s.P[j >> 1] >> (16 * (j & 1))) & 0xffffu;
      if ((partial >> j) & 1u)
        M[j] = board_place(S[j], static_cast<int8_t>(xy & 0xff) + dx, static_cast<int8_t>((xy >> 8) & 0xff) + dy);
    }
  }
#pragma unroll
  for (int j = 0; j < NP; j++) {
    const uint64_t w = j == 0 ? awb : wb;
    stopped |= (((M[j] & w) != 0ull && (B[j] & w) == 0ull) ? 1u : 0u) << j;
    leaves |= ((B[j] & edge) != 0ull ? 1u : 0u) << j;
  }
  uint32_t pushed = 0;
  if (!(stopped & 1u)) {  // the agent is free to move (puzzle.py:353)
    pushed = 1u;
    uint32_t frontier = 1u;
    bool blocked = false;
    while (frontier && !blocked) {
      const int i = __ffs(frontier) - 1;
      frontier &= frontier - 1;
      uint64_t bi = 0, mi = 0;
#pragma unroll
      for (int k = 0; k < NP; k++) {
        bi = k == i ? B[k] : bi;
        mi = k == i ? M[k] : mi;
      }
      uint32_t fresh = 0;  // what i pushes: overlap after its move and none now (puzzle.py:567-593)
#pragma unroll
      for (int j = 1; j < NP; j++) fresh |= (((mi & B[j]) != 0ull && (bi & B[j]) == 0ull) ? 1u : 0u) << j;
      fresh &= ~pushed;
      blocked = (fresh & stopped) != 0u;  // ... one of them into a wall: nothing moves (:522-564)
      pushed |= fresh;
      frontier |= fresh;
    }
    if (blocked) pushed = 0;
  }
  stale = pushed & (leaves | partial);
  // displaced state + goal bookkeeping (puzzle.py:384-411), as lane_step
  int before = 0, after = 0;
#pragma unroll
  for (int j = 0; j < NP; j++) {
    const uint32_t sh = 16 * (j & 1);
    const uint32_t cur = (s.P[j >> 1] >> sh) & 0xffffu;
    uint32_t nxt = cur;
    if ((pushed >> j) & 1u) {
      const int x = static_cast<int8_t>(cur & 0xff) + dx, y = static_cast<int8_t>((cur >> 8) & 0xff) + dy;
      nxt = static_cast<uint32_t>(x & 0xff) | (static_cast<uint32_t>(y & 0xff) << 8);
      s.P[j >> 1] = (s.P[j >> 1] & ~(0xffffu << sh)) | (nxt << sh);
      B[j] = M[j];
    }
    if (j >= 1 && j <= G) {
      before += cur == GL[j];
      after += nxt == GL[j];
    }
  }
  const bool terminated = after == G;  // vacuously true without goals (trap T8)
  s.steps += 1;
  s.term = terminated ? 1 : 0;
  s.trunc = (max_steps >= 0 && s.steps >= max_steps) ? 1 : 0;
  s.reward = terminated ? 10.0 : static_cast<double>(after - before) - 0.01;  // gym_env.py:212-221
  s.dgoals = after - before;
  return pushed != 0;
}

template <int NP>
__global__ __launch_bounds__(256) void pw_step_board_kernel(RolloutArgs r) {
  const StepArgs& a = r.s;
  const int env = blockIdx.x * 256 + threadIdx.x;
  if (env >= a.batch) return;
  LaneEnv<NP> s;
  lane_load<NP>(a, env, s);
  const int pid = pw_clamp_pid(a.puzzle_id[env], a.num_puzzles);
  const PwPuzzleHeader* h = a.hdrs + pid;
  const int N = h->N, G = h->G;
  const uint64_t wb = a.boards[2 * pid], awb = a.boards[2 * pid + 1];
  uint64_t S[NP];
  const uint64_t* smalls = reinterpret_cast<const uint64_t*>(a.blob + h->base + h->off_small);
  uint32_t GL[NP];  // goal of movable j (j = 1 .. G), in registers for every step of the launch
#pragma unroll
  for (int j = 0; j < NP; j++) {
    S[j] = j < N ? smalls[j] : 0ull;
    GL[j] = (j >= 1 && j <= G) ? reinterpret_cast<const uint16_t*>(h->goal)[j - 1] : 0xffffffffu;
  }
  uint64_t B[NP];         // the movables on the grid, kept from step to step (board_step)
  uint32_t stale = ~0u;   // boards to be placed from the positions
  uint32_t partial = 0;   // boards that are not their whole shape (a movable partly outside the window)
#pragma unroll
  for (int j = 0; j < NP; j++) B[j] = 0ull;
  bool changed = false, any_played = false;
  uint32_t n_ended = 0, n_solved = 0;  // wave-uniform sums (pw_counters)
  // Actions sixteen steps at a time: a step is a few hundred register instructions, its action a new cache line of the [T][B]
  // array -- an HBM latency several times that (C2, 64 wavefronts on the whole chip: 1.5 us per step when every step waits for
  // its own).  Sixteen independent loads pay ONE latency; they wait in LDS (a rotating register window does not work: moving
  // a register that a load is still to fill waits for the load).
  __shared__ uint8_t s_act[16][256];
  for (int t = 0; t < r.num_steps; t++) {
    const int64_t o = static_cast<int64_t>(t) * a.batch + env;
    if ((t & 15) == 0) {
      int tmp[16];
#pragma unroll
      for (int k = 0; k < 16; k++) tmp[k] = t + k < r.num_steps ? static_cast<int>(a.actions[o + static_cast<int64_t>(k) * a.batch]) : 0;
#pragma unroll
      for (int k = 0; k < 16; k++) s_act[k][threadIdx.x] = static_cast<uint8_t>(tmp[k]);
    }
    const int act = s_act[t & 15][threadIdx.x];
    const bool resets = (a.flags & PW_STEP_AUTORESET) && (s.term | s.trunc);
    if (act > 3 && !resets) atomicAdd(a.bad_actions, 1u);
    else any_played = true;
    changed = board_step<NP>(h, N, G, wb, awb, S, GL, B, stale, partial, s, act, a.flags, a.max_steps) || changed;
    n_ended += static_cast<uint32_t>(__popcll(__ballot(s.term != 0xFF && (s.term | s.trunc) != 0)));
    n_solved += static_cast<uint32_t>(__popcll(__ballot(s.term != 0xFF && s.term != 0)));
    if (r.reward_hist) r.reward_hist[o] = s.reward;
    if (r.term_hist) r.term_hist[o] = static_cast<uint8_t>(s.term);
    if (r.trunc_hist) r.trunc_hist[o] = static_cast<uint8_t>(s.trunc);
  }
  pw_count_add(a.counters, static_cast<uint32_t>(__popcll(__ballot(true))) * static_cast<uint32_t>(r.num_steps), n_ended, n_solved);
  if (changed) lane_store_pos<NP>(a, env, s);
  a.term[env] = static_cast<uint8_t>(s.term);
  a.trunc[env] = static_cast<uint8_t>(s.trunc);
  if (any_played) {  // (a launch of nothing but bad actions leaves the counters alone, as the lane-group kernel)
    a.steps[env] = s.steps;
    if (a.reward) a.reward[env] = s.reward;
    if (a.dgoals) a.dgoals[env] = static_cast<int8_t>(s.dgoals);
  }
}

// The agent's wall test spread over the lanes of its group: lane k tests grid row y - 1 + k of the window
// the agent can reach (h + 2 rows), the verdict is two ballots.  ~6x fewer VALU cycles than one lane walking
// the window (the step kernel is VALU bound, profiles/r01_sq2.txt).  Wave-uniform fallback for agents taller
// than the group.
template <int GS, typename P>
__device__ __forceinline__ bool group_agent_blocked(const P& p, int xy, uint32_t ot, uint64_t small, int lj, int gbase,
                                                    unsigned long long gmask, bool play, int act) {
  const LaneObj ag = lane_obj(static_cast<uint32_t>(__shfl(static_cast<int>(ot), gbase, PW_WAVE)), __shfl(xy, gbase, PW_WAVE));
  const uint64_t asmall = __shfl(static_cast<unsigned long long>(small), gbase, PW_WAVE);
  if constexpr (P::kTables != 0) {
    if (P::kTables == 2 || p.wtab != nullptr) {  // (group-uniform) overlap tables: every lane of the group reads the verdict
      const int dxx = act == 0 ? -1 : (act == 1 ? 1 : 0), dyy = act == 2 ? -1 : (act == 3 ? 1 : 0);
      return play && table_blocked(p, 0, ag, dxx, dyy);
    }
  }
  if (__ballot(play && (asmall == 0ull || ag.h + 2 > GS)) == 0ull) {
    // every agent of the wavefront fits into 8 x 8 (all but 4 of the benchmark's): its rows come out of its board,
    // the only load is the lane's agent-wall row
    const int yy = ag.y - 1 + lj, dyy = act == 2 ? -1 : (act == 3 ? 1 : 0);
    bool hit = false, now = false;
    if (play && lj < ag.h + 2 && static_cast<unsigned>(yy) < static_cast<unsigned>(p.H)) {
      const uint64_t g = p.awall[yy];
      const uint64_t src = small_row(asmall, yy - dyy - ag.y, ag.x);
      now = (small_row(asmall, yy - ag.y, ag.x) & g) != 0ull;
      hit = ((act == 0 ? src >> 1 : (act == 1 ? src << 1 : src)) & g) != 0ull;
    }
    const unsigned long long hm = __ballot(hit) & gmask, nm = __ballot(now) & gmask;
    return hm != 0ull && nm == 0ull && lane_inside(p, ag);
  }
  if (__ballot(ag.h + 2 > GS) != 0ull) {
    // (the plain row loop, not lane_agent_blocked's unrolled 8-row window: inlined here that window costs every
    // lane-group kernel ~25 VGPRs for a path no shipped puzzle takes)
    bool blk = false;
    if (play && lj == 0) blk = lane_blocked(p, ag, p.awall, act);
    return (__ballot(blk) & gmask) != 0ull;
  }
  const int yy = ag.y - 1 + lj;
  bool hit = false, now = false;
  if (play && lj < ag.h + 2 && static_cast<unsigned>(yy) < static_cast<unsigned>(p.H)) {
    const uint64_t g = p.awall[yy];
    now = (lane_row(p, ag, yy) & g) != 0ull;
    hit = (lane_row_shifted(p, ag, yy, act) & g) != 0ull;
  }
  const unsigned long long hm = __ballot(hit) & gmask, nm = __ballot(now) & gmask;
  return hm != 0ull && nm == 0ull && lane_inside(p, ag);
}

// The push set of one action for the environment / state held by a lane group (lane j = movable j):
// agent wall test, then the fixed point "some member pushes my object" by ballots; any wall-blocked member
// kills the move (transitive stopping, puzzle.py:376-379).  Returns the mask of the objects that move
// (bit 0 = agent), 0 when nothing moves.  Shared by the step, planner-expansion and search kernels.
// One movable of a lane: position, packed PwObjEntry, its 8 x 8 board (PwPuzzleHeader::off_small; 0: the object does
// not fit, or there is no object in this slot) and the decoded geometry.
struct LaneSlot {
  int xy;
  uint32_t ot;
  uint64_t small;
  LaneObj me;
};

__device__ __forceinline__ LaneSlot lane_slot(int xy, uint32_t ot, uint64_t small) {
  LaneSlot s;
  s.xy = xy;
  s.ot = ot;
  s.small = small;
  s.me = lane_obj(ot, xy);
  return s;
}

// does `pusher` push the slot's object, and is that object then stopped by a wall
// (pi = index of the pusher, si = index of the slot's object: the keys of the puzzle's overlap tables, if it has any)
template <typename P>
__device__ __forceinline__ void slot_test(const P& p, const LaneObj& pusher, int pi, uint64_t psmall, const LaneSlot& s, int si,
                                          int act, int dx, int dy, bool& hit, bool& blk) {
  if constexpr (P::kTables == 2) {  // every puzzle has tables: no row loop is compiled in
    if (s.small != 0ull && psmall != 0ull) hit = small_pushes(psmall, pusher, s.small, s.me, dx, dy);
    else hit = table_pushes(p, pi, pusher, si, s.me, dx, dy);
    if (hit) blk = table_blocked(p, si, s.me, dx, dy);
  } else if constexpr (P::kTables == 1) {
    if (s.small != 0ull && psmall != 0ull) hit = small_pushes(psmall, pusher, s.small, s.me, dx, dy);
    else if (p.pair != nullptr) hit = table_pushes(p, pi, pusher, si, s.me, dx, dy);
    else hit = lane_pushes(p, pusher, s.me, act, dx, dy);
    if (hit) {
      if (p.wtab != nullptr) blk = table_blocked(p, si, s.me, dx, dy);
      else blk = s.small != 0ull ? small_blocked(p, s.small, s.me, p.wall, dx, dy) : lane_blocked(p, s.me, p.wall, act);
    }
  } else {
    if (s.small != 0ull && psmall != 0ull) hit = small_pushes(psmall, pusher, s.small, s.me, dx, dy);
    else hit = lane_pushes(p, pusher, s.me, act, dx, dy);
    if (hit) blk = s.small != 0ull ? small_blocked(p, s.small, s.me, p.wall, dx, dy) : lane_blocked(p, s.me, p.wall, act);
  }
}

// kTwo: every lane holds TWO movables, j = lane (slot s0) and j = GS + lane (slot s1), so that a 16-lane group
// carries the 17..32 movables of the largest puzzles and a mixed pool whose N_pad is 32 still runs 4 environments
// per wavefront; the second slot costs nothing where N <= GS (its branch is skipped for the whole wavefront).
// The fixed point from a given (pushed, frontier): the group's next pusher is the lowest member of `frontier`.
template <int GS, bool kTwo = false, typename P>
__device__ __forceinline__ uint32_t group_push_closure_from(const P& p, const LaneSlot& s0, const LaneSlot& s1, int lj, int gbase,
                                                            unsigned long long gmask, bool play, bool dead, uint32_t pushed,
                                                            uint32_t frontier, int act, int dx, int dy) {
  int cur = 0;
  bool active = play && !dead && frontier != 0u;
  if (active) {
    cur = __ffs(frontier) - 1;
    frontier &= frontier - 1u;
  }
  while (__ballot(active) != 0ull) {  // every lane tests the group's current pusher against its own object(s)
    const int src = gbase + (cur & (GS - 1));
    int pxy = __shfl(s0.xy, src, PW_WAVE);
    uint32_t pot = static_cast<uint32_t>(__shfl(static_cast<int>(s0.ot), src, PW_WAVE));
    uint64_t psmall = __shfl(static_cast<unsigned long long>(s0.small), src, PW_WAVE);
    if (kTwo && __ballot(active && cur >= GS) != 0ull) {  // some group's pusher is one of the movables GS .. 2 GS - 1
      const int pxy1 = __shfl(s1.xy, src, PW_WAVE);
      const uint32_t pot1 = static_cast<uint32_t>(__shfl(static_cast<int>(s1.ot), src, PW_WAVE));
      const uint64_t psmall1 = __shfl(static_cast<unsigned long long>(s1.small), src, PW_WAVE);
      if (cur >= GS) {
        pxy = pxy1;
        pot = pot1;
        psmall = psmall1;
      }
    }
    const LaneObj pusher = lane_obj(pot, pxy);
    bool hit0 = false, blk0 = false, hit1 = false, blk1 = false;
    if (active && lj >= 1 && lj < p.N && !((pushed >> lj) & 1u)) slot_test(p, pusher, cur, psmall, s0, lj, act, dx, dy, hit0, blk0);
    if (kTwo && active && lj + GS < p.N && !((pushed >> (lj + GS)) & 1u))
      slot_test(p, pusher, cur, psmall, s1, lj + GS, act, dx, dy, hit1, blk1);
    const unsigned long long hm = __ballot(hit0), bk = __ballot(blk0 || blk1);
    uint32_t fresh = static_cast<uint32_t>((hm & gmask) >> gbase);
    if (kTwo) fresh |= static_cast<uint32_t>((__ballot(hit1) & gmask) >> gbase) << GS;
    if ((bk & gmask) != 0ull) dead = true;
    pushed |= fresh;
    frontier |= fresh;
    active = active && !dead && frontier != 0u;
    if (active) {
      cur = __ffs(frontier) - 1;
      frontier &= frontier - 1u;
    }
  }
  return (play && !dead) ? pushed : 0u;
}

template <int GS, bool kTwo = false, typename P>
__device__ __forceinline__ uint32_t group_push_closure(const P& p, const LaneSlot& s0, const LaneSlot& s1, int lj, int gbase,
                                                       unsigned long long gmask, bool play, bool dead, int act, int dx,
                                                       int dy) {
  return group_push_closure_from<GS, kTwo>(p, s0, s1, lj, gbase, gmask, play, dead, 1u, 1u, act, dx, dy);  // the agent pushes first
}

// ---- planner expansion: the agent's sweep for all four actions of one state at once.  The four closures of a state all
// start with the agent as the pusher; what it does not depend on the action -- the broadcast of the agent, the offset of
// every movable to it, whether they overlap now -- is computed once, and an action's first closure iteration is one bit
// test per lane.  Bit a of the result: the agent, moved by action a, pushes the slot's movable (same verdicts as
// slot_test with the agent as the pusher).
template <typename P>
__device__ __forceinline__ uint32_t agent_pushes4(const P& p, const LaneObj& ag, uint64_t asmall, const LaneSlot& s, int si,
                                                  bool valid) {
  if (!valid) return 0u;
  // no action brings the agent's bounding box onto the movable's
  if (ag.x - 1 >= s.me.x + s.me.w || s.me.x >= ag.x + ag.w + 1 || ag.y - 1 >= s.me.y + s.me.h || s.me.y >= ag.y + ag.h + 1) return 0u;
  uint32_t m = 0u;
  if (asmall != 0ull && s.small != 0ull) {
    const int ox = s.me.x - ag.x, oy = s.me.y - ag.y;  // the movable in the agent's frame
    if ((asmall & small_moved(s.small, ox, oy)) != 0ull) return 0u;  // overlapping now: never pushed (puzzle.py:592)
    if ((asmall & small_moved(s.small, ox + 1, oy)) != 0ull) m |= 1u;  // LEFT: the agent at x - 1
    if ((asmall & small_moved(s.small, ox - 1, oy)) != 0ull) m |= 2u;
    if ((asmall & small_moved(s.small, ox, oy + 1)) != 0ull) m |= 4u;  // UP
    if ((asmall & small_moved(s.small, ox, oy - 1)) != 0ull) m |= 8u;
    return m;
  }
  if constexpr (P::kTables == 2) {
    const uint64_t* t = p.pair + static_cast<size_t>(si) * static_cast<size_t>(p.R);  // pair (0, si): i * N + j with i = 0
    const int row = ag.y - s.me.y + ag.h - 1, bit = ag.x - s.me.x + ag.w - 1;
    uint64_t r[3];
#pragma unroll
    for (int k = 0; k < 3; k++) r[k] = (static_cast<unsigned>(row - 1 + k) < static_cast<unsigned>(p.R)) ? t[row - 1 + k] : 0ull;
    auto at = [](uint64_t w, int b) { return static_cast<unsigned>(b) < 64u && ((w >> b) & 1ull) != 0ull; };
    if (at(r[1], bit)) return 0u;
    if (at(r[1], bit - 1)) m |= 1u;
    if (at(r[1], bit + 1)) m |= 2u;
    if (at(r[0], bit)) m |= 4u;
    if (at(r[2], bit)) m |= 8u;
    return m;
  } else {
    for (int act = 0; act < 4; act++) {
      const int dx = act == 0 ? -1 : (act == 1 ? 1 : 0), dy = act == 2 ? -1 : (act == 3 ? 1 : 0);
      if (lane_pushes(p, ag, s.me, act, dx, dy)) m |= 1u << act;
    }
    return m;
  }
}

// is the slot's movable, pushed by action (dx, dy), stopped by a wall
template <typename P>
__device__ __forceinline__ bool slot_blocked(const P& p, const LaneSlot& s, int si, int act, int dx, int dy) {
  if constexpr (P::kTables == 2) return table_blocked(p, si, s.me, dx, dy);
  else return s.small != 0ull ? small_blocked(p, s.small, s.me, p.wall, dx, dy) : lane_blocked(p, s.me, p.wall, act);
}

// One action of a planner expansion from the agent's sweep (hit4_0 / hit4_1: agent_pushes4 of the lane's slots)
template <int GS, bool kTwo = false, typename P>
__device__ __forceinline__ uint32_t group_push_closure_swept(const P& p, const LaneSlot& s0, const LaneSlot& s1, uint32_t hit4_0,
                                                             uint32_t hit4_1, int lj, int gbase, unsigned long long gmask,
                                                             bool play, bool dead, int act, int dx, int dy) {
  const bool hit0 = play && !dead && ((hit4_0 >> act) & 1u) != 0u;
  const bool hit1 = kTwo && play && !dead && ((hit4_1 >> act) & 1u) != 0u;
  bool blk = false;
  if (hit0) blk = slot_blocked(p, s0, lj, act, dx, dy);
  if (kTwo && hit1) blk = blk || slot_blocked(p, s1, lj + GS, act, dx, dy);
  uint32_t fresh = static_cast<uint32_t>((__ballot(hit0) & gmask) >> gbase);
  if (kTwo) fresh |= static_cast<uint32_t>((__ballot(hit1) & gmask) >> gbase) << GS;
  if ((__ballot(blk) & gmask) != 0ull) dead = true;
  return group_push_closure_from<GS, kTwo>(p, s0, s1, lj, gbase, gmask, play, dead, 1u | fresh, fresh, act, dx, dy);
}

// (Looking up the wall verdict of EVERY movable ahead of the closure, so that its iterations wait for no memory, was tried for
// the one-step launches: 14.5 -> 14.4 us on the C4 shard -- those launches are not waiting for that chain.)
template <int GS, bool kTwo = false, typename P>
__device__ __forceinline__ uint32_t group_push_set(const P& p, const LaneSlot& s0, const LaneSlot& s1, int lj, int gbase,
                                                   unsigned long long gmask, bool play, int act, int dx, int dy) {
  const bool dead = group_agent_blocked<GS>(p, s0.xy, s0.ot, s0.small, lj, gbase, gmask, play, act);
  return group_push_closure<GS, kTwo>(p, s0, s1, lj, gbase, gmask, play, dead, act, dx, dy);
}

// The agent's wall test for all four actions of one state (planner expansion): the window rows are loaded
// once, LEFT / RIGHT are in-lane shifts, UP / DOWN take the neighbouring lane's row.  Bit a of the result =
// action a is blocked.  Same verdicts as four group_agent_blocked calls.
template <int GS, typename P>
__device__ __forceinline__ uint32_t group_agent_blocked4(const P& p, int xy, uint32_t ot, uint64_t small, int lj, int gbase,
                                                         unsigned long long gmask, bool play) {
  const LaneObj ag = lane_obj(static_cast<uint32_t>(__shfl(static_cast<int>(ot), gbase, PW_WAVE)), __shfl(xy, gbase, PW_WAVE));
  if constexpr (P::kTables != 0) {  // (one puzzle per launch: it has tables) three rows of the agent's wall table
    const int row = ag.y + 1, bit = ag.x + 1;
    uint64_t t[3];
#pragma unroll
    for (int k = 0; k < 3; k++) t[k] = (static_cast<unsigned>(row - 1 + k) < static_cast<unsigned>(p.Hs)) ? p.wtab[row - 1 + k] : 0ull;
    const bool in_x = static_cast<unsigned>(bit) < 64u;
    if (!play || (in_x && ((t[1] >> bit) & 1ull))) return 0u;  // already inside a wall: never "blocked" (puzzle.py:562)
    uint32_t m = 0;
    if (static_cast<unsigned>(bit - 1) < 64u && ((t[1] >> (bit - 1)) & 1ull)) m |= 1u;
    if (static_cast<unsigned>(bit + 1) < 64u && ((t[1] >> (bit + 1)) & 1ull)) m |= 2u;
    if (in_x && ((t[0] >> bit) & 1ull)) m |= 4u;
    if (in_x && ((t[2] >> bit) & 1ull)) m |= 8u;
    return m;
  }
  if (__ballot(ag.h + 2 > GS) != 0ull) {
    uint32_t m = 0;
    for (int act = 0; act < 4; act++)
      if (group_agent_blocked<GS>(p, xy, ot, small, lj, gbase, gmask, play, act)) m |= 1u << act;
    return m;
  }
  const uint64_t asmall = __shfl(static_cast<unsigned long long>(small), gbase, PW_WAVE);
  const int yy = ag.y - 1 + lj;
  const bool in_win = play && lj < ag.h + 2;
  // the agent's row yy: out of its 8 x 8 board when it has one, else from the shape rows (0 outside the object's rows)
  const uint64_t sh = !in_win ? 0ull : (asmall != 0ull ? small_row(asmall, yy - ag.y, ag.x) : lane_row(p, ag, yy));
  const uint64_t g = (in_win && static_cast<unsigned>(yy) < static_cast<unsigned>(p.H)) ? p.awall[yy] : 0ull;
  // UP: new row yy holds old row yy + 1 (next lane); DOWN: old row yy - 1 (previous lane)
  uint64_t up = __shfl_down(sh, 1, PW_WAVE), dn = __shfl_up(sh, 1, PW_WAVE);
  if (lj == GS - 1 || yy == 63) up = 0ull;
  if (lj == 0 || yy == 0) dn = 0ull;
  const bool now = (sh & g) != 0ull;
  const bool overlapping = (__ballot(now) & gmask) != 0ull;  // already inside a wall: never "blocked" (puzzle.py:562)
  uint32_t m = 0;
  if ((__ballot(((sh >> 1) & g) != 0ull) & gmask) != 0ull) m |= 1u;
  if ((__ballot(((sh << 1) & g) != 0ull) & gmask) != 0ull) m |= 2u;
  if ((__ballot((up & g) != 0ull) & gmask) != 0ull) m |= 4u;
  if ((__ballot((dn & g) != 0ull) & gmask) != 0ull) m |= 8u;
  return (overlapping || !lane_inside(p, ag)) ? 0u : m;
}

// ------------------------------------------------------------------------------------
// K1d step / rollout, GS lanes per environment (lane j of a group = movable j)
//
// The lane-per-env kernel above is bound by the latency of its serial loop over the objects with
// one wave per SIMD; here the objects of an environment are tested in parallel (each lane asks
// "does the current pusher push MY object, and am I wall-blocked?"), the push set grows by ballots
// inside the 16- or 32-lane group, and a 65 536-env batch is 16 k waves instead of 1 k, so the
// remaining L1/L2 latencies overlap.  Default kernel of pw_step and pw_rollout.
// ------------------------------------------------------------------------------------
// kLds (PW_OPT_STEP_LDS_TABLES, the A/B of profiles/r02_step_ab.txt): every lane group first copies its puzzle's
// wall, agent-wall and shape rows (<= 2 KB) into LDS and all row reads of the push-set logic are ds_read_b64
// instead of global loads through L1.
#define PW_LDS_SHAPE_ROWS 128
// (__launch_bounds__(256, W) with W = 5 / 6 / 8 waves per SIMD instead of the 4 the 108 VGPRs allow: no gain at 5,
// spills and 1.5-1.8x slower at 6 and 8 -- profiles/r02_step_ab.txt)
// kSingle: the one-step-per-launch instance (pw_step, pw_step_render*): no step loop, no histories -- 58 VGPRs
// instead of 84, i.e. 8 instead of 5 waves per SIMD for a kernel that is bound by the latency of its loads.
// kTwo: two movables per lane (j = lane and j = GS + lane), see group_push_closure.
// kTab: 0 the engine has no overlap tables (PW_OPT_STEP_TABLES) -- no table code at all; 1 some puzzles of the set have
// them (both paths: 15-25 VGPRs more, one or two waves per SIMD fewer for a kernel that lives on hiding latencies);
// 2 every puzzle has them -- no row loops at all (and nothing to stage in LDS: kLds is not combined with it).
// (the body: the GS consecutive threads that share threadIdx.x / GS advance environment `env`; a workgroup may call it
// more than once, see pw_step_group_mixed_kernel)
template <int GS, bool kLds, bool kSingle, bool kTwo, int kTab>
__device__ __forceinline__ void step_group_body(const RolloutArgs& r, const int env) {
  const StepArgs& a = r.s;
  constexpr int kGroups = 256 / GS;
  const int lane = threadIdx.x & (PW_WAVE - 1);
  const int lj = threadIdx.x & (GS - 1);
  const int gbase = lane & ~(GS - 1);
  const unsigned long long gmask = ((1ull << (GS - 1) << 1) - 1ull) << gbase;
  // (an environment of a bound batch that belongs to a segment is stepped by the segment role of the launch)
  const bool live = env < a.batch && !(a.bound && a.bound[env]);
  const int e = live ? env : 0;

  const int pid = pw_clamp_pid(a.puzzle_id[e], a.num_puzzles);
  typename std::conditional<kLds, LanePuzzleT<PwLdsRows, kTab>, LanePuzzleT<const uint64_t*, kTab>>::type p;
  const PwPuzzleHeader* h = a.hdrs + pid;
  p.h = h;
  {
    const uint8_t* b = a.blob + h->base;
    const uint64_t* g_wall = reinterpret_cast<const uint64_t*>(b + h->off_wall);
    const uint64_t* g_awall = reinterpret_cast<const uint64_t*>(b + h->off_awall);
    const uint64_t* g_shapes = reinterpret_cast<const uint64_t*>(b + h->off_shapes);
    if constexpr (kLds) {
      __shared__ uint64_t s_rows[kGroups][2 * PW_MAX_DIM + PW_LDS_SHAPE_ROWS];
      uint64_t* mine = s_rows[threadIdx.x / GS];
      const int H = h->H, S = static_cast<int>((h->off_static - h->off_shapes) >> 3);
      for (int i = lj; i < H; i += GS) {
        mine[i] = g_wall[i];
        mine[PW_MAX_DIM + i] = g_awall[i];
      }
      for (int i = lj; i < S && i < PW_LDS_SHAPE_ROWS; i += GS) mine[2 * PW_MAX_DIM + i] = g_shapes[i];
      __syncthreads();
      p.wall = (PwLdsRows)(mine);
      p.awall = (PwLdsRows)(mine + PW_MAX_DIM);
      p.shapes = (PwLdsRows)(mine + 2 * PW_MAX_DIM);
    } else {
      p.wall = g_wall;
      p.awall = g_awall;
      p.shapes = g_shapes;
    }
  }
  lane_tables(p, a.ovl, a.ovl_dir, pid);
  p.H = h->H;
  p.N = live ? h->N : 0;
  p.G = h->G;
  const int N = p.N;
  int16_t* prow = reinterpret_cast<int16_t*>(a.pos) + static_cast<int64_t>(e) * a.np;
  int xy = (lj < N) ? static_cast<int>(static_cast<uint16_t>(prow[lj])) : 0;
  const uint32_t ot = (lj < N) ? reinterpret_cast<const uint32_t*>(h->objtab)[lj] : 0u;
  const uint64_t small = (lj < N) ? reinterpret_cast<const uint64_t*>(a.blob + h->base + h->off_small)[lj] : 0ull;
  const bool is_goal_lane = live && lj >= 1 && lj <= p.G;
  const int gxy = is_goal_lane ? static_cast<int>(reinterpret_cast<const uint16_t*>(h->goal)[lj - 1]) : -1;
  // second slot (kTwo): movable GS + lane
  const int lj1 = lj + GS;
  const bool has1 = kTwo && lj1 < N;
  int xy1 = has1 ? static_cast<int>(static_cast<uint16_t>(prow[lj1])) : 0;
  const uint32_t ot1 = has1 ? reinterpret_cast<const uint32_t*>(h->objtab)[lj1] : 0u;
  const uint64_t small1 = has1 ? reinterpret_cast<const uint64_t*>(a.blob + h->base + h->off_small)[lj1] : 0ull;
  const bool is_goal_lane1 = kTwo && live && lj1 <= p.G;
  const int gxy1 = is_goal_lane1 ? static_cast<int>(reinterpret_cast<const uint16_t*>(h->goal)[lj1 - 1]) : -1;
  int steps = a.steps[e], term = a.term[e], trunc = a.trunc[e];
  double reward = 0.0;
  int dgoals = 0;
  bool changed = false, any_played = false;
  bool was_reset = false;  // the environment was reset in this launch: the row's slots beyond the group's are zeroed below
  uint32_t n_ended = 0, n_solved = 0;  // wave-uniform sums over the wavefront's environments (pw_counters)
  int row_lo = 127, row_hi = -1;  // cell rows whose pixels the LAST step changed (a.dirty)

  const int n_steps = kSingle ? 1 : r.num_steps;
  // The actions of the next four steps are in flight while a step runs: every step's action is a new cache line (the
  // actions are [T][B]), and in a launch of many steps that load -- an HBM latency, several times the work of a step --
  // sat on every step's critical path.
  auto load_action = [&](int t) { return (live && t < n_steps) ? static_cast<int>(a.actions[static_cast<int64_t>(t) * a.batch + e]) : 0; };
  int q0 = load_action(0), q1 = 0, q2 = 0, q3 = 0;
  if (!kSingle) {
    q1 = load_action(1);
    q2 = load_action(2);
    q3 = load_action(3);
  }
  for (int t = 0; t < n_steps; t++) {
    const int64_t o = static_cast<int64_t>(t) * a.batch + e;
    const int act = q0;
    if (!kSingle) {
      q0 = q1;
      q1 = q2;
      q2 = q3;
      q3 = load_action(t + 4);
    }
    const bool do_reset = live && (a.flags & PW_STEP_AUTORESET) && (term | trunc);
    const bool bad = live && !do_reset && act > 3;
    const bool play = live && !do_reset && !bad;
    const int dx = act == 0 ? -1 : (act == 1 ? 1 : 0);
    const int dy = act == 2 ? -1 : (act == 3 ? 1 : 0);
    const LaneSlot s0 = lane_slot(xy, ot, small), s1 = lane_slot(xy1, ot1, small1);

    const uint32_t moved = group_push_set<GS, kTwo>(p, s0, s1, lj, gbase, gmask, play, act, dx, dy);

    // displaced state + goal bookkeeping (puzzle.py:384-411)
    int nxy = xy, nxy1 = xy1;
    if ((moved >> lj) & 1u) {
      const int x = static_cast<int8_t>(xy & 0xff) + dx, y = static_cast<int8_t>((xy >> 8) & 0xff) + dy;
      nxy = (x & 0xff) | ((y & 0xff) << 8);
    }
    if (kTwo && ((moved >> lj1) & 1u)) {
      const int x = static_cast<int8_t>(xy1 & 0xff) + dx, y = static_cast<int8_t>((xy1 >> 8) & 0xff) + dy;
      nxy1 = (x & 0xff) | ((y & 0xff) << 8);
    }
    int before = __popcll(__ballot(is_goal_lane && xy == gxy) & gmask);
    int after = __popcll(__ballot(is_goal_lane && nxy == gxy) & gmask);
    if (kTwo && __ballot(is_goal_lane1) != 0ull) {  // a puzzle with more than GS - 1 goals
      before += __popcll(__ballot(is_goal_lane1 && xy1 == gxy1) & gmask);
      after += __popcll(__ballot(is_goal_lane1 && nxy1 == gxy1) & gmask);
    }
    if (a.dirty) {  // rows swept by the moved objects, old and new position (pushed objects touch: one interval)
      int lo = 127, hi = -1;
      if ((moved >> lj) & 1u) {
        const int y1 = static_cast<int8_t>((nxy >> 8) & 0xff);
        lo = min(y1, y1 - dy);
        hi = max(y1, y1 - dy) + s0.me.h;
      }
      if (kTwo && ((moved >> lj1) & 1u)) {
        const int y1 = static_cast<int8_t>((nxy1 >> 8) & 0xff);
        lo = min(lo, min(y1, y1 - dy));
        hi = max(hi, max(y1, y1 - dy) + s1.me.h);
      }
#pragma unroll
      for (int o = GS / 2; o > 0; o >>= 1) {
        lo = min(lo, __shfl_xor(lo, o, GS));
        hi = max(hi, __shfl_xor(hi, o, GS));
      }
      row_lo = do_reset ? 0 : lo;
      row_hi = do_reset ? PW_MAX_DIM : hi;
    }
    if (play) {
      xy = nxy;
      xy1 = nxy1;
      changed = changed || moved != 0u;
      const bool terminated = after == p.G;  // vacuously true without goals (trap T8)
      steps += 1;
      term = terminated ? 1 : 0;
      trunc = (a.max_steps >= 0 && steps >= a.max_steps) ? 1 : 0;
      reward = terminated ? 10.0 : static_cast<double>(after - before) - 0.01;  // gym_env.py:212-221
      dgoals = after - before;
      any_played = true;
    } else if (do_reset) {
      xy = (lj < N) ? static_cast<int>(reinterpret_cast<const uint16_t*>(h->init)[lj]) : 0;
      xy1 = has1 ? static_cast<int>(reinterpret_cast<const uint16_t*>(h->init)[lj1]) : 0;
      changed = true;
      was_reset = true;
      steps = 0;
      term = 0;
      trunc = 0;
      reward = 0.0;
      dgoals = 0;
      any_played = true;
    } else if (bad) {  // not in Discrete(4): flag, leave the env untouched (gym_env.py:195-196)
      term = 0xFF;
      trunc = 0xFF;
      if (lj == 0) atomicAdd(a.bad_actions, 1u);
    }
    {
      const bool fin = live && lj == 0 && term != 0xFF;
      n_ended += static_cast<uint32_t>(__popcll(__ballot(fin && (term | trunc) != 0)));
      n_solved += static_cast<uint32_t>(__popcll(__ballot(fin && term != 0)));
    }
    if (!kSingle && live && lj == 0) {
      if (r.reward_hist) r.reward_hist[o] = reward;
      if (r.term_hist) r.term_hist[o] = static_cast<uint8_t>(term);
      if (r.trunc_hist) r.trunc_hist[o] = static_cast<uint8_t>(trunc);
    }
  }
  pw_count_add(a.counters, static_cast<uint32_t>(__popcll(__ballot(live && lj == 0))) * static_cast<uint32_t>(n_steps), n_ended, n_solved);
  if (!live) return;
  if (changed && lj < a.np) prow[lj] = static_cast<int16_t>(xy);
  if (kTwo && changed && lj1 < a.np) prow[lj1] = static_cast<int16_t>(xy1);
  // An episode that restarts on ANOTHER puzzle (pw_resample) may come from one with more movables than this group's lanes hold:
  // the slots beyond them return to zero with the reset (the layout's padding: include/pushworld_amd.h, pw_validate_state).
  if (was_reset)
    for (int sl = lj + (kTwo ? 2 : 1) * GS; sl < a.np; sl += GS) prow[sl] = 0;
  if (a.rec) {  // grid rows under some movable's bounding box: OR over the group's lanes
    uint64_t m = 0;
    if (lj < N) {
      const int y = static_cast<int8_t>((xy >> 8) & 0xff), hh = static_cast<int>((ot >> 8) & 0xffu);
      if (static_cast<unsigned>(y) < 64u) m = (hh >= 64 ? ~0ull : ((1ull << hh) - 1ull)) << y;
    }
    if (has1) {
      const int y = static_cast<int8_t>((xy1 >> 8) & 0xff), hh = static_cast<int>((ot1 >> 8) & 0xffu);
      if (static_cast<unsigned>(y) < 64u) m |= (hh >= 64 ? ~0ull : ((1ull << hh) - 1ull)) << y;
    }
#pragma unroll
    for (int o = GS / 2; o > 0; o >>= 1) m |= __shfl_xor(m, o, GS);
    if (lj == 0) {
      PageRec rec;
      rec.pid = pid;
      rec.H = h->H;
      rec.W = h->W;
      rec.reserved = 0;
      rec.rows = m;
      a.rec[env] = rec;
    }
    if (a.changed) {  // PW_OPT_OBS_CHANGED_PAGES: every lane compares its own movables with what the retained buffer shows
      uint16_t* srow = reinterpret_cast<uint16_t*>(a.shown) + static_cast<int64_t>(env) * a.np;
      uint64_t c = 0;
      if (lj < N) c = pw_shown_rows(srow[lj], static_cast<uint32_t>(xy), static_cast<int>((ot >> 8) & 0xffu));
      if (has1) c |= pw_shown_rows(srow[lj1], static_cast<uint32_t>(xy1), static_cast<int>((ot1 >> 8) & 0xffu));
#pragma unroll
      for (int o = GS / 2; o > 0; o >>= 1) c |= __shfl_xor(c, o, GS);
      if (c) {
        if (lj < N) srow[lj] = static_cast<uint16_t>(xy);
        if (has1) srow[lj1] = static_cast<uint16_t>(xy1);
      }
      if (lj == 0) a.changed[env] = c;
    }
  }
  if (lj == 0) {
    a.term[env] = static_cast<uint8_t>(term);
    a.trunc[env] = static_cast<uint8_t>(trunc);
    if (a.dirty) {
      const int lo = max(row_lo, 0), hi = min(row_hi, PW_MAX_DIM);
      a.dirty[env] = hi > lo ? static_cast<uint32_t>(lo | (hi << 8) | (p.H << 16)) : 0u;
    }
    if (any_played) {
      a.steps[env] = steps;
      if (a.reward) a.reward[env] = reward;
      if (a.dgoals) a.dgoals[env] = static_cast<int8_t>(dgoals);
    }
  }
}

// ------------------------------------------------------------------------------------
// K1e one step per launch on whole-grid boards of 16 x 16 cells, FOUR lanes per environment (VERDICT r4 #4)
//
// Puzzles whose grid (with its border walls) fits 16 x 16 cells, with at most 8 movables of at most 16 x 8 cells -- every
// Level-0 puzzle (7 .. 12 cells per side, 3 .. 5 movables) and 55 of the 68 Level-1 ones.  A board is 16 rows of 16 bits =
// 8 words of two rows; lane q of an environment's quad holds words 2q and 2q + 1 (rows 4q .. 4q + 3) of every board, so a
// movable on the grid is TWO registers per lane.  "i pushes j" = (moved_i & board_j) != 0 and (board_i & board_j) == 0,
// "j is stopped by a wall" likewise against the wall board: ANDs on registers, the four lanes' partial verdicts packed one
// bit per test into ONE word that is OR-reduced over the quad with two DPP instructions -- no ballot, no scalar
// instruction per test, no table.  A move is one v_alignbit per word (rows cross lanes through DPP quad_perm).
//
// Everything the step needs about the puzzle sits in ONE record per puzzle (PwQuadDesc, 576 bytes: counts, per-movable
// position limits, goals, initial positions, the wall boards, the movables' shapes) whose address depends on the puzzle id
// alone.  The dependent memory levels of a step are TWO: {puzzle id, positions, counters, action} -> {the record} ->
// registers; every load of a level is issued before anything waits (quad16_load, ahead of the workgroup's choice of
// formulation: a workgroup that does not take this path has read a few lines for nothing).  The lane groups walk id -> header /
// table directory -> boards / table rows -> wall rows.  A movable's board at (x, y) is an UNALIGNED 8-byte load out of its
// shape record (8 rows of 16 bits between 32 zero bytes either side: the row offset y is part of the address) shifted by x.
//
// Exactness: the board verdicts are the reference's (puzzle.py:522-593) as long as every movable lies inside the grid --
// cells outside a 16 x 16 window do not exist on a board, and a movable that is not entirely inside the grid is never
// stopped by a wall (the bounds clause, puzzle.py:557-561).  A state with a movable outside the grid (reachable only from
// states that overlap a wall; the position limits are checked bytewise) takes the quad through the table formulation
// (group_push_set<4, .>) instead.  Launches of several steps stay with the lane groups: boards kept from step to step double
// the registers of every path of the kernel they share (191 instead of 117: rollouts of the C4 shard 290 -> 460 us).
// ------------------------------------------------------------------------------------
#define PW_QD_BYTES 576
#define PW_QD_LIM 16      // uint8 [8][2]: W - w_j, H - h_j (0x7f beyond N)
#define PW_QD_GOAL 32     // int8 [8][2]: goal of movable j (j = 1 .. G)
#define PW_QD_INIT 48     // int8 [8][2]
#define PW_QD_WALL 64     // uint32 [8]: rows 2k | (2k + 1) << 16
#define PW_QD_AWALL 96    // uint32 [8]: wall | agent wall
#define PW_QD_SHAPE 160   // movable j: 8 rows of uint16 at PW_QD_SHAPE + 48 j, 32 zero bytes before and after
#define PW_QD_SHAPE_STRIDE 48

// value of the previous / next lane of the quad (0 at the quad's ends), OR over the quad
__device__ __forceinline__ uint32_t quad_prev(uint32_t v, int q) {
  const uint32_t t = static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x90, 0xf, 0xf, false));  // quad_perm [0,0,1,2]
  return q == 0 ? 0u : t;
}
__device__ __forceinline__ uint32_t quad_next(uint32_t v, int q) {
  const uint32_t t = static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0xF9, 0xf, 0xf, false));  // quad_perm [1,2,3,3]
  return q == 3 ? 0u : t;
}
__device__ __forceinline__ uint32_t quad_or(uint32_t v) {
  v |= static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0xB1, 0xf, 0xf, false));  // quad_perm [1,0,3,2]
  v |= static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x4E, 0xf, 0xf, false));  // quad_perm [2,3,0,1]
  return v;
}

// the lane's two words of a board moved by one cell: `odd` = RIGHT / DOWN (cells come from the lower word), sh = 1 / 31 / 16 /
// 16 for L / R / U / D, keep clears the column that wrapped into the neighbouring row
__device__ __forceinline__ void quad_shift(uint32_t w0, uint32_t w1, int q, bool odd, uint32_t sh, uint32_t keep, uint32_t& m0,
                                           uint32_t& m1) {
  const uint32_t pv = quad_prev(w1, q), nx = quad_next(w0, q);
  m0 = __builtin_amdgcn_alignbit(odd ? w0 : w1, odd ? pv : w0, sh) & keep;
  m1 = __builtin_amdgcn_alignbit(odd ? w1 : nx, odd ? w0 : w1, sh) & keep;
}

// bytewise a + d of packed int8 values (no carry between the bytes)
__device__ __forceinline__ uint32_t bytes_add(uint32_t a, uint32_t d) {
  return ((a & 0x7f7f7f7fu) + (d & 0x7f7f7f7fu)) ^ ((a ^ d) & 0x80808080u);
}

// what a lane of a quad reads before its workgroup knows which formulation it runs: level 0 (environment) and level 1 (record)
struct QuadIn {
  int pid;
  uint32_t P[4];           // positions of movables 0 .. 7 (N_pad 4 rows: the upper half zero)
  int steps, term, trunc, act;
  int masked;              // a bound batch: the environment belongs to a segment (StepArgs::bound), this role skips it
  uint32_t meta, nreal;    // W | H << 8 | N << 16 | G << 24 (N = 0: no record); the puzzle's real movable count
  uint32_t LIM[4], GOAL[4];
  uint2 wall, awall;       // the lane's words 2q, 2q + 1
  uint32_t B0[8], B1[8];   // the lane's words of the movables' boards at their positions (0 .. 3 always, 4 .. 7 when asked for)
};

// the lane's words of movable j's board at position xy: 8 bytes out of its shape record, the row offset in the address
__device__ __forceinline__ void quad_place(const uint8_t* d, int j, uint32_t xy, int q, uint32_t& w0, uint32_t& w1) {
  const int x = static_cast<int>(xy & 0xfu), y = min(static_cast<int>((xy >> 8) & 0xffu), 16);  // (inside the grid: 0 .. 15)
  const uint2 v = *reinterpret_cast<const uint2*>(d + PW_QD_SHAPE + PW_QD_SHAPE_STRIDE * j - 2 * y + 8 * q);
  w0 = v.x << x;
  w1 = v.y << x;
}

__device__ __forceinline__ void quad16_load(const StepArgs& a, int e, const uint8_t* qdesc, int q, QuadIn& in) {
  in.pid = pw_clamp_pid(a.puzzle_id[e], a.num_puzzles);
  const uint32_t* prow = reinterpret_cast<const uint32_t*>(a.pos) + static_cast<int64_t>(e) * (a.np / 2);
  if (a.np >= 8) {
    const uint4 v = *reinterpret_cast<const uint4*>(prow);
    in.P[0] = v.x, in.P[1] = v.y, in.P[2] = v.z, in.P[3] = v.w;
  } else {
    const uint2 v = *reinterpret_cast<const uint2*>(prow);
    in.P[0] = v.x, in.P[1] = v.y, in.P[2] = 0u, in.P[3] = 0u;
  }
  in.steps = a.steps[e];
  in.term = a.term[e];
  in.trunc = a.trunc[e];
  in.act = a.actions[e];
  in.masked = a.bound ? a.bound[e] : 0;  // (read HERE, with the other first-level loads: a read after the workgroup's reduction is a latency of its own)
  const uint8_t* d = qdesc + static_cast<size_t>(in.pid) * PW_QD_BYTES;
  const uint2 m = *reinterpret_cast<const uint2*>(d);
  in.meta = m.x;
  in.nreal = m.y & 0xffu;
  const uint4 limv = *reinterpret_cast<const uint4*>(d + PW_QD_LIM);
  const uint4 goalv = *reinterpret_cast<const uint4*>(d + PW_QD_GOAL);
  in.LIM[0] = limv.x, in.LIM[1] = limv.y, in.LIM[2] = limv.z, in.LIM[3] = limv.w;
  in.GOAL[0] = goalv.x, in.GOAL[1] = goalv.y, in.GOAL[2] = goalv.z, in.GOAL[3] = goalv.w;
  in.wall = *reinterpret_cast<const uint2*>(d + PW_QD_WALL + 8 * q);
  in.awall = *reinterpret_cast<const uint2*>(d + PW_QD_AWALL + 8 * q);
#pragma unroll
  for (int j = 0; j < 4; j++) quad_place(d, j, (in.P[j >> 1] >> (16 * (j & 1))) & 0xffffu, q, in.B0[j], in.B1[j]);
#pragma unroll
  for (int j = 4; j < 8; j++) in.B0[j] = in.B1[j] = 0u;
}

// NB: movables the instance carries (4: puzzles with at most 4 movables -- half the registers and instructions; 8)
template <int NB>
__device__ __forceinline__ void step_quad16_body(const StepArgs& a, const int env, const uint8_t* qdesc, QuadIn& in) {
  const int lane = threadIdx.x & (PW_WAVE - 1);
  const int q = threadIdx.x & 3;
  const int gbase = lane & ~3;
  const unsigned long long gmask = 0xFull << gbase;
  const bool live = env < a.batch && !in.masked;
  const int pid = in.pid;
  const uint8_t* d = qdesc + static_cast<size_t>(pid) * PW_QD_BYTES;
  const int W = static_cast<int>(in.meta & 0xffu), H = static_cast<int>((in.meta >> 8) & 0xffu);
  const int N = live ? static_cast<int>((in.meta >> 16) & 0xffu) : 0, G = static_cast<int>(in.meta >> 24);
  uint32_t (&P)[4] = in.P;
  uint32_t (&B0)[8] = in.B0;
  uint32_t (&B1)[8] = in.B1;
  if (NB == 8 && __ballot(N > 4) != 0ull) {  // (wave-uniform; the second level of a few Level-0 puzzles: five movables)
#pragma unroll
    for (int j = 4; j < 8; j++) quad_place(d, j, (P[j >> 1] >> (16 * (j & 1))) & 0xffffu, q, B0[j], B1[j]);
  }
  // every movable inside the grid: bytewise 0 <= P <= LIM  (LIM < 0x80, so (LIM | 0x80) - P borrows nothing between bytes)
  uint32_t outside = 0u;
#pragma unroll
  for (int k = 0; k < NB / 2; k++) outside |= (P[k] | ~((in.LIM[k] | 0x80808080u) - (P[k] & 0x7f7f7f7fu))) & 0x80808080u;
  const bool fast = outside == 0u;  // the boards are the state (false: a movable is outside the grid, the tables decide)

  int steps = in.steps, term = in.term, trunc = in.trunc;
  const int act = in.act;
  double reward = 0.0;
  int dgoals = 0;
  bool changed = false, any_played = false;
  int row_lo = 127, row_hi = -1;
  const bool do_reset = live && (a.flags & PW_STEP_AUTORESET) && (term | trunc);
  const bool bad = live && !do_reset && act > 3;
  const bool play = live && !do_reset && !bad;
  const int dx = act == 0 ? -1 : (act == 1 ? 1 : 0);
  const int dy = act == 2 ? -1 : (act == 3 ? 1 : 0);
  uint32_t pushed = 0u;  // bit j: movable j moves
  if (play && fast) {
    const bool odd = (act & 1) != 0;
    const uint32_t sh = act == 0 ? 1u : (act == 1 ? 31u : 16u);
    const uint32_t keep = act == 0 ? 0x7fff7fffu : (act == 1 ? 0xfffefffeu : 0xffffffffu);
    // one bit per test and lane, OR-reduced over the quad at once: 4 j + 0 moved_j hits a wall, + 1 j overlaps a wall now,
    // + 2 the moved agent hits j, + 3 the agent overlaps j now
    uint32_t M0[NB], M1[NB];
    uint32_t acc = 0u;
    quad_shift(B0[0], B1[0], q, odd, sh, keep, M0[0], M1[0]);
    acc |= min(((M0[0] & in.awall.x) | (M1[0] & in.awall.y)), 1u) << 0;
    acc |= min(((B0[0] & in.awall.x) | (B1[0] & in.awall.y)), 1u) << 1;
#pragma unroll
    for (int j = 1; j < NB; j++) {
      quad_shift(B0[j], B1[j], q, odd, sh, keep, M0[j], M1[j]);
      acc |= min(((M0[j] & in.wall.x) | (M1[j] & in.wall.y)), 1u) << (4 * j + 0);
      acc |= min(((B0[j] & in.wall.x) | (B1[j] & in.wall.y)), 1u) << (4 * j + 1);
      acc |= min(((M0[0] & B0[j]) | (M1[0] & B1[j])), 1u) << (4 * j + 2);
      acc |= min(((B0[0] & B0[j]) | (B1[0] & B1[j])), 1u) << (4 * j + 3);
    }
    acc = quad_or(acc);
    const uint32_t stop4 = acc & ~(acc >> 1) & 0x11111111u;         // bit 4 j: j would be stopped by a wall
    const uint32_t push4 = (acc >> 2) & ~(acc >> 3) & 0x11111110u;  // bit 4 j: the agent pushes j
    if (!(stop4 & 1u)) {  // the agent is free to move (puzzle.py:353)
      uint32_t in4 = 1u | push4, frontier = push4;
      bool blocked = (push4 & stop4) != 0u;
      // pushed movables push further ones (about 0.1 % of the steps): the quad's next pusher is the lowest of `frontier`
      while (frontier != 0u && !blocked) {
        const int i4 = __ffs(frontier) - 1;
        frontier &= frontier - 1u;
        uint32_t bi0 = 0u, bi1 = 0u, mi0 = 0u, mi1 = 0u;
#pragma unroll
        for (int k = 1; k < NB; k++) {
          const bool is = i4 == 4 * k;
          bi0 = is ? B0[k] : bi0;
          bi1 = is ? B1[k] : bi1;
          mi0 = is ? M0[k] : mi0;
          mi1 = is ? M1[k] : mi1;
        }
        uint32_t acc2 = 0u;
#pragma unroll
        for (int j = 1; j < NB; j++) {
          acc2 |= min(((mi0 & B0[j]) | (mi1 & B1[j])), 1u) << (4 * j + 2);
          acc2 |= min(((bi0 & B0[j]) | (bi1 & B1[j])), 1u) << (4 * j + 3);
        }
        acc2 = quad_or(acc2);
        const uint32_t fresh = (acc2 >> 2) & ~(acc2 >> 3) & 0x11111110u & ~in4;
        blocked = (fresh & stop4) != 0u;  // ... one of them into a wall: nothing moves (puzzle.py:376-379)
        in4 |= fresh;
        frontier |= fresh;
      }
      if (!blocked) {
#pragma unroll
        for (int j = 0; j < NB; j++) pushed |= ((in4 >> (4 * j)) & 1u) << j;
      }
    }
  } else if (play) {
    // a movable outside the grid: the table formulation, lane q = movables q and q + 4 (no 8 x 8 boards: every test a table test)
    LanePuzzleT<const uint64_t*, 2> p;
    p.h = a.hdrs + pid;
    p.wall = nullptr;
    p.awall = nullptr;
    p.shapes = nullptr;
    p.H = H;
    p.N = N;
    p.G = G;
    lane_tables(p, a.ovl, a.ovl_dir, pid);
    auto slot_of = [&](int j) {  // (j differs between the lanes: selects, not an indexed -- memory -- access)
      uint32_t pw = 0u, lw = 0u;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        pw = (k == ((j >> 1) & 3)) ? P[k] : pw;
        lw = (k == ((j >> 1) & 3)) ? in.LIM[k] : lw;
      }
      const uint32_t xy = (pw >> (16 * (j & 1))) & 0xffffu;
      const uint32_t lim = (lw >> (16 * (j & 1))) & 0xffffu;
      const uint32_t ot = j < N ? static_cast<uint32_t>(W - static_cast<int>(lim & 0xffu)) | (static_cast<uint32_t>(H - static_cast<int>(lim >> 8)) << 8) : 0u;
      return lane_slot(j < N ? static_cast<int>(xy) : 0, ot, 0ull);
    };
    const LaneSlot s0 = slot_of(q), s1 = slot_of(NB == 8 ? q + 4 : 8);  // (NB = 4: the second slot is empty)
    pushed = group_push_set<4, NB == 8>(p, s0, s1, q, gbase, gmask, true, act, dx, dy);
  }

  // displaced state + goal bookkeeping (puzzle.py:384-411); every lane of the quad holds all positions
  int before = 0, after = 0;
  uint32_t NP_[NB / 2];
  {
    const uint32_t delta = static_cast<uint32_t>(dx & 0xff) | (static_cast<uint32_t>(dy & 0xff) << 8);
#pragma unroll
    for (int k = 0; k < NB / 2; k++) {
      const uint32_t dd = (((pushed >> (2 * k)) & 1u) ? delta : 0u) | (((pushed >> (2 * k + 1)) & 1u) ? delta << 16 : 0u);
      NP_[k] = bytes_add(P[k], dd);
    }
#pragma unroll
    for (int j = 1; j < NB; j++) {
      const uint32_t sft = 16 * (j & 1);
      const uint32_t g = (in.GOAL[j >> 1] >> sft) & 0xffffu;
      before += j <= G && ((P[j >> 1] >> sft) & 0xffffu) == g;
      after += j <= G && ((NP_[j >> 1] >> sft) & 0xffffu) == g;
    }
  }
  if (a.dirty) {  // rows swept by the moved objects, old and new position (pushed objects touch: one interval)
    int lo = 127, hi = -1;
#pragma unroll
    for (int j = 0; j < NB; j++) {
      if ((pushed >> j) & 1u) {
        const int y1 = static_cast<int8_t>((NP_[j >> 1] >> (16 * (j & 1) + 8)) & 0xffu);
        const int hh = H - static_cast<int>((in.LIM[j >> 1] >> (16 * (j & 1) + 8)) & 0xffu);
        lo = min(lo, min(y1, y1 - dy));
        hi = max(hi, max(y1, y1 - dy) + hh);
      }
    }
    row_lo = do_reset ? 0 : lo;
    row_hi = do_reset ? PW_MAX_DIM : hi;
  }
  if (play) {
#pragma unroll
    for (int k = 0; k < NB / 2; k++) P[k] = NP_[k];
    changed = pushed != 0u;
    const bool terminated = after == G;  // vacuously true without goals (trap T8)
    steps += 1;
    term = terminated ? 1 : 0;
    trunc = (a.max_steps >= 0 && steps >= a.max_steps) ? 1 : 0;
    reward = terminated ? 10.0 : static_cast<double>(after - before) - 0.01;  // gym_env.py:212-221
    dgoals = after - before;
    any_played = true;
  } else if (do_reset) {
#pragma unroll
    for (int k = 0; k < NB / 2; k++) P[k] = reinterpret_cast<const uint32_t*>(d + PW_QD_INIT)[k];
    changed = true;
    steps = 0;
    term = 0;
    trunc = 0;
    any_played = true;
  } else if (bad) {  // not in Discrete(4): flag, leave the env untouched (gym_env.py:195-196)
    term = 0xFF;
    trunc = 0xFF;
    if (q == 0) atomicAdd(a.bad_actions, 1u);
  }
  {
    const bool fin = live && q == 0 && term != 0xFF;
    pw_count_add(a.counters, static_cast<uint32_t>(__popcll(__ballot(live && q == 0))),
                 static_cast<uint32_t>(__popcll(__ballot(fin && (term | trunc) != 0))), static_cast<uint32_t>(__popcll(__ballot(fin && term != 0))));
  }
  if (!live || q != 0) return;
  uint32_t* prow = reinterpret_cast<uint32_t*>(a.pos) + static_cast<int64_t>(env) * (a.np / 2);
  if (changed) {
    if (NB == 8 && a.np >= 8) *reinterpret_cast<uint4*>(prow) = make_uint4(P[0], P[1], P[2], P[3]);
    else *reinterpret_cast<uint2*>(prow) = make_uint2(P[0], P[1]);
  }
  // (an episode that restarts on another puzzle -- pw_resample -- may come from one with more movables: zero padding beyond
  // what this instance holds)
  if (do_reset)
    for (int k = (NB == 8 && a.np >= 8) ? 4 : 2; k < a.np / 2; k++) prow[k] = 0u;
  if (a.rec) {  // grid rows under some movable's bounding box
    uint64_t m = 0;
#pragma unroll
    for (int j = 0; j < NB; j++) {
      if (j < N) {
        const int y = static_cast<int8_t>((P[j >> 1] >> (16 * (j & 1) + 8)) & 0xffu);
        const int hh = H - static_cast<int>((in.LIM[j >> 1] >> (16 * (j & 1) + 8)) & 0xffu);
        if (static_cast<unsigned>(y) < 64u) m |= ((1ull << hh) - 1ull) << y;
      }
    }
    PageRec rec;
    rec.pid = pid;
    rec.H = static_cast<uint8_t>(H);
    rec.W = static_cast<uint8_t>(W);
    rec.reserved = 0;
    rec.rows = m;
    a.rec[env] = rec;
    if (a.changed) {  // PW_OPT_OBS_CHANGED_PAGES (from the state as stored above and the puzzle header: no register array is indexed)
      const PwObjEntry* objtab = a.hdrs[pid].objtab;
      pw_shown_update(a.pos + static_cast<int64_t>(env) * a.np * 2, a.shown + static_cast<int64_t>(env) * a.np * 2, a.changed + env, N,
                      [&](int j) { return static_cast<int>(objtab[j].h); });
    }
  }
  a.term[env] = static_cast<uint8_t>(term);
  a.trunc[env] = static_cast<uint8_t>(trunc);
  if (a.dirty) {
    const int lo = max(row_lo, 0), hi = min(row_hi, PW_MAX_DIM);
    a.dirty[env] = hi > lo ? static_cast<uint32_t>(lo | (hi << 8) | (H << 16)) : 0u;
  }
  if (any_played) {
    a.steps[env] = steps;
    if (a.reward) a.reward[env] = reward;
    if (a.dgoals) a.dgoals[env] = static_cast<int8_t>(dgoals);
  }
}

#include "pw_seg_kernels.inc"

// Which block of environments workgroup b of nb takes (PW_OPT_STEP_BLOCK_ORDER).  Bit 1: XCD-contiguous -- workgroups are
// dispatched round robin over the 8 XCDs (b mod 8), each with an L2 of its own; with the plain order the workgroups of ONE puzzle
// (batches are sorted by puzzle) land on all eight, and every L2 holds every puzzle's tables.  Here XCD x takes the x-th
// contiguous eighth of the blocks: an L2 sees an eighth of the puzzles.  Bit 0: the last block first.
__device__ __forceinline__ unsigned pw_block_order(unsigned b, unsigned nb, int order) {
  if (order & 2) {
    const unsigned x = b & 7u, q = nb >> 3, rem = nb & 7u;  // XCD x owns q + (x < rem) blocks, starting at x q + min(x, rem)
    b = x * q + min(x, rem) + (b >> 3);
  }
  return (order & 1) ? nb - 1u - b : b;
}

template <int GS, bool kLds = false, bool kSingle = false, bool kTwo = false, int kTab = 0>
__global__ __launch_bounds__(256) void pw_step_group_kernel(RolloutArgs r) {
  const unsigned blk = pw_block_order(blockIdx.x, gridDim.x, r.s.reverse);
  step_group_body<GS, kLds, kSingle, kTwo, kTab>(r, static_cast<int>(blk) * (256 / GS) + static_cast<int>(threadIdx.x) / GS);
}

// N_pad 32 sets with tables for every puzzle: most of their environments still have at most 16 movables (the C4 shard: the
// Level-0 half and all but a handful of the Level 1-4 puzzles) and fit 8 lanes with two movables each -- 8 environments per
// wavefront instead of the 4 of the 16-lane groups that the few puzzles with 17 .. 32 movables need.  A workgroup owns 32
// consecutive environments (batches are sorted by puzzle: the choice is uniform over long runs) and looks at their N first:
// none beyond 16 -> one pass in 8-lane groups.  Otherwise 16-lane groups, 16 environments at a time: one step per launch
// (kSingle) the same workgroup runs both halves one after the other (two short latency chains, still shorter than the
// launch); launches of several steps hand the second half to a twin workgroup of the FIRST half of the grid (twins of
// narrow workgroups leave at once; the long-running second halves start at t = 0, not at the tail).
// kNoWide: a set without a puzzle beyond 16 movables (N_pad 8 / 16 sets with tables for every puzzle): no twin workgroups, no
// 16-lane code -- what is left is the choice of 4 lanes / 8 lanes with one movable / 8 lanes with two movables per workgroup.
// kSeg: the instance that carries the SEGMENT role of a bound batch at the front of its grid (single steps only: a lane of that
// role holds a whole environment in registers, which launches of several steps must not make the lane groups pay for)
template <bool kSingle, bool kNoWide = false, bool kSeg = false>
__global__ __launch_bounds__(256) void pw_step_group_mixed_kernel(RolloutArgs r) {
  const StepArgs& a = r.s;
  unsigned bid = blockIdx.x, grid = gridDim.x;
  if constexpr (kSeg) {
    // A bound batch (pw_batch_bind): the first seg_grid workgroups of the launch step the SEGMENTS -- one lane per environment, the
    // puzzle's push tables in LDS (pw_seg_kernels.inc) -- and the others, below, the environments no segment holds.  One launch:
    // both roles start together (the segments first: the longer-running Level 1-4 puzzles).
    extern __shared__ __attribute__((aligned(16))) uint8_t s_seg_tab[];  // (the launch's dynamic LDS: the largest bound block)
    if (bid < static_cast<unsigned>(a.seg_grid)) {
      if (static_cast<int>(bid) < a.bind_meta[0]) {
        if constexpr (kNoWide) {
          if (a.np == 4) step_seg_body<4, kSingle>(r, static_cast<int>(bid), s_seg_tab);
          else if (a.np == 8) step_seg_body<8, kSingle>(r, static_cast<int>(bid), s_seg_tab);
          else step_seg_body<16, kSingle>(r, static_cast<int>(bid), s_seg_tab);
        } else {
          step_seg_body<32, kSingle>(r, static_cast<int>(bid), s_seg_tab);
        }
      }
      return;
    }
    bid -= static_cast<unsigned>(a.seg_grid);
    grid -= static_cast<unsigned>(a.seg_grid);
  }
  const unsigned nb = (kSingle || kNoWide) ? grid : grid / 2u;  // workgroups that own 32 environments
  const bool twin = !(kSingle || kNoWide) && bid < nb;
  const unsigned own = twin ? bid : bid - ((kSingle || kNoWide) ? 0u : nb);
  const unsigned blk = pw_block_order(own, nb, a.reverse);
  const int base = static_cast<int>(blk) * 32;
  const int e8 = base + static_cast<int>(threadIdx.x) / 8;
  // bit 4 of the workgroup's class word: one of its 32 environments is NOT held by a segment (a workgroup without one leaves)
  auto unbound = [&](int e) { return (e < a.batch && !(a.bound && a.bound[e])) ? 16 : 0; };
  int cls4;
  if constexpr (kSingle) {
    if (a.qdesc) {
      // One step per launch on a set with 16 x 16 records: the first two wavefronts read, four lanes per environment, what the
      // whole-grid formulation needs (environment AND record: two memory levels, every load in flight at once) and tell the
      // workgroup what its 32 puzzles are -- bit 3 = one without a record, bit 2 = one beyond 16 movables, bit 1 = beyond 8,
      // bit 0 = beyond 4 -- in one reduction.
      QuadIn in;
      const int e4 = base + static_cast<int>(threadIdx.x) / 4;
      int bits = 0;
      if (threadIdx.x < 128) {
        quad16_load(a, e4 < a.batch ? e4 : 0, a.qdesc, static_cast<int>(threadIdx.x) & 3, in);
        if (e4 < a.batch) {
          const int n = static_cast<int>(in.nreal);
          bits = (n > 16 ? 4 : (n > 8 ? 2 : (n > 4 ? 1 : 0))) | (((in.meta >> 16) & 0xffu) == 0u ? 8 : 0) | (in.masked ? 0 : 16);
        }
      }
      cls4 = __ockl_wgred_or_i32(bits);
      if (!(cls4 & 16)) return;
      if (!(cls4 & 8)) {  // every environment of the workgroup fits the boards: registers only from here
        if (threadIdx.x < 128) {
          if ((cls4 & 7) == 0) step_quad16_body<4>(a, e4, a.qdesc, in);
          else step_quad16_body<8>(a, e4, a.qdesc, in);
        }
        return;
      }
    } else {
      int n8 = 0;
      if (e8 < a.batch) n8 = a.hdrs[pw_clamp_pid(a.puzzle_id[e8], a.num_puzzles)].N;
      cls4 = __ockl_wgred_or_i32((n8 > 16 ? 4 : (n8 > 8 ? 2 : (n8 > 4 ? 1 : 0))) | unbound(e8));
      if (!(cls4 & 16)) return;
    }
  } else {
    int n8 = 0;
    if (e8 < a.batch) n8 = a.hdrs[pw_clamp_pid(a.puzzle_id[e8], a.num_puzzles)].N;
    // (one workgroup reduction for the three questions: bit 2 = a puzzle beyond 16 movables, bit 1 = one beyond 8, bit 0 = one
    // beyond 4)
    cls4 = __ockl_wgred_or_i32((n8 > 16 ? 4 : (n8 > 8 ? 2 : (n8 > 4 ? 1 : 0))) | unbound(e8));
    if (!(cls4 & 16)) return;
  }
  const int cls = cls4 & 7;
  const bool wide = !kNoWide && (cls & 4) != 0;
  if (kNoWide || !wide) {
    if (twin) return;
    if (cls == 0) {
      // at most 4 movables everywhere (the Level-0 half of the C4 shard: 3 or 4 movables in 98 % of its puzzles): 4 lanes per
      // environment -- the workgroup's 32 environments take its first two wavefronts, the other two leave
      if (threadIdx.x < 128) step_group_body<4, false, kSingle, false, 2>(r, base + static_cast<int>(threadIdx.x) / 4);
      return;
    }
    // at most 8 movables everywhere (most of Level 1-4): one movable per lane -- the second slot's share of the instructions
    // (a third of the step) is not issued at all
    // (5 .. 8 movables in 4 lanes with two movables each -- 16 environments per wavefront -- was tried: rollouts 1.42e10 ->
    // 1.32e10 env-steps/s on the C4 shard)
    if (cls == 1) step_group_body<8, false, kSingle, false, 2>(r, e8);
    else step_group_body<8, false, kSingle, true, 2>(r, e8);
    return;
  }
  if constexpr (!kNoWide) {
    if (kSingle) {
      step_group_body<16, false, kSingle, true, 2>(r, base + static_cast<int>(threadIdx.x) / 16);
      step_group_body<16, false, kSingle, true, 2>(r, base + 16 + static_cast<int>(threadIdx.x) / 16);
    } else {
      step_group_body<16, false, kSingle, true, 2>(r, base + (twin ? 16 : 0) + static_cast<int>(threadIdx.x) / 16);
    }
  }
}

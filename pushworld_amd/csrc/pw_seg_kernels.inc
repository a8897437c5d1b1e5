// pw_seg_kernels.inc -- stepping of a BOUND batch (pw_batch_bind): one lane per environment, the puzzle's push tables in LDS.
// Part of the single translation unit pw_kernels.hip (included by pw_step_kernels.inc ahead of the lane-group kernels, which
// carry the segment role in their launches).
//
// The lane groups (pw_step_group_mixed_kernel) walk puzzle id -> header / directory -> table rows through L2 for every push
// test of every environment -- ~75 instructions and a chain of four dependent memory levels per env-step on the Level 1-4
// puzzles, 1.7x / 2.8x the algorithmic bytes in table rows (VERDICT r5 #4).  A batch whose puzzle ids are known in advance
// (pw_batch_bind) is cut into SEGMENTS: up to 256 environments of ONE puzzle per workgroup.  The workgroup copies that puzzle's
// block -- per-pair push tables (one nibble per relative offset = all four actions, puzzle.py:567-593), wall bitmaps
// (puzzle.py:522-564), object table -- into LDS once (median 3 KB, 222 of the 223 benchmark puzzles within 16 KB), then every
// lane steps its own environment: a push test is two subtractions, two minima, one multiply-add and one ds_read_u8; the
// environment lives in registers between the steps of a rollout.  Same verdicts as every other formulation (gym_env.py:188-226,
// puzzle.py:348-411; tests/test_gpu_parity.py, tests/test_gpu_deep.py, tests/test_gpu_bind.py).

#define PW_SEG_LDS_BYTES 49152  // largest block that is bound (all 223 benchmark puzzles: `Mind The Gap` needs 37 KB, the next 15 KB, the median 3 KB).
                                // The launches carry as much dynamic LDS as the largest block among the BOUND puzzles needs.
#define PW_SEG_ENVS 256         // environments per segment = threads per workgroup
#define PW_SEG_ACT_TILE 8        // launches of several steps: the actions of this many steps are staged in LDS at a time

// Per puzzle: where its block lives and what is in it (engine-built, csrc/pw_engine.inc build_seg_tables).  Block layout:
//   0          uint32 desc[N][NS]   pair (i, j): byte offset of its table | (columns - 1) << 16 | guard row index << 24.  NS = N rounded up
//                                   to a multiple of 4; j == 0, i == j and j >= N point at a one-byte zero table (the agent is
//                                   never pushed, puzzle.py:364): a lookup of such a pair needs no test, it finds "no push"
//   obj_off    uint32 objtab[NS]    w | h << 8 | shape row offset << 16 (PwObjEntry)
//   goal_off   uint16 goal[NS]      goal[j] = packed (x, y) target of movable j (j = 1 .. G; 0xFFFF elsewhere)
//   init_off   uint32 init[NS / 2]  initial positions, two movables per word
//   wall_off   wall tables, in one of two forms (wall_fmt):
//              1 (the segment kernels' blocks)  stop[N][Hs + 2][wall_stride] nibbles, two per byte: nibble (y + 2, x + 2) of movable j, bit a =
//                                   "j at (x, y) is stopped by a wall in action a" = it overlaps one after the move and none now (puzzle.py:522-564;
//                                   j = 0: or an agent wall).  One row / column further than the bitmaps on every side: a position out of the
//                                   grid whose move leads into it still finds its verdict; beyond that nothing stops (no overlap).  W + 4
//                                   nibbles per row (wall_cols), wall_per bytes per movable
//              0 (the blocks of pw_step_mseg_kernel: a lane's slot holds ~1 KB)  wall[N][Hs] rows, bit (x + 1) of row (y + 1): movable j at
//                                   (x, y) overlaps a wall; rows of wall_stride bytes: uint16 where W + 2 <= 16, else uint64
//   ...        pair tables          (i, j): h_i + h_j + 2 rows of w_i + w_j + 2 bytes, byte (ry + h_i, rx + w_i) = nibble, bit a
//                                   = "i at (rx, ry) relative to j overlaps it after action a and not now"; the last row and
//                                   column are zero guards (a lookup clamps instead of testing)
struct PwSegDir {
  uint32_t off;       // 8-byte units from PwEngine::d_ovl; 0 = no block (no overlap tables, or beyond PW_SEG_LDS_BYTES)
  uint32_t bytes;     // multiple of 16
  uint16_t wall_off, obj_off, goal_off, init_off;
  uint16_t Hs;        // H + 2
  uint8_t N, G, NS;
  uint8_t init_goals; // count_achieved_goals(initial state) (puzzle.py:396-407)
  uint16_t w0h0;      // the agent's w | h << 8
  uint8_t wall_stride;  // bytes per wall row -- bitmaps: 2 (grids up to 14 columns + border: every Level-0 puzzle) or 8; nibbles: (W + 5) / 2
  uint8_t wall_fmt;     // 0 bitmaps, 1 stop nibbles
  uint8_t wall_cols;    // nibbles: W + 4
  uint8_t reserved0;
  uint16_t wall_per;    // nibbles: bytes per movable = (Hs + 2) * wall_stride
  uint8_t reserved[2];
};
static_assert(sizeof(PwSegDir) == 32, "PwSegDir is read with two 16-byte scalar loads");

struct PwSegDesc {    // one workgroup's share of a bound batch: 80 bytes, five 16-byte scalar loads at ONE address level
  int32_t pid;
  int32_t start;      // flags & 1: first environment (the puzzle's environments are consecutive); else first index into perm
  int32_t count;      // 1 .. PW_SEG_ENVS >> (lanes_log2 + spread_log2)
  int32_t flags;      // bit 0 consecutive environments, bits 8 .. 9 log2 of the lanes per environment (0 .. 3), bits 10 .. 12 log2 of the spread
                      // (only the first 64 >> spread lanes of a wavefront carry environments)
  PwSegDir dir;       // the puzzle's directory entry, copied by pw_bind_plan_kernel: a segment's workgroup reads its descriptor and
                      // then the block -- not descriptor -> directory -> block (a dependent memory level of a single-step launch)
  PwSegDir dir0;      // ... and the entry of the block with wall BITMAPS: what a launch of ONE step copies (it looks a wall up once or
                      // twice per environment: the smaller block is worth more than the cheaper test -- `Mind The Gap`: 37 instead of 42 KB
                      // of LDS for every workgroup of the launch, lane groups included; C4 shard 12.4 against 14.3 us per step)
};
static_assert(sizeof(PwSegDesc) == 80, "PwSegDesc layout");

// movable j's packed position out of the registers (j is a compile-time constant where it matters)
template <int NP>
__device__ __forceinline__ uint32_t seg_xy(const uint32_t (&P)[NP / 2], int j) {
  return (P[j >> 1] >> (16 * (j & 1))) & 0xffffu;
}

// P[idx] for a per-lane idx: a binary tree of selects (NP / 2 - 1 v_cndmask, log2 compares) instead of a chain of compare +
// select per register
template <int N>
__device__ __forceinline__ uint32_t seg_select(const uint32_t (&P)[N], uint32_t idx) {
  if constexpr (N == 1) {
    return P[0];
  } else {
    // (bit arithmetic -- one v_bfi_b32 per pair --, not `odd ? a : b`: the compiler recognises a tree of selects over an array as an
    // indexed load and moves the positions to SCRATCH memory to perform it)
    uint32_t H[N / 2];
    const uint32_t m = 0u - (idx & 1u);
#pragma unroll
    for (int k = 0; k < N / 2; k++) H[k] = (P[2 * k + 1] & m) | (P[2 * k] & ~m);
    return seg_select<N / 2>(H, idx >> 1);
  }
}

// f(block 0), f(block 1), ... while the block index is below `bound` (wave-uniform): NESTED tests, so that the blocks a puzzle does
// not have cost ONE taken branch, not one each (a wavefront alone on its SIMD pays an instruction-fetch restart per taken branch;
// `for (r) if (r < bound)` compiles into a test per block, and a `break` keeps the loop from unrolling -- the positions must stay
// registers with compile-time indices).  f takes the block index as a std::integral_constant.
template <int R, int RMAX, typename F>
__device__ __forceinline__ void seg_blocks(const int bound, F&& f) {
  if constexpr (R < RMAX) {
    if (R < bound) {
      f(std::integral_constant<int, R>{});
      seg_blocks<R + 1, RMAX>(bound, f);
    }
  }
}

// OR over the LPE lanes of an environment (DPP quad_perm, row_half_mirror)
template <int LPE>
__device__ __forceinline__ uint32_t seg_group_or(uint32_t v) {
  if constexpr (LPE >= 2) v |= static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0xB1, 0xf, 0xf, false));  // quad_perm [1,0,3,2]
  if constexpr (LPE >= 4) v |= static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x4E, 0xf, 0xf, false));  // quad_perm [2,3,0,1]
  if constexpr (LPE >= 8) v |= static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), 0x141, 0xf, 0xf, false));  // row_half_mirror: lane i <- 7 - i of its eight (the other quad)
  return v;
}

// The puzzle of a segment as the step sees it: LDS pointers into the block and its wave-uniform sizes.
struct SegPuzzle {
  const uint8_t* tab;       // the block (LDS)
  const uint32_t* pd;       // desc[N][NS]
  const uint32_t* obj;
  const uint16_t* goal;
  const uint32_t* init;
  const uint8_t* wall;
  int wstride;              // bytes per wall row
  int wper, wcols;          // stop nibbles (PwSegDir::wall_fmt 1): bytes per movable, nibbles per row
  int N, G, NS, NB, Hs, w0, h0, init_goals;
  int BPL;                  // blocks of four pairs a lane looks up per pass: ceil(NB / LPE)
  int NBu;                  // WAVE-UNIFORM bound of the block loops: NB in the segment kernels, the largest NB of the wavefront's 64
                            // puzzles in pw_step_mseg_kernel (a lane with fewer blocks masks what the surplus ones find)
  uint32_t jmask;           // bits of this lane's movables: (1 << NS) - 1
};

// LPE lanes per environment (1, 2, 4 or 8 consecutive lanes).  Every lane of an environment holds ALL its positions, as NB = NS / 4
// blocks of four movables (two registers each) -- ROTATED: register block r of lane q holds movable block (r + rot) mod NB, rot = q BPL mod NB, so
// that the same instruction stream ("look up the pairs of register blocks 0 .. BPL - 1") covers different movables in the LPE
// lanes, with the positions in registers at compile-time indices.  The partial push masks are OR-ed over the lanes (DPP); the
// rest of a step (walls, the move, goals, bookkeeping) is the same in all lanes of an environment.  Lane 0's registers are in
// natural order: it loads nothing rotated and is the one that stores.
//   jb_of(r)   first movable of register block r in this lane
template <int NP, int LPE>
struct SegLane {
  int q;      // lane of the environment
  int rot;    // (q * BPL) mod NB
  __device__ __forceinline__ int jb_of(int r, int NB) const {
    if constexpr (LPE == 1) return 4 * r;
    int t = r + rot;
    t -= t >= NB ? NB : 0;
    return 4 * t;
  }
};

// how many goal movables sit on their goals (puzzle.py:396-407)
template <int NP, int LPE>
__device__ __forceinline__ int seg_goals(const SegPuzzle& z, const SegLane<NP, LPE>& ln, const uint32_t (&P)[NP / 2]) {
  int n = 0;
  seg_blocks<0, NP / 4>(z.NBu, [&](auto rc) {
    constexpr int r = decltype(rc)::value;
    if (LPE == 1 ? 4 * r <= z.G : r < z.NB) {  // (goals are movables 1 .. G; a rotated lane looks at every block)
      const int jb = ln.jb_of(r, z.NB);
      // (element loads, here and below: a lane's block in pw_step_mseg_kernel is 4-byte aligned only -- the compiler pairs them)
      const uint32_t* gp = reinterpret_cast<const uint32_t*>(z.goal + jb);
      const uint2 g = make_uint2(gp[0], gp[1]);  // goal[j] = 0x8080 for j = 0 and beyond G: no position has it
      n += (P[2 * r] & 0xffffu) == (g.x & 0xffffu);
      n += (P[2 * r] >> 16) == (g.x >> 16);
      n += (P[2 * r + 1] & 0xffffu) == (g.y & 0xffffu);
      n += (P[2 * r + 1] >> 16) == (g.y >> 16);
    }
  });
  return n;
}

// One pw_step of one environment against the block in LDS; the environment is the caller's registers (P: packed positions, see
// SegLane; xy0: the agent's; goals_now: how many goal movables are on their goals).  Returns true when the positions changed.
// kNib: the block's wall tables are stop nibbles (the segment kernels), else bitmaps (pw_step_mseg_kernel).
template <int NP, int LPE, bool kNib>
__device__ __forceinline__ bool seg_step(const SegPuzzle& z, const SegLane<NP, LPE>& ln, uint32_t (&P)[NP / 2], uint32_t& xy0, int& goals_now,
                                         int& steps, int& term, int& trunc, double& reward, int& dgoals, const int act,
                                         const uint32_t flags, const int max_steps) {
  const bool do_reset = (flags & PW_STEP_AUTORESET) && (term | trunc) != 0;  // next-step autoreset: this step is the reset() of a finished episode
  const bool play = !do_reset && act <= 3;                                   // (else: not in Discrete(4), gym_env.py:195-196)
  const int dx = act == 0 ? -1 : (act == 1 ? 1 : 0);
  const int dy = act == 2 ? -1 : (act == 3 ? 1 : 0);
  const int Hs = z.Hs;

  // movable j at (x, y) is stopped by a wall: overlap after the move and none now (puzzle.py:522-564); two byte reads out of the
  // wall bitmaps (bit (x + 1) of row (y + 1))
  const uint32_t act2 = static_cast<uint32_t>(act) & 3u;
  auto wall_stops = [&](int j, int x, int y) -> bool {
    if constexpr (kNib) {
      // ONE byte read, no branch (the read of a position out of the table goes to byte 0 and is discarded): the loads of a pass --
      // this one, the object entry, the pair descriptors -- are issued together
      const uint32_t r2 = static_cast<uint32_t>(y + 2), c2 = static_cast<uint32_t>(x + 2);
      const bool in = r2 < static_cast<uint32_t>(Hs + 2) && c2 < static_cast<uint32_t>(z.wcols);
      const uint32_t at = __umul24(static_cast<uint32_t>(j), static_cast<uint32_t>(z.wper)) + __umul24(r2, static_cast<uint32_t>(z.wstride)) + (c2 >> 1);
      const uint32_t b = z.wall[in ? at : 0u];
      return ((in ? b : 0u) >> (4u * (c2 & 1u) + act2)) & 1u;
    }
    const uint32_t ws = static_cast<uint32_t>(z.wstride), wbits = 8u * ws;
    const uint8_t* t = z.wall + __umul24(ws, __umul24(static_cast<uint32_t>(j), static_cast<uint32_t>(Hs)));
    const int row = y + 1, bit = x + 1, rh = row + dy, bh = bit + dx;
    const bool in_h = static_cast<unsigned>(rh) < static_cast<unsigned>(Hs) && static_cast<unsigned>(bh) < wbits;
    const bool in_n = static_cast<unsigned>(row) < static_cast<unsigned>(Hs) && static_cast<unsigned>(bit) < wbits;
    const uint32_t bh_ = static_cast<uint32_t>(bh) & (wbits - 1u), bn_ = static_cast<uint32_t>(bit) & (wbits - 1u);
    const uint32_t th = t[__umul24(ws, static_cast<uint32_t>(min(max(rh, 0), Hs - 1))) + (bh_ >> 3)];
    const uint32_t tn = t[__umul24(ws, static_cast<uint32_t>(min(max(row, 0), Hs - 1))) + (bn_ >> 3)];
    return in_h && ((th >> (bh_ & 7u)) & 1u) != 0u && !(in_n && ((tn >> (bn_ & 7u)) & 1u) != 0u);
  };
  // bit j: the pusher with descriptor row `drow` and far corner (cbase, rbase) = (x + w, y + h) pushes movable j (puzzle.py:567-593).
  // Blocks of four pairs behind ONE wave-uniform test (rows are padded to NS descriptors: a padding pair, the agent and the pusher
  // itself find the one-byte zero table).  A lane looks at its first BPL register blocks; the masks meet in seg_group_or.
  auto pushes_of = [&](const uint32_t* drow, int cbase, int rbase) -> uint32_t {
    uint32_t m = 0;
    seg_blocks<0, NP / 4>(LPE == 1 ? z.NBu : z.BPL, [&](auto rc) {
      constexpr int r = decltype(rc)::value;
      const int jb = ln.jb_of(r, z.NB);
      const uint32_t dsc[4] = {drow[jb], drow[jb + 1], drow[jb + 2], drow[jb + 3]};
      uint32_t bits = 0;
#pragma unroll
      for (int jj = 0; jj < 4; jj++) {
        // (fields the byte-select forms of the instructions read in place: no extraction)
        const uint32_t off = dsc[jj] & 0xffffu, cm1 = (dsc[jj] >> 16) & 0xffu, rlim = dsc[jj] >> 24;
        const uint32_t xy = seg_xy<NP>(P, 4 * r + jj);
        const int xj = static_cast<int8_t>(xy & 0xff), yj = static_cast<int8_t>(xy >> 8);
        const uint32_t rr = min(static_cast<uint32_t>(rbase - yj), rlim);
        const uint32_t cc = min(static_cast<uint32_t>(cbase - xj), cm1);
        const uint32_t nib = z.tab[off + (__umul24(rr, cm1) + rr + cc)];
        bits |= ((nib >> act) & 1u) << jj;
      }
      m |= bits << jb;
    });
    return seg_group_or<LPE>(m) & z.jmask;
  };

  uint32_t pushed = 0;
  const int x0 = static_cast<int8_t>(xy0 & 0xff), y0 = static_cast<int8_t>(xy0 >> 8);
  // (the agent's wall test and its pass over the pairs do not depend on each other: both are issued, no branch between them -- a
  // wavefront is one dependent chain per step here, and some lane's agent is free to move in practically every step anyway)
  const bool stop0 = wall_stops(0, x0, y0);  // puzzle.py:353
  const uint32_t hits = pushes_of(z.pd, x0 + z.w0, y0 + z.h0);
  if (play && !stop0) {
    pushed = 1u | hits;
    uint32_t frontier = hits;
    bool blocked = false;
    // The push set is a fixed point of the CURRENT positions: "some member is stopped by a wall" does not depend on the order of
    // discovery (puzzle.py:361-382 aborts at the first one it meets).  ~15 % of the steps push anything.
    while (frontier != 0u && !blocked) {
      const uint32_t i = static_cast<uint32_t>(__ffs(static_cast<int>(frontier)) - 1);
      frontier &= frontier - 1u;
      // where movable i sits in THIS lane's registers: block (i / 4 - rot) mod NB
      uint32_t rb = (i >> 2);
      if constexpr (LPE > 1) {
        const int t = static_cast<int>(rb) - ln.rot;
        rb = static_cast<uint32_t>(t < 0 ? t + z.NB : t);
      }
      uint32_t pw;
      if (NP > 8 && z.NBu <= 2) {  // (wave-uniform: at most 8 movables -- a tree over four registers, not NP / 2)
        const uint32_t Q[4] = {P[0], P[1], P[2], P[3]};
        pw = seg_select<4>(Q, 2u * rb + ((i >> 1) & 1u));
      } else {
        pw = seg_select<NP / 2>(P, 2u * rb + ((i >> 1) & 1u));
      }
      const uint32_t xyi = (pw >> (16 * (i & 1u))) & 0xffffu;
      const int xi = static_cast<int8_t>(xyi & 0xff), yi = static_cast<int8_t>(xyi >> 8);
      blocked = wall_stops(static_cast<int>(i), xi, yi);
      const uint32_t oti = z.obj[i];
      const uint32_t next = pushes_of(z.pd + __umul24(i, static_cast<uint32_t>(z.NS)), xi + static_cast<int>(oti & 0xffu),
                                      yi + static_cast<int>((oti >> 8) & 0xffu));
      const uint32_t fresh = next & ~pushed;
      pushed |= fresh;
      frontier |= fresh;
    }
    if (blocked) pushed = 0u;
  }

  // displaced state (puzzle.py:384-394): bytewise add of (dx, dy) to the pushed movables, two per register
  const int before = goals_now;
  const uint32_t d16 = static_cast<uint32_t>(dx & 0xff) | (static_cast<uint32_t>(dy & 0xff) << 8);
  if (__ballot(pushed != 0u) != 0ull) {
    seg_blocks<0, NP / 4>(z.NBu, [&](auto rc) {
      constexpr int r = decltype(rc)::value;
      const uint32_t b4 = pushed >> ln.jb_of(r, z.NB);
#pragma unroll
      for (int k = 2 * r; k < 2 * r + 2; k++) {
        const uint32_t d = (((b4 >> (2 * (k - 2 * r))) & 1u) ? d16 : 0u) | (((b4 >> (2 * (k - 2 * r) + 1)) & 1u) ? d16 << 16 : 0u);
        P[k] = ((P[k] & 0x7f7f7f7fu) + (d & 0x7f7f7f7fu)) ^ ((P[k] ^ d) & 0x80808080u);
      }
    });
    const uint32_t d0 = (pushed & 1u) ? d16 : 0u;
    xy0 = (((xy0 & 0x7f7fu) + (d0 & 0x7f7fu)) ^ ((xy0 ^ d0) & 0x8080u)) & 0xffffu;
  }
  if (__builtin_expect(__ballot(do_reset) != 0ull, 0)) {  // (a few percent of the steps)
#pragma unroll
    for (int r = 0; r < NP / 4; r++) {
      uint2 v = make_uint2(0u, 0u);
      if (r < z.NBu && r < z.NB) {
        const uint32_t* ip = z.init + (ln.jb_of(r, z.NB) >> 1);
        v = make_uint2(ip[0], ip[1]);
      }
      P[2 * r] = do_reset ? v.x : P[2 * r];
      P[2 * r + 1] = do_reset ? v.y : P[2 * r + 1];
    }
    xy0 = do_reset ? (z.init[0] & 0xffffu) : xy0;
  }
  // goal bookkeeping (puzzle.py:396-411): the count before the step is the one the previous step (or the reset) left
  int after = before;
  if (__ballot(pushed > 1u) != 0ull) after = seg_goals<NP, LPE>(z, ln, P);  // (the agent is no goal movable: alone it changes nothing)
  after = do_reset ? z.init_goals : after;
  goals_now = after;
  const bool terminated = after == z.G;  // vacuously true without goals (trap T8)
  const int steps1 = steps + 1;
  steps = play ? steps1 : (do_reset ? 0 : steps);
  term = play ? (terminated ? 1 : 0) : (do_reset ? 0 : 0xFF);
  trunc = play ? ((max_steps >= 0 && steps1 >= max_steps) ? 1 : 0) : (do_reset ? 0 : 0xFF);
  const double rplay = terminated ? 10.0 : static_cast<double>(after - before) - 0.01;  // gym_env.py:212-221
  reward = play ? rplay : (do_reset ? 0.0 : reward);
  dgoals = play ? after - before : (do_reset ? 0 : dgoals);
  return pushed != 0u || do_reset;
}

// The steps of ONE environment per LPE lanes, once its puzzle's block is (being) copied into LDS and `z` points at it: loads the
// environment, runs the launch's steps, stores what pw_step / pw_rollout leave behind.  `z`'s sizes are wave-uniform in the segment
// kernels and per-lane values in the kernel of many puzzles per wavefront (pw_step_mseg_kernel): the same code, scalar or vector.
//   s_act / act_stride   this lane's column of the action tile in LDS (launches of several steps)
//   wg_barrier           the block was copied by the whole workgroup: wait for it (all threads of the workgroup are here)
template <int NP, bool kSingle, int LPE, bool kNib>
__device__ __forceinline__ void seg_run(const RolloutArgs& r, const SegPuzzle& z, const SegLane<NP, LPE>& ln, const int env, const bool live,
                                        const bool lead, const int pid, uint8_t* s_act, const int act_stride, const bool wg_barrier) {
  const StepArgs& a = r.s;
  const PwPuzzleHeader* h = a.hdrs + pid;
  // the environment (issued before the barrier: one memory level together with the table copy); rotated lanes load block by block
  uint32_t P[NP / 2];
  {
    const uint32_t* prow = reinterpret_cast<const uint32_t*>(a.pos) + static_cast<int64_t>(env) * (NP / 2);
    if constexpr (LPE == 1) {
      if constexpr (NP == 4) {
        const uint2 v = *reinterpret_cast<const uint2*>(prow);
        P[0] = v.x, P[1] = v.y;
      } else {
#pragma unroll
        for (int k = 0; k < NP / 8; k++) {
          const uint4 v = reinterpret_cast<const uint4*>(prow)[k];
          P[4 * k] = v.x, P[4 * k + 1] = v.y, P[4 * k + 2] = v.z, P[4 * k + 3] = v.w;
        }
      }
    } else {
#pragma unroll
      for (int rr = 0; rr < NP / 4; rr++) {
        uint2 v = make_uint2(0u, 0u);
        if (rr < z.NB) v = *reinterpret_cast<const uint2*>(prow + (ln.jb_of(rr, z.NB) >> 1));
        P[2 * rr] = v.x, P[2 * rr + 1] = v.y;
      }
    }
  }
  uint32_t xy0 = *reinterpret_cast<const uint16_t*>(a.pos + static_cast<int64_t>(env) * NP * 2);
  int steps = a.steps[env], term = a.term[env], trunc = a.trunc[env], dgoals = 0;
  double reward = 0.0;
  // the binding is a promise about puzzle_id (pw_batch_bind): an environment whose id has changed since is played on the puzzle
  // it was bound to, and counted
  if (lead && pw_clamp_pid(a.puzzle_id[env], a.num_puzzles) != pid) atomicAdd(a.bind_mismatch, 1u);
  const int n_steps = kSingle ? 1 : r.num_steps;
  auto load_action = [&](int t) { return t < n_steps ? static_cast<int>(a.actions[static_cast<int64_t>(t) * a.batch + env]) : 0; };
  // The actions of a launch of several steps travel through LDS, a tile of PW_SEG_ACT_TILE steps at a time: the loads of the NEXT
  // tile are issued when this one is written, so that nothing waits for them for a whole tile of steps.
  int R[PW_SEG_ACT_TILE];
#pragma unroll
  for (int u = 0; u < PW_SEG_ACT_TILE; u++) R[u] = (kSingle && u > 0) ? 0 : load_action(u);
  if (wg_barrier) __syncthreads();  // the block is in LDS
  int goals_now = seg_goals<NP, LPE>(z, ln, P);

  bool changed = false, any_played = false;
  uint32_t n_ended = 0, n_solved = 0;
  auto one_step = [&](const int t, const int act) {
    const bool was_done = (a.flags & PW_STEP_AUTORESET) && (term | trunc) != 0;
    // (rare paths are marked as such: the common path then falls through them -- a taken branch costs a wavefront that runs alone on
    // its SIMD an instruction-fetch restart, ~25 cycles: profiles/r06_bind_per_puzzle.txt, median 1.87 -> 1.62 us per step)
    if (__builtin_expect(__ballot(lead && act > 3 && !was_done) != 0ull, 0))
      if (lead && act > 3 && !was_done) atomicAdd(a.bad_actions, 1u);
    any_played = any_played || was_done || act <= 3;
    changed = seg_step<NP, LPE, kNib>(z, ln, P, xy0, goals_now, steps, term, trunc, reward, dgoals, act, a.flags, a.max_steps) || changed;
    n_ended += static_cast<uint32_t>(__popcll(__ballot(lead && term != 0xFF && (term | trunc) != 0)));
    n_solved += static_cast<uint32_t>(__popcll(__ballot(lead && term != 0xFF && term != 0)));
    if (!kSingle && (r.reward_hist || r.term_hist || r.trunc_hist)) {  // (one wave-uniform test for the three optional histories)
      if (lead) {
        const int64_t o = static_cast<int64_t>(t) * a.batch + env;
        if (r.reward_hist) r.reward_hist[o] = reward;
        if (r.term_hist) r.term_hist[o] = static_cast<uint8_t>(term);
        if (r.trunc_hist) r.trunc_hist[o] = static_cast<uint8_t>(trunc);
      }
    }
  };
  if constexpr (kSingle) {
    one_step(0, R[0]);
  } else {
    for (int tb = 0; tb < n_steps; tb += PW_SEG_ACT_TILE) {
#pragma unroll
      for (int u = 0; u < PW_SEG_ACT_TILE; u++) s_act[u * act_stride] = static_cast<uint8_t>(R[u]);
#pragma unroll
      for (int u = 0; u < PW_SEG_ACT_TILE; u++) R[u] = load_action(tb + PW_SEG_ACT_TILE + u);
      const int lim = min(PW_SEG_ACT_TILE, n_steps - tb);
      // (every lane reads back its own bytes only: no barrier; LDS accesses of a wavefront complete in order)
      int act = static_cast<int>(s_act[0]);
#pragma unroll 1
      for (int u = 0; u < lim; u++) {  // (the next step's action is read from LDS while this one runs)
        const int nxt = static_cast<int>(s_act[min(u + 1, PW_SEG_ACT_TILE - 1) * act_stride]);
        one_step(tb + u, act);
        act = nxt;
      }
    }
  }
  pw_count_add(a.counters, static_cast<uint32_t>(__popcll(__ballot(lead))) * static_cast<uint32_t>(n_steps), n_ended, n_solved);
  if (!lead) return;
  if (changed) {
    uint32_t* prow = reinterpret_cast<uint32_t*>(a.pos) + static_cast<int64_t>(env) * (NP / 2);
    if constexpr (NP == 4) {
      *reinterpret_cast<uint2*>(prow) = make_uint2(P[0], P[1]);
    } else {
#pragma unroll
      for (int k = 0; k < NP / 8; k++)
        reinterpret_cast<uint4*>(prow)[k] = make_uint4(P[4 * k], P[4 * k + 1], P[4 * k + 2], P[4 * k + 3]);
    }
  }
  if (a.rec) {  // page record of the NEW state for the page-ordered render of the same call (pw_step_render)
    uint64_t m = 0;
#pragma unroll
    for (int j = 0; j < NP; j++) {
      if (j < z.N) {  // (wave-uniform)
        const int y = static_cast<int8_t>(seg_xy<NP>(P, j) >> 8);
        const int hh = static_cast<int>((z.obj[j] >> 8) & 0xffu);
        if (static_cast<unsigned>(y) < 64u) m |= (hh >= 64 ? ~0ull : ((1ull << hh) - 1ull)) << y;
      }
    }
    PageRec rec;
    rec.pid = pid;
    rec.H = h->H;
    rec.W = h->W;
    rec.reserved = 0;
    rec.rows = m;
    a.rec[env] = rec;
    if (a.changed) {  // PW_OPT_OBS_CHANGED_PAGES: the rows in which the new state differs from what the retained buffer shows
      uint32_t* srow = reinterpret_cast<uint32_t*>(a.shown) + static_cast<int64_t>(env) * (NP / 2);
      uint32_t S[NP / 2];  // (loaded here, after the step: the single-step launch is bound by its registers)
      if constexpr (NP == 4) {
        const uint2 v = *reinterpret_cast<const uint2*>(srow);
        S[0] = v.x, S[1] = v.y;
      } else {
#pragma unroll
        for (int k = 0; k < NP / 8; k++) {
          const uint4 v = reinterpret_cast<const uint4*>(srow)[k];
          S[4 * k] = v.x, S[4 * k + 1] = v.y, S[4 * k + 2] = v.z, S[4 * k + 3] = v.w;
        }
      }
      uint64_t c = 0;
#pragma unroll
      for (int k = 0; k < NP / 2; k++) {
        if (2 * k < z.N && S[k] != P[k]) {
          c |= pw_shown_rows(S[k], P[k], static_cast<int>((z.obj[2 * k] >> 8) & 0xffu));
          if (2 * k + 1 < z.N) c |= pw_shown_rows(S[k] >> 16, P[k] >> 16, static_cast<int>((z.obj[2 * k + 1] >> 8) & 0xffu));
        }
      }
      a.changed[env] = c;
      if (c) {
        if constexpr (NP == 4) {
          *reinterpret_cast<uint2*>(srow) = make_uint2(P[0], P[1]);
        } else {
#pragma unroll
          for (int k = 0; k < NP / 8; k++)
            reinterpret_cast<uint4*>(srow)[k] = make_uint4(P[4 * k], P[4 * k + 1], P[4 * k + 2], P[4 * k + 3]);
        }
      }
    }
  }
  a.term[env] = static_cast<uint8_t>(term);
  a.trunc[env] = static_cast<uint8_t>(trunc);
  if (any_played) {
    a.steps[env] = steps;
    if (a.reward) a.reward[env] = reward;
    if (a.dgoals) a.dgoals[env] = static_cast<int8_t>(dgoals);
  }
}

// `z` over a block at `tab` described by `sd`
__device__ __forceinline__ void seg_puzzle(SegPuzzle& z, const uint8_t* tab, const PwSegDir& sd, const int lpe) {
  z.tab = tab;
  z.pd = reinterpret_cast<const uint32_t*>(tab);
  z.obj = reinterpret_cast<const uint32_t*>(tab + sd.obj_off);
  z.goal = reinterpret_cast<const uint16_t*>(tab + sd.goal_off);
  z.init = reinterpret_cast<const uint32_t*>(tab + sd.init_off);
  z.wall = tab + sd.wall_off;
  z.wstride = sd.wall_stride;
  z.wper = sd.wall_per;
  z.wcols = sd.wall_cols;
  z.N = sd.N;
  z.G = sd.G;
  z.NS = sd.NS;
  z.NB = sd.NS >> 2;
  z.Hs = sd.Hs;
  z.w0 = sd.w0h0 & 0xff;
  z.h0 = sd.w0h0 >> 8;
  z.init_goals = sd.init_goals;
  z.BPL = (z.NB + lpe - 1) / lpe;
  z.NBu = z.NB;
  z.jmask = sd.NS >= 32 ? ~0u : (1u << sd.NS) - 1u;
}

// The segment role of a launch: workgroup `seg` steps the environments of segment `seg` (all 256 threads must call it), LPE
// lanes per environment (256 / LPE environments per segment).
// kSingle: one step, no histories.
// s_tab: the launch's dynamic LDS (16-byte aligned; as large as the largest block among the bound puzzles).
template <int NP, bool kSingle, int LPE>
__device__ __forceinline__ void step_seg_lanes(const RolloutArgs& r, const PwSegDesc& d, const PwSegDir& sd, uint8_t* s_tab) {
  const StepArgs& a = r.s;
  {
    const uint4* src = reinterpret_cast<const uint4*>(a.ovl + sd.off);
    uint4* dst = reinterpret_cast<uint4*>(s_tab);
    for (uint32_t i = threadIdx.x; i < sd.bytes / 16u; i += PW_SEG_ENVS) dst[i] = src[i];
  }
  SegPuzzle z;
  seg_puzzle(z, s_tab, sd, LPE);
  SegLane<NP, LPE> ln;
  ln.q = static_cast<int>(threadIdx.x) & (LPE - 1);
  ln.rot = (ln.q * z.BPL) % z.NB;  // (< NB: LPE * BPL may exceed NB -- 5 blocks on 4 lanes: the last lane starts over at block 1)
  // SPREAD segments (bits 10 .. 12 of the flags): only the first 64 >> spread lanes of a wavefront carry environments.  A wavefront's
  // step lasts as long as its DEEPEST push chain: 0.1 .. 0.2 pushed movables per environment and step on average, but 3 .. 5 for the
  // worst of 64 environments, 1.2 .. 2.2 for the worst of 16 (DESIGN K1g) -- and a launch of many steps lasts as long as its slowest
  // wavefront.  Idle lanes cost nothing; the wavefronts they add run on SIMDs that have room.
  const int sp = (d.flags >> 10) & 7;
  const int lane = static_cast<int>(threadIdx.x) & (PW_WAVE - 1), wave = static_cast<int>(threadIdx.x) >> 6;
  const int li = (wave * (PW_WAVE >> sp) + lane) / LPE;
  const bool live = lane < (PW_WAVE >> sp) && li < d.count;
  const bool lead = live && ln.q == 0;  // the lane whose registers are in natural order: it stores
  int env = d.start + (live ? li : 0);
  if (!(d.flags & 1)) env = a.perm[env];
  uint8_t* s_act = s_tab + ((sd.bytes + 15u) & ~15u) + threadIdx.x;  // [PW_SEG_ACT_TILE][PW_SEG_ENVS] behind the block
  seg_run<NP, kSingle, LPE, !kSingle>(r, z, ln, env, live, lead, d.pid, s_act, PW_SEG_ENVS, true);
}

// (the lanes per environment of a segment: bits 8 .. 9 of its descriptor's flags = log2, chosen by pw_bind_plan_kernel)
template <int NP, bool kSingle>
__device__ __forceinline__ void step_seg_body(const RolloutArgs& r, const int seg, uint8_t* s_tab) {
  const PwSegDesc d = r.s.segs[seg];
  const PwSegDir& sd = kSingle ? d.dir0 : d.dir;  // (one step: the block with wall bitmaps; several: stop nibbles)
  const int lg = (d.flags >> 8) & 3;
  if constexpr (NP >= 32) {
    if (lg == 3) return step_seg_lanes<NP, kSingle, 8>(r, d, sd, s_tab);
  }
  if constexpr (NP >= 8) {
    if (lg == 2) return step_seg_lanes<NP, kSingle, 4>(r, d, sd, s_tab);
    if (lg == 1) return step_seg_lanes<NP, kSingle, 2>(r, d, sd, s_tab);
  }
  step_seg_lanes<NP, kSingle, 1>(r, d, sd, s_tab);
}

// a launch of segments only (batches whose every environment is bound; the A/B against the fused launches)
template <int NP, bool kSingle>
__global__ __launch_bounds__(PW_SEG_ENVS) void pw_step_seg_kernel(RolloutArgs r) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_seg_dyn[];
  if (static_cast<int>(blockIdx.x) >= r.s.bind_meta[0]) return;  // (the grid is an upper bound after an asynchronous re-bind)
  // A segment's wavefront is ONE dependent chain per step (a SIMD holds one of them); next to the lane groups of the same batch
  // (launches of several steps: the other stream's kernel, eight wavefronts per SIMD) it must not queue for the issue slot.
  __builtin_amdgcn_s_setprio(3);
  step_seg_body<NP, kSingle>(r, static_cast<int>(blockIdx.x), s_seg_dyn);
}

// Launches of several steps, the environments NO segment holds (puzzles played by fewer than min_envs environments: a C4 shard's
// Level-0 half, two per puzzle): one lane per environment all the same -- every lane copies ITS puzzle's block (~0.4 KB: up to
// 8 movables, PW_SEG_MULTI_BYTES at most) into its own slot of LDS, 64 puzzles per wavefront, and runs seg_run with per-lane sizes.
// 64 threads per workgroup (one wavefront: no barrier); bind_meta[5] environments in StepArgs::mlist; bind_meta[6] = the most LDS any
// wavefront's 64 blocks need (4-byte aligned blocks, hence element loads in seg_step).
#define PW_SEG_MULTI_BYTES 1008   // largest block that goes into a lane's slot.  Slots are an ODD number of dwords apart: the lanes of a wavefront
                                  // read the same offset of 64 different blocks -- consecutive banks, not eight lanes per bank (944-byte slots: 5.1 us
                                  // per step; see DESIGN K1g)
template <int NP>
__device__ __forceinline__ void step_mseg_body(const RolloutArgs& r, const int group, uint8_t* s_mseg_dyn) {  // (one wavefront: threads 0 .. 63)
  const StepArgs& a = r.s;
  const int n = a.bind_meta[5];
  const int per = PW_WAVE >> a.mseg_spread;  // (spread: see step_seg_lanes)
  const int first = group * per;
  if (first >= n) return;
  const int i = first + static_cast<int>(threadIdx.x);
  const bool live = static_cast<int>(threadIdx.x) < per && i < n;
  const int2 ep = reinterpret_cast<const int2*>(a.mlist)[live ? i : first];  // (environment, the puzzle it was bound to)
  const int env = ep.x, pid = ep.y;
  const PwSegDir sd = a.seg_dir[a.num_puzzles + pid];  // (the second half of the directory: the blocks with wall BITMAPS, at most PW_SEG_MULTI_BYTES)
  // the lane's slot: the blocks of the wavefront's 64 puzzles one behind the other (an exclusive scan of their sizes), each 4 bytes
  // further than its size -- an odd number of dwords between neighbouring lanes' blocks, whatever their sizes: the same offset of 64
  // blocks falls on consecutive banks
  const uint32_t mine = live ? sd.bytes + 4u : 0u;
  uint32_t incl = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t v = static_cast<uint32_t>(__shfl_up(static_cast<int>(incl), o, PW_WAVE));
    incl += static_cast<int>(threadIdx.x) >= o ? v : 0u;
  }
  uint8_t* tab = s_mseg_dyn + (incl - mine);
  {
    const uint4* src = reinterpret_cast<const uint4*>(a.ovl + sd.off);
    uint32_t* dst = reinterpret_cast<uint32_t*>(tab);  // (4-byte aligned)
    for (uint32_t k = 0; live && k < sd.bytes / 16u; k++) {
      const uint4 v = src[k];
      dst[4 * k] = v.x, dst[4 * k + 1] = v.y, dst[4 * k + 2] = v.z, dst[4 * k + 3] = v.w;
    }
  }
  SegPuzzle z;
  seg_puzzle(z, live ? tab : s_mseg_dyn, sd, 1);  // (a lane past the list shadows lane 0's block and stores nothing)
  z.NBu = __builtin_amdgcn_readfirstlane(__ballot(z.NB > 1) != 0ull ? 2 : 1);  // (blocks of at most 8 movables: one or two)
  SegLane<NP, 1> ln;
  ln.q = 0;
  ln.rot = 0;
  uint8_t* s_act = s_mseg_dyn + ((static_cast<uint32_t>(a.bind_meta[6]) + 15u) & ~15u) + threadIdx.x;
  seg_run<NP, false, 1, false>(r, z, ln, env, live, live, pid, s_act, 64, false);
}
template <int NP>
__global__ __launch_bounds__(64) void pw_step_mseg_kernel(RolloutArgs r) {
  extern __shared__ __attribute__((aligned(16))) uint8_t s_mseg_dyn[];
  __builtin_amdgcn_s_setprio(3);
  step_mseg_body<NP>(r, static_cast<int>(blockIdx.x), s_mseg_dyn);
}

// ------------------------------------------------------------------------------------
// pw_batch_bind on the device: three small kernels, no host round trip.
//   count   per environment: its puzzle's number of environments (the atomic's return value = the environment's rank among them),
//           lowest / highest environment index
//   plan    one workgroup over the puzzles: a puzzle with a block and at least min_envs environments is BOUND -- its segments
//           (ceil(count / 256)) get their descriptors; consecutive environments (batches sorted by puzzle: highest - lowest + 1 ==
//           count) need no index list, the others take a run of `perm`
//   fill    per environment: bound[e], and its slot of perm
// ------------------------------------------------------------------------------------
struct BindArgs {
  const int32_t* puzzle_id;
  const PwSegDir* seg_dir;
  int32_t* cnt;        // [P]
  int32_t* mn;         // [P]
  int32_t* mx;         // [P]
  int32_t* seg_base;   // [P]: first segment of the puzzle, -1 = not bound
  int32_t* perm_base;  // [P]: first perm slot, -1 = consecutive environments
  int32_t* rank;       // [B]
  int32_t* perm;       // [B]
  uint8_t* bound;      // [B]
  PwSegDesc* segs;     // [seg_cap]
  int32_t* meta;       // [0] segments, [1] bound environments, [2] bound puzzles, [3] of them with an index list, [4] bytes of the largest bound block,
                       // [5] environments in mlist, [6] bytes of a lane's slot for them (largest block, 16 x odd), [7] as [4] for the blocks with wall bitmaps
  int32_t* mlist;      // [B][2]: (environment, puzzle) of the environments no segment holds whose block fits a lane's slot (pw_step_mseg_kernel)
  int32_t batch, num_puzzles, min_envs, seg_cap;
  int32_t max_block;   // PW_OPT_BIND_MAX_KB: puzzles whose block exceeds this many bytes are not bound
  int32_t lanes_log2;  // PW_OPT_BIND_LANES: -1 automatic (by the puzzle's movables), else at most 2^this lanes per environment
  int32_t epw_log2;    // PW_OPT_BIND_SPREAD: a wavefront of a segment carries at most 64 >> this environments (lanes per environment and
                       // spread together)
  int32_t mepw_log2;   // ... and a wavefront of pw_step_mseg_kernel 64 >> this (0 .. 4)
};

__global__ __launch_bounds__(256) void pw_bind_count_kernel(BindArgs b) {
  // One atomic triple per RUN of equal puzzle ids inside a wavefront, not per environment: batches are mostly sorted by puzzle
  // (a C3 batch: 964 consecutive environments per puzzle -- 65 536 x 3 atomics on 68 addresses took 385 us), so a wavefront holds one
  // or two runs.  The run's first lane reserves `length` ranks and the others take theirs from it.
  const int e = blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & (PW_WAVE - 1);
  const bool in = e < b.batch;
  const int pid = in ? pw_clamp_pid(b.puzzle_id[e], b.num_puzzles) : -1;
  const bool bindable = in && b.seg_dir[pid].off != 0u;
  const int key = bindable ? pid : -1 - lane;  // (environments that are not counted never join a run)
  const int prev = __shfl_up(key, 1, PW_WAVE);
  const unsigned long long starts = __ballot(lane == 0 || key != prev);  // bit l: a run starts at lane l
  const int start = 63 - __clzll(starts & ((2ull << lane) - 1ull));        // this lane's run: first lane ...
  const unsigned long long above = lane == 63 ? 0ull : starts >> (lane + 1);
  const unsigned long long after = start == 63 ? 0ull : starts >> (start + 1);
  const int len = after ? __ffsll(after) : PW_WAVE - start;                  // ... and length
  (void)above;
  int base = 0;
  if (bindable && lane == start) {
    base = atomicAdd(&b.cnt[pid], len);
    atomicMin(&b.mn[pid], e);
    atomicMax(&b.mx[pid], e + len - 1);
  }
  base = __shfl(base, start, PW_WAVE);
  if (in) b.rank[e] = bindable ? base + (lane - start) : -1;
}

__global__ __launch_bounds__(1024) void pw_bind_plan_kernel(BindArgs b) {
  __shared__ int s_seg[1024], s_perm[1024];
  __shared__ int s_run[7];  // running totals: segments, perm slots, bound environments, bound puzzles, of them with an index list; [5] largest block, [6] ... in the bitmap form
  const int tid = threadIdx.x;
  if (tid < 7) s_run[tid] = 0;
  __syncthreads();
  for (int base = 0; base < b.num_puzzles; base += 1024) {
    const int p = base + tid;
    const int c = p < b.num_puzzles ? b.cnt[p] : 0;
    const bool ok = c >= b.min_envs && c > 0 && static_cast<int>(b.seg_dir[p].bytes) <= b.max_block;
    const bool contig = ok && (b.mx[p] - b.mn[p] + 1 == c);
    // lanes per environment: a step's latency grows with the movables (a pass of pair lookups per pushed movable), and a launch
    // lasts as long as its slowest segment -- the heavy puzzles' passes are shared by 2, 4 or (from 17 movables) 8 lanes: one block of
    // four pairs per lane and pass
    const int ns = ok ? static_cast<int>(b.seg_dir[p].NS) : 0;
    const int lg = b.lanes_log2 >= 0 ? (ns >= 8 ? min(b.lanes_log2, ns >= 20 ? 3 : (ns >= 16 ? 2 : 1)) : 0) : (ns >= 20 ? 3 : (ns >= 12 ? 2 : (ns >= 8 ? 1 : 0)));
    const int sp = max(0, min(b.epw_log2, 4) - lg);  // (at least 4 environments per wavefront)
    const int per_seg = PW_SEG_ENVS >> (lg + sp);
    const int nseg = ok ? (c + per_seg - 1) / per_seg : 0;
    const int nperm = (ok && !contig) ? c : 0;
    s_seg[tid] = nseg;
    s_perm[tid] = nperm;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {  // inclusive scans of both columns
      const int vs = tid >= o ? s_seg[tid - o] : 0, vp = tid >= o ? s_perm[tid - o] : 0;
      __syncthreads();
      s_seg[tid] += vs;
      s_perm[tid] += vp;
      __syncthreads();
    }
    const int seg0 = s_run[0] + s_seg[tid] - nseg, perm0 = s_run[1] + s_perm[tid] - nperm;
    if (p < b.num_puzzles) {
      b.seg_base[p] = ok ? seg0 : -1;
      b.perm_base[p] = nperm ? perm0 : -1;
      for (int k = 0; k < nseg && seg0 + k < b.seg_cap; k++) {
        PwSegDesc d;
        d.pid = p;
        d.start = (contig ? b.mn[p] : perm0) + k * per_seg;
        d.count = min(per_seg, c - k * per_seg);
        d.flags = (contig ? 1 : 0) | (lg << 8) | (sp << 10);
        d.dir = b.seg_dir[p];
        d.dir0 = b.seg_dir[b.num_puzzles + p];
        b.segs[seg0 + k] = d;
      }
    }
    if (ok) {
      atomicAdd(&s_run[2], c);
      atomicAdd(&s_run[3], 1);
      if (!contig) atomicAdd(&s_run[4], 1);
      atomicMax(&s_run[5], static_cast<int>(b.seg_dir[p].bytes));
      atomicMax(&s_run[6], static_cast<int>(b.seg_dir[b.num_puzzles + p].bytes));
    }
    __syncthreads();
    if (tid == 1023) {
      s_run[0] += s_seg[1023];
      s_run[1] += s_perm[1023];
    }
    __syncthreads();
  }
  if (tid == 0) {
    b.meta[0] = min(s_run[0], b.seg_cap);
    b.meta[1] = s_run[2];
    b.meta[2] = s_run[3];
    b.meta[3] = s_run[4];
    b.meta[4] = s_run[5];
    b.meta[7] = s_run[6];
    b.meta[5] = 0;  // (pw_bind_multi_kernel counts)
    b.meta[6] = 0;
  }
}

__global__ __launch_bounds__(256) void pw_bind_fill_kernel(BindArgs b) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= b.batch) return;
  const int pid = pw_clamp_pid(b.puzzle_id[e], b.num_puzzles);
  const int rk = b.rank[e];
  const bool is_bound = rk >= 0 && b.seg_base[pid] >= 0;
  b.bound[e] = is_bound ? 1 : 0;
  if (is_bound && b.perm_base[pid] >= 0) b.perm[b.perm_base[pid] + rk] = e;
}

// after the fill: the environments no segment holds whose puzzle has a small block (<= 8 movables, <= PW_SEG_MULTI_BYTES) are listed for
// pw_step_mseg_kernel -- one append per wavefront (ballot + prefix)
__global__ __launch_bounds__(256) void pw_bind_multi_kernel(BindArgs b) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  const int lane = threadIdx.x & (PW_WAVE - 1);
  const bool in = e < b.batch;
  const int pid = in ? pw_clamp_pid(b.puzzle_id[e], b.num_puzzles) : 0;
  uint32_t bytes = 0;
  bool take = false;
  if (in && !b.bound[e]) {
    const PwSegDir sd = b.seg_dir[b.num_puzzles + pid];  // (the bitmap form of the block)
    take = sd.off != 0u && sd.NS <= 8 && sd.bytes <= PW_SEG_MULTI_BYTES;
    bytes = take ? sd.bytes : 0u;
  }
  const unsigned long long m = __ballot(take);
  if (m == 0ull) return;
  int base = 0;
  if (lane == __ffsll(static_cast<long long>(m)) - 1) base = atomicAdd(&b.meta[5], __popcll(m));
  base = __shfl(base, __ffsll(static_cast<long long>(m)) - 1, PW_WAVE);
  if (take) {
    const int k = base + __popcll(m & ((1ull << lane) - 1ull));
    b.mlist[2 * k] = e;
    b.mlist[2 * k + 1] = pid;
  }
}

// ... and once the list is complete: the LDS a wavefront of pw_step_mseg_kernel needs = its 64 puzzles' blocks, 4 bytes apart; the
// launch carries the largest of them (bind_meta[6])
__global__ __launch_bounds__(256) void pw_bind_mslot_kernel(BindArgs b) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  uint32_t bytes = i < b.meta[5] ? b.seg_dir[b.num_puzzles + b.mlist[2 * i + 1]].bytes + 4u : 0u;
  const int per = PW_WAVE >> b.mepw_log2;  // environments per wavefront of pw_step_mseg_kernel
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t v = static_cast<uint32_t>(__shfl_xor(static_cast<int>(bytes), o, PW_WAVE));
    bytes += o < per ? v : 0u;
  }
  if ((threadIdx.x & (per - 1)) == 0 && bytes) atomicMax(&b.meta[6], static_cast<int>(bytes));
}

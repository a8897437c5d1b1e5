// pw_guide.inc -- K28: the cost-to-go tables DURING an episode.  pw_guide_step runs behind a step launch (and behind the pool
// draw) and leaves, per environment, the exact cost-to-go of the state the step left, its optimal / safe action bits, whether it
// is a dead end, the potential-shaped reward, and counts per puzzle of guided / optimal / dead-entering / unknown steps; with
// PW_GUIDE_END_DEAD it truncates an environment that has just entered a dead end.  Part of the single translation unit
// pw_kernels.hip (included there after pw_start_pool.inc: uses pw_solution_batch.inc's tables and check_launch).
//
// One launch, one lane per environment, no allocation, no wait, capturable.  The integers are exact; the shaped reward is
// computed with individually rounded operations (guide_shaped: nothing is contracted into a fused multiply-add), so it is the
// same double as the same expression evaluated on the host.
//
// The fused form is a chain of dependent loads -- puzzle id -> item -> (row_off, slot_off, slot_log2) -> slot -> key -> cost /
// acts -- with no arithmetic to hide behind, so what hides it is other wavefronts.  A workgroup is ONE wavefront: 65 536
// environments are 1 024 workgroups, four per CU, as 256-lane workgroups would be, but a batch of 4 096 spreads over 64 CUs
// instead of 16, and the counts are summed inside the wavefront without LDS or a barrier.
#define PW_GUIDE_THREADS 64
#define PW_GUIDE_FLAGS (PW_GUIDE_AUTORESET | PW_GUIDE_END_DEAD | PW_GUIDE_REFRESH)

struct GuideArgs {
  // the fused lookup, used when cost_in is NULL (num_puzzles is always set)
  SolveBatchTables t;
  // the applied form
  int32_t* cost_in;
  uint8_t* acts_in;  // or NULL
  // the environments
  const int32_t* puzzle_id;
  const int8_t* pos;
  const double* reward;  // or NULL (without shaped)
  const uint8_t* term;
  uint8_t* trunc;
  const uint8_t* mask;   // or NULL
  int32_t npad, n;
  // the guide
  int32_t* cost;
  uint8_t* acts;
  uint8_t* seen;
  uint8_t* dead;
  double* shaped;             // or NULL
  const int32_t* dead_cost;   // [P], or NULL (without shaped)
  double gamma, scale;
  unsigned long long* counts;    // [P][PW_GUIDE_COUNTS] or NULL
  unsigned long long* counters;  // the engine's pw_counters slots
  uint32_t flags;
};

// reward + F, F = gamma * phi(c) - phi(c_prev), phi(x) = -(scale * x), a dead end worth `dc`; F = 0 when `flat`.  Every operation
// is rounded on its own: contraction is switched off HERE -- hipcc contracts by default, and __dmul_rn / __dadd_rn are the plain
// operators in its headers, so they would be fused into one v_fma_f64 like any other product and sum.
__device__ __forceinline__ double guide_shaped(double reward, double gamma, double scale, int32_t c, int32_t c_prev, int32_t dc,
                                               bool flat) {
#pragma clang fp contract(off)
  double f = 0.0;
  if (!flat) {
    const double phi = -(scale * static_cast<double>(c == -1 ? dc : c));
    const double phi_prev = -(scale * static_cast<double>(c_prev == -1 ? dc : c_prev));
    f = gamma * phi - phi_prev;
  }
  return reward + f;
}

// count column k of the wavefront's lanes that raise `flag`: lanes of one puzzle (wave-uniform `p`) are summed first
__device__ __forceinline__ void guide_count(unsigned long long* counts, bool uniform, int32_t p, int k, bool flag, int lane) {
  if (uniform) {
    const unsigned long long m = __ballot(flag);
    if (m != 0ull && lane == __ffsll(m) - 1)
      atomicAdd(counts + static_cast<int64_t>(p) * PW_GUIDE_COUNTS + k, static_cast<unsigned long long>(__popcll(m)));
  } else if (flag) {
    atomicAdd(counts + static_cast<int64_t>(p) * PW_GUIDE_COUNTS + k, 1ull);
  }
}

__global__ __launch_bounds__(PW_GUIDE_THREADS) void pw_guide_step_kernel(GuideArgs a) {
  const int lane = threadIdx.x;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * PW_GUIDE_THREADS + lane;
  // (no early return: the ballots below want every lane of the wavefront)
  const bool live = i < a.n && !(a.mask && a.mask[i] == 0);
  int32_t p = -1, c = -2, c_prev = -2;
  uint32_t acts = 0u, t = 0u, u = 0u, was_seen = 0u;
  if (live) {
    p = a.puzzle_id[i];
    t = a.term[i];
    u = a.trunc[i];
    was_seen = a.seen[i];
    c_prev = a.cost[i];
    if (a.cost_in) {
      c = a.cost_in[i];
      if (a.acts_in) acts = a.acts_in[i];
      a.cost_in[i] = -2;  // behind the read: the next call's queries start clean
      if (a.acts_in) a.acts_in[i] = 0;
    } else {
      // pw_solve_batch_query's answer: cost -2 / acts 0 also for an id outside the set and a puzzle without a stored table
      int64_t base;
      const int64_t row = pw_sb_lookup(a.t, p, a.pos + i * a.npad * 2, a.npad, base);
      c = pw_sb_row_cost(a.t, base, row);
      acts = pw_sb_row_acts(a.t, base, row);
    }
  }
  const bool refresh = (a.flags & PW_GUIDE_REFRESH) != 0u;
  const bool fresh = (a.flags & PW_GUIDE_AUTORESET) && was_seen != 0u;
  const bool refused = t == 0xFFu;
  const bool cut = live && !refresh && (a.flags & PW_GUIDE_END_DEAD) && c == -1 && t == 0u && u == 0u && !fresh;
  if (cut) {
    a.trunc[i] = 1;
    u = 1u;
  }
  if (!refresh) {
    // pw_counters: a cut episode has ended (PW_PUSH_END_STUCK's rule), one add per wavefront
    const unsigned long long m = __ballot(cut);
    if (m != 0ull && lane == 0)
      atomicAdd(a.counters + (blockIdx.x & (PW_COUNTER_SLOTS - 1)) * 8u + 1, static_cast<unsigned long long>(__popcll(m)));
    if (live && a.shaped) {
      const int32_t dc = (p >= 0 && p < a.t.num_puzzles) ? a.dead_cost[p] : 0;
      a.shaped[i] = guide_shaped(a.reward[i], a.gamma, a.scale, c, c_prev, dc, fresh || refused || c == -2 || c_prev == -2);
    }
    if (a.counts) {
      const bool counted = live && p >= 0 && p < a.t.num_puzzles && !fresh && !refused;
      const bool guided = counted && c != -2 && c_prev != -2;
      // the counted lanes of a wavefront share a puzzle (bound batches are contiguous per puzzle): one add per column
      const unsigned long long cm = __ballot(counted);
      if (cm != 0ull) {
        const int32_t p0 = __shfl(p, __ffsll(cm) - 1, PW_WAVE);
        const bool uniform = __ballot(counted && p != p0) == 0ull;
        const int32_t pc = uniform ? p0 : p;
        guide_count(a.counts, uniform, pc, PW_GUIDE_GUIDED, guided, lane);
        guide_count(a.counts, uniform, pc, PW_GUIDE_OPTIMAL, guided && c_prev > 0 && c == c_prev - 1, lane);
        guide_count(a.counts, uniform, pc, PW_GUIDE_DEAD_ENTERED, guided && c == -1 && c_prev >= 0, lane);
        guide_count(a.counts, uniform, pc, PW_GUIDE_UNKNOWN, counted && c == -2, lane);
      }
    }
  }
  if (live) {
    a.cost[i] = c;
    a.acts[i] = static_cast<uint8_t>(acts);
    a.dead[i] = c == -1 ? 1 : 0;
    a.seen[i] = (t | u) != 0u ? 1 : 0;
  }
}

extern "C" {

int pw_guide_step(PwEngine* e, PwSolveBatch* tables, int32_t* cost_in, uint8_t* acts_in, const int32_t* puzzle_id,
                  const int8_t* pos, int32_t npad, const double* reward, const uint8_t* terminated, uint8_t* truncated,
                  const uint8_t* mask, int32_t n, int32_t* cost, uint8_t* acts, uint8_t* seen, uint8_t* dead, double* shaped,
                  const int32_t* dead_cost, double gamma, double scale, int64_t* counts, uint32_t flags, void* stream) try {
  if (!e) return pw_fail(PW_EINVAL, "pw_guide_step: null engine");
  if (tables && cost_in) return pw_fail(PW_EINVAL, "pw_guide_step: tables and cost_in are two sources: pass exactly one");
  if (!tables && !cost_in) return pw_fail(PW_EINVAL, "pw_guide_step: no source: pass tables or cost_in");
  if (acts_in && !cost_in) return pw_fail(PW_EINVAL, "pw_guide_step: acts_in goes with cost_in");
  if (!puzzle_id) return pw_fail(PW_EINVAL, "pw_guide_step: null puzzle_id");
  if (!pos) return pw_fail(PW_EINVAL, "pw_guide_step: null pos");
  if (!pw_npad_ok(npad)) return pw_fail(PW_EINVAL, "pw_guide_step: npad must be 4, 8, 16 or 32");
  if (!terminated) return pw_fail(PW_EINVAL, "pw_guide_step: null terminated");
  if (!truncated) return pw_fail(PW_EINVAL, "pw_guide_step: null truncated");
  if (n < 0) return pw_fail(PW_EINVAL, "pw_guide_step: n must be >= 0");
  if (!cost) return pw_fail(PW_EINVAL, "pw_guide_step: null cost");
  if (!acts) return pw_fail(PW_EINVAL, "pw_guide_step: null acts");
  if (!seen) return pw_fail(PW_EINVAL, "pw_guide_step: null seen");
  if (!dead) return pw_fail(PW_EINVAL, "pw_guide_step: null dead");
  if (shaped && !reward) return pw_fail(PW_EINVAL, "pw_guide_step: null reward with shaped");
  if (shaped && !dead_cost) return pw_fail(PW_EINVAL, "pw_guide_step: null dead_cost with shaped");
  if (flags & ~PW_GUIDE_FLAGS)
    return pw_fail(PW_EINVAL, "pw_guide_step: unknown flags (PW_GUIDE_AUTORESET / _END_DEAD / _REFRESH)");
  if (tables) {
    if (tables->eng != e) return pw_fail(PW_EINVAL, "pw_guide_step: tables belong to another engine");
    if (tables->n < 1) return pw_fail(PW_EINVAL, "pw_guide_step: tables: no run yet (call pw_solve_batch_run)");
  }
  if (n == 0) return PW_OK;
  PwDeviceGuard guard(e->set->device);
  GuideArgs a{};
  if (tables) a.t = solve_batch_tables(tables);
  a.t.num_puzzles = e->set->count;  // (also without tables: the range test of the counts)
  a.cost_in = cost_in;
  a.acts_in = acts_in;
  a.puzzle_id = puzzle_id;
  a.pos = pos;
  a.reward = reward;
  a.term = terminated;
  a.trunc = truncated;
  a.mask = mask;
  a.npad = npad;
  a.n = n;
  a.cost = cost;
  a.acts = acts;
  a.seen = seen;
  a.dead = dead;
  a.shaped = shaped;
  a.dead_cost = dead_cost;
  a.gamma = gamma;
  a.scale = scale;
  a.counts = reinterpret_cast<unsigned long long*>(counts);
  a.counters = e->d_counters;
  a.flags = flags;
  const dim3 grid(static_cast<unsigned>((static_cast<int64_t>(n) + PW_GUIDE_THREADS - 1) / PW_GUIDE_THREADS));
  hipLaunchKernelGGL(pw_guide_step_kernel, grid, dim3(PW_GUIDE_THREADS), 0, static_cast<hipStream_t>(stream), a);
  return check_launch("pw_guide_step");
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

}  // extern "C"

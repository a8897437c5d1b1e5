// pw_curriculum.inc -- K25: the level above the single puzzle, on the device.  Statistics per puzzle from the flags a step
// left (pw_episode_stats), sampling weights and their prefix sums from the statistics (pw_curriculum_update), and the weighted
// draw of the next puzzle of a finished environment (pw_resample_weighted).  Part of the single translation unit
// pw_kernels.hip (included there after pw_engine_step.inc: uses mix64, rebind_async and check_launch).
//
// Everything is integer arithmetic: the results are exact and independent of launch geometry and atomic order.  Every launch
// runs on the caller's stream, allocates nothing, never waits and can be captured.  No atomic returns a value (DESIGN K1f:
// returning atomics on one address are served one after the other).

// ------------------------------------------------------------------------------------------------------- statistics
// One lane per environment, 256 lanes per workgroup, workgroups striding over the batch.  In a typical step a few percent of the
// lanes contribute.
//   LDS form (the set has at most PW_STATS_LDS_PUZZLES puzzles, PW_OPT_STATS_LDS_PUZZLES): the workgroup sums its environments
//     into uint32 counters [P][PW_EPISODE_STATS] in LDS with ds atomics and then adds the non-zero ones to the caller's block, one
//     64-bit global atomic each.  A counter cannot overflow: the host gives a workgroup at most PW_STATS_GROUP_ENVS = 65 536
//     environments, and an environment adds at most PW_STATS_LDS_STEPS = 2^16 - 1 to one counter per call:
//     65 536 * 65 535 < 2^32.  An environment whose step count is outside 0 .. PW_STATS_LDS_STEPS (an engine without max_steps
//     after a long episode, or a caller's own array) adds to the block directly instead: the bound needs no promise from
//     anybody.
//   global form (larger sets): the contributing lanes add to the block directly.
// Which form and how many workgroups: DESIGN.md K25 has the measurements.
#define PW_STATS_LDS_PUZZLES 1024  // 16 KB of LDS per workgroup at most
#define PW_STATS_LDS_DEFAULT 256   // sets up to this size take the LDS form unless PW_OPT_STATS_LDS_PUZZLES says otherwise
#define PW_STATS_LDS_STEPS 65535
#define PW_STATS_GROUP_ENVS 65536

struct EpisodeStatsArgs {
  const int32_t* puzzle_id;
  const int32_t* steps;
  const uint8_t* term;
  const uint8_t* trunc;
  unsigned long long* stats;  // [P][PW_EPISODE_STATS]
  int32_t batch;
  int32_t num_puzzles;
};

__device__ __forceinline__ void stats_add_global(unsigned long long* row, bool solved, int32_t steps) {
  // (two's complement: a negative step count of a caller's own array subtracts, as the int64 sum of the definition does)
  const unsigned long long s = static_cast<unsigned long long>(static_cast<long long>(steps));
  atomicAdd(row + 0, 1ull);
  if (solved) atomicAdd(row + 1, 1ull);
  if (s) atomicAdd(row + 2, s);
  if (solved && s) atomicAdd(row + 3, s);
}

template <bool LDS>
__global__ __launch_bounds__(256) void pw_episode_stats_kernel(EpisodeStatsArgs a) {
  extern __shared__ uint32_t stats_lds[];  // LDS form: [num_puzzles][PW_EPISODE_STATS]
  const int words = a.num_puzzles * PW_EPISODE_STATS;
  bool any = false;  // this lane added to the LDS counters
  const int64_t stride = static_cast<int64_t>(gridDim.x) * 256;
  for (int64_t first = static_cast<int64_t>(blockIdx.x) * 256; first < a.batch; first += stride) {  // (uniform per workgroup)
    const int64_t env = first + threadIdx.x;
    bool live = false, solved = false;
    int32_t pid = 0, steps = 0;
    if (env < a.batch) {
      const uint32_t t = a.term[env], u = a.trunc[env];
      pid = a.puzzle_id[env];
      // (a refused action leaves 0xFF in both flags: no episode end, and the episode it abandons is not counted)
      live = (t | u) != 0 && t != 0xFFu && pid >= 0 && pid < a.num_puzzles;
      solved = t != 0;
      if (live) steps = a.steps[env];
    }
    if constexpr (LDS) {
      if (first == static_cast<int64_t>(blockIdx.x) * 256) {  // the first round: clear the counters
        for (int c = threadIdx.x; c < words; c += 256) stats_lds[c] = 0u;
        __syncthreads();
      }
      if (live && steps >= 0 && steps <= PW_STATS_LDS_STEPS) {
        uint32_t* row = stats_lds + pid * PW_EPISODE_STATS;
        atomicAdd(row + 0, 1u);
        if (solved) atomicAdd(row + 1, 1u);
        if (steps) atomicAdd(row + 2, static_cast<uint32_t>(steps));
        if (solved && steps) atomicAdd(row + 3, static_cast<uint32_t>(steps));
        any = true;
        live = false;
      }
    }
    if (live) stats_add_global(a.stats + static_cast<int64_t>(pid) * PW_EPISODE_STATS, solved, steps);
  }
  if constexpr (LDS) {
    if (!__syncthreads_or(any)) return;  // (uniform: nothing ended in this workgroup's environments; also the barrier before the flush)
    for (int c = threadIdx.x; c < words; c += 256) {
      const uint32_t v = stats_lds[c];
      if (v) atomicAdd(a.stats + c, static_cast<unsigned long long>(v));  // (the block has the layout of the LDS counters)
    }
  }
}

// ------------------------------------------------------------------------------------------------ weights and prefix sums
// ONE workgroup of 1024 lanes walks the set in tiles of 1024 puzzles: the weight of a lane's puzzle, an inclusive scan over the
// wavefront (shuffles), the sixteen wavefront totals through LDS, and a carry from tile to tile.  (The decoupled look-back scan
// was measured five times slower at this scale, DESIGN section 8; four puzzles per lane and tile were measured no faster than
// one -- the 64-bit division of a weight is what a tile takes, DESIGN K25.)
#define PW_CURRICULUM_THREADS 1024

struct CurriculumArgs {
  const long long* stats;  // [P][PW_EPISODE_STATS]
  const long long* base;   // or NULL
  const uint32_t* given;   // PW_CURRICULUM_GIVEN
  uint32_t* weights;       // or NULL
  unsigned long long* cdf;
  int32_t mode;
  uint32_t floor_q16;
  int32_t num_puzzles;
};

__device__ __forceinline__ uint32_t curriculum_weight(int32_t mode, long long n_in, long long s_in, uint32_t given,
                                                      uint32_t floor_q16) {
  uint64_t w;
  if (mode == PW_CURRICULUM_UNIFORM) {
    w = 65536u;
  } else if (mode == PW_CURRICULUM_GIVEN) {
    w = given;
  } else {
    const uint64_t n = n_in > 0 ? static_cast<uint64_t>(n_in) : 0u, s = s_in > 0 ? static_cast<uint64_t>(s_in) : 0u;
    const int bits = 64 - __clzll(static_cast<long long>(n));  // bit_length(n); 0 for n = 0
    const int k = bits > 20 ? bits - 20 : 0;
    const uint64_t n1 = n >> k;                         // < 2^20
    const uint64_t s1 = (s >> k) < n1 ? (s >> k) : n1;  // (a block with more solved than ended episodes is nobody's record: s' <= n')
    const uint64_t f1 = n1 - s1;
    if (mode == PW_CURRICULUM_FAILURE) w = (65536ull * (f1 + 1)) / (n1 + 2);
    else w = (262144ull * (s1 + 1) * (f1 + 1)) / ((n1 + 2) * (n1 + 2));  // the product stays below 2^61
  }
  return static_cast<uint32_t>(w > floor_q16 ? w : floor_q16);
}

__global__ __launch_bounds__(PW_CURRICULUM_THREADS) void pw_curriculum_update_kernel(CurriculumArgs a) {
  __shared__ unsigned long long wave_total[PW_CURRICULUM_THREADS / PW_WAVE];
  __shared__ unsigned long long carry_lds;
  const int tid = threadIdx.x, lane = tid & (PW_WAVE - 1), wave = tid >> 6;
  unsigned long long carry = 0;
  for (int first = 0; first < a.num_puzzles; first += PW_CURRICULUM_THREADS) {  // (uniform bounds: every lane takes every barrier)
    const int p = first + tid;
    unsigned long long x = 0;
    if (p < a.num_puzzles) {
      long long n = 0, s = 0;
      if (a.mode == PW_CURRICULUM_FAILURE || a.mode == PW_CURRICULUM_FRONTIER) {
        n = a.stats[static_cast<int64_t>(p) * PW_EPISODE_STATS + 0];
        s = a.stats[static_cast<int64_t>(p) * PW_EPISODE_STATS + 1];
        if (a.base) {
          // (a negative difference counts as 0: curriculum_weight clamps)
          n -= a.base[static_cast<int64_t>(p) * PW_EPISODE_STATS + 0];
          s -= a.base[static_cast<int64_t>(p) * PW_EPISODE_STATS + 1];
        }
      }
      const uint32_t w = curriculum_weight(a.mode, n, s, a.mode == PW_CURRICULUM_GIVEN ? a.given[p] : 0u, a.floor_q16);
      if (a.weights) a.weights[p] = w;
      x = w;
    }
    for (int o = 1; o < PW_WAVE; o <<= 1) {
      const unsigned long long y = __shfl_up(x, o, PW_WAVE);
      if (lane >= o) x += y;
    }
    if (lane == PW_WAVE - 1) wave_total[wave] = x;
    __syncthreads();
    unsigned long long before = carry;
    for (int v = 0; v < wave; v++) before += wave_total[v];
    if (p < a.num_puzzles) a.cdf[p] = before + x;
    if (tid == PW_CURRICULUM_THREADS - 1) carry_lds = before + x;
    __syncthreads();
    carry = carry_lds;
  }
}

// ------------------------------------------------------------------------------------------------------- weighted draw
// pw_resample_kernel's stream (episode += 1, r = mix64(seed, env, episode)); the puzzle is the smallest p with cdf[p] > t,
// t = mulhi64(r, cdf[P - 1]), found by a binary search that only the redrawn lanes run.
//   FENCE (PW_OPT_RESAMPLE_FENCE = 1; off by default, DESIGN.md K25 has the measurements): the workgroup first copies every ceil(P / 256)-th entry of the cdf into LDS (2 KB), a lane searches those and then the
//   one interval of the cdf between two of them: ceil(log2(ceil(P / 256))) dependent global loads instead of ceil(log2(P)).
//   A workgroup in which no lane draws returns before it loads anything.
#define PW_FENCE_ENTRIES 256

struct ResampleWeightedArgs {
  int32_t* puzzle_id;
  const uint8_t* term;
  const uint8_t* trunc;
  const unsigned long long* cdf;
  uint32_t* episode;
  uint64_t seed;
  int32_t num_puzzles;
  int32_t batch;
};

template <bool FENCE>
__global__ __launch_bounds__(256) void pw_resample_weighted_kernel(ResampleWeightedArgs a) {
  __shared__ unsigned long long fence[FENCE ? PW_FENCE_ENTRIES : 1];
  const int env = blockIdx.x * 256 + threadIdx.x;
  const bool done = env < a.batch && ((!a.term && !a.trunc) || (a.term && a.term[env]) || (a.trunc && a.trunc[env]));
  const int P = a.num_puzzles;
  const int stride = (P + PW_FENCE_ENTRIES - 1) / PW_FENCE_ENTRIES;  // cdf entries per fence interval
  if constexpr (FENCE) {
    if (!__syncthreads_or(done)) return;
    // fence[j] = the last entry of interval j (entries j * stride .. (j + 1) * stride - 1, cut at P; P - 1 once past the end)
    const int64_t last = static_cast<int64_t>(threadIdx.x + 1) * stride - 1;
    fence[threadIdx.x] = a.cdf[last < P ? last : P - 1];
    __syncthreads();
  }
  if (!done) return;
  const uint32_t ep = a.episode[env] + 1u;
  a.episode[env] = ep;
  const uint64_t r = mix64(a.seed, static_cast<uint64_t>(env), ep);
  const unsigned long long total = FENCE ? fence[PW_FENCE_ENTRIES - 1] : a.cdf[P - 1];
  if (total == 0) {  // no weight anywhere: uniform over the set, pw_resample's own draw
    a.puzzle_id[env] = static_cast<int32_t>(__umul64hi(r, static_cast<uint64_t>(P)));
    return;
  }
  const unsigned long long t = __umul64hi(r, total);  // t < total = cdf[P - 1]: the search below always ends inside the set
  int lo = 0, hi = P - 1;                            // the answer lies in lo .. hi and cdf[hi] > t
  if constexpr (FENCE) {
    int flo = 0, fhi = PW_FENCE_ENTRIES - 1;  // the smallest j with fence[j] > t
    while (flo < fhi) {
      const int mid = (flo + fhi) >> 1;
      if (fence[mid] > t) fhi = mid;
      else flo = mid + 1;
    }
    // (fence[flo] > t and fence[flo - 1] <= t: the answer is an entry of interval flo, whose last entry is known to exceed t)
    lo = flo * stride;
    hi = lo + stride - 1 < P - 1 ? lo + stride - 1 : P - 1;
    if (lo > hi) lo = hi;  // (never taken: the first interval that reaches P - 1 exceeds t, so flo * stride <= P - 1; keeps the loads in bounds)
  }
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a.cdf[mid] > t) hi = mid;
    else lo = mid + 1;
  }
  a.puzzle_id[env] = lo;
}

// ------------------------------------------------------------------------------------------------------------ host side
extern "C" {

int pw_episode_stats(PwEngine* e, const int32_t* puzzle_id, const int32_t* steps, const uint8_t* terminated,
                     const uint8_t* truncated, int64_t* stats, int32_t batch, void* stream) try {
  if (!e) return pw_fail(PW_EINVAL, "pw_episode_stats: null engine");
  if (!puzzle_id) return pw_fail(PW_EINVAL, "pw_episode_stats: null puzzle_id");
  if (!steps) return pw_fail(PW_EINVAL, "pw_episode_stats: null steps");
  if (!terminated) return pw_fail(PW_EINVAL, "pw_episode_stats: null terminated");
  if (!truncated) return pw_fail(PW_EINVAL, "pw_episode_stats: null truncated");
  if (!stats) return pw_fail(PW_EINVAL, "pw_episode_stats: null stats");
  if (batch < 0) return pw_fail(PW_EINVAL, "pw_episode_stats: batch must be >= 0");
  if (batch == 0) return PW_OK;
  PwDeviceGuard guard(e->set->device);
  const int P = e->set->count;
  EpisodeStatsArgs a{puzzle_id, steps, terminated, truncated, reinterpret_cast<unsigned long long*>(stats), batch, P};
  const int lds_puzzles = e->stats_lds_puzzles == 0 ? PW_STATS_LDS_DEFAULT : e->stats_lds_puzzles <= PW_STATS_LDS_PUZZLES ? e->stats_lds_puzzles : 0;
  const bool lds = P <= lds_puzzles;
  // one workgroup per 256 environments, at most PW_OPT_STATS_GROUPS (fewer workgroups merge more in LDS before they add to the
  // block: faster when every environment ends at once, slower in a typical step); never more than PW_STATS_GROUP_ENVS environments each
  int64_t groups = (static_cast<int64_t>(batch) + 255) / 256;
  if (e->stats_groups > 0) groups = std::min<int64_t>(groups, e->stats_groups);
  groups = std::max<int64_t>(groups, (static_cast<int64_t>(batch) + PW_STATS_GROUP_ENVS - 1) / PW_STATS_GROUP_ENVS);
  const dim3 grid(static_cast<unsigned>(groups)), block(256);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (lds)
    hipLaunchKernelGGL(pw_episode_stats_kernel<true>, grid, block, static_cast<size_t>(P) * PW_EPISODE_STATS * sizeof(uint32_t), st, a);
  else
    hipLaunchKernelGGL(pw_episode_stats_kernel<false>, grid, block, 0, st, a);
  return check_launch("pw_episode_stats");
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_curriculum_update(PwEngine* e, int32_t mode, const int64_t* stats, const int64_t* base, const uint32_t* given,
                         uint32_t floor_q16, uint32_t* weights, uint64_t* cdf, void* stream) try {
  if (!e) return pw_fail(PW_EINVAL, "pw_curriculum_update: null engine");
  if (mode < PW_CURRICULUM_UNIFORM || mode > PW_CURRICULUM_GIVEN)
    return pw_fail(PW_EINVAL, "pw_curriculum_update: unknown mode (PW_CURRICULUM_UNIFORM / _FAILURE / _FRONTIER / _GIVEN)");
  if (!stats && (mode == PW_CURRICULUM_FAILURE || mode == PW_CURRICULUM_FRONTIER))
    return pw_fail(PW_EINVAL, "pw_curriculum_update: null stats");
  if (!given && mode == PW_CURRICULUM_GIVEN) return pw_fail(PW_EINVAL, "pw_curriculum_update: null given with PW_CURRICULUM_GIVEN");
  if (!cdf) return pw_fail(PW_EINVAL, "pw_curriculum_update: null cdf");
  PwDeviceGuard guard(e->set->device);
  CurriculumArgs a{reinterpret_cast<const long long*>(stats), reinterpret_cast<const long long*>(base), given, weights,
                   reinterpret_cast<unsigned long long*>(cdf), mode, floor_q16, e->set->count};
  hipLaunchKernelGGL(pw_curriculum_update_kernel, dim3(1), dim3(PW_CURRICULUM_THREADS), 0, static_cast<hipStream_t>(stream), a);
  return check_launch("pw_curriculum_update");
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_resample_weighted(PwEngine* e, int32_t* puzzle_id, const uint8_t* terminated, const uint8_t* truncated,
                         const uint64_t* cdf, uint64_t seed, uint32_t* episode, int32_t batch, void* stream) try {
  if (!e) return pw_fail(PW_EINVAL, "pw_resample_weighted: null engine");
  if (!puzzle_id) return pw_fail(PW_EINVAL, "pw_resample_weighted: null puzzle_id");
  if (!cdf) return pw_fail(PW_EINVAL, "pw_resample_weighted: null cdf");
  if (!episode) return pw_fail(PW_EINVAL, "pw_resample_weighted: null episode");
  if (batch < 0) return pw_fail(PW_EINVAL, "pw_resample_weighted: batch must be >= 0");
  if (batch == 0 || e->set->count < 1) return PW_OK;
  PwDeviceGuard guard(e->set->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  ResampleWeightedArgs a{puzzle_id, terminated, truncated, reinterpret_cast<const unsigned long long*>(cdf), episode, seed,
                         e->set->count, batch};
  const dim3 grid(static_cast<unsigned>((static_cast<int64_t>(batch) + 255) / 256)), block(256);
  if (e->resample_fence == 1) hipLaunchKernelGGL(pw_resample_weighted_kernel<true>, grid, block, 0, st, a);
  else hipLaunchKernelGGL(pw_resample_weighted_kernel<false>, grid, block, 0, st, a);
  rebind_async(e, puzzle_id, batch, st);  // (as behind pw_resample: the ids of a bound buffer may have changed)
  return check_launch("pw_resample_weighted");
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

}  // extern "C"

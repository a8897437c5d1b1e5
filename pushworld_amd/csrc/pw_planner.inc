// ====================================================================================================
// Best-first planner (cpp/include/search/best_first_search.h:45-98, cpp/src/run_planner.cc:37-61) on the device.
// Included after pw_search.inc and pw_rgd.inc (one translation unit).
//
// The reference pops ONE state off a BucketPriorityQueue (priority_queue.h:150-226), expands it with the four actions of
// the next RandomActionIterator group and pushes every new successor under its heuristic cost.  Here a ROUND pops up to K
// states and expands them in one pw_search pass (search_pass: the same expand / claim / novelty / count / scan / publish
// kernels as the breadth-first search, given a parent list and the action groups), so the new states are numbered in
// (pop rank, position in the action group) order.  At K = 1 that is the reference's loop.  A round is:
//
//   pop       one workgroup: the lowest non-empty buckets from the device-held minimum, newest entries first, up to K of
//             them -> plist (store indices, -1 past the end) and the action group of each rank (pperm)
//   pass      search_pass over the K ranks: new states published after the store's end, the first goal in info[1]
//   finish    one lane: solved?  otherwise the round's new states are store indices [first, first + new)
//   unpack    new states -> int32 Position2D rows; pw_rgd_eval_kernel with the count in device memory
//   key       bucket of every new state (RGD: the integer cost; N+RGD: (novelty, cost)), +inf and NaN after the finite ones
//   sort      rocprim radix sort of (bucket, store index) over the K * 4 slots (padding sorts last): stable, so the
//             states of one bucket stay in store order
//   segment   each run of one bucket in the sorted round becomes a SEGMENT pushed onto that bucket's stack; the entries
//             array holds the sorted store indices at positions [first, first + new) (every state is pushed once)
//
// Queue (all O(max_states) or O(buckets), allocated by pw_planner_create):
//   head      int32 [B]        top segment of bucket b, -1 = empty
//   seg_*     int32 [max]      (start, length, next) of the segment that starts at entries position p (ids are positions)
//   ent       int32 [max]      store indices, sorted by bucket within each round
//   bits0/1/2 uint64           occupancy: bit b of level 0 = bucket b non-empty; bit w of level 1 = word w of level 0 != 0;
//                              level 2 likewise over level 1.  The lowest non-empty bucket >= b costs at most three words
//                              plus a scan of level 2 (<= 17 words).
// Every kernel of this file and of the search pass returns at once when the status word info[0] is not 0 (done), so the
// host enqueues rounds in groups and reads the status once per group: whatever the group size, the device does the same
// rounds.  The rocPRIM sort cannot read the status word: in the rounds of a group left after the end it still sorts the
// 4 K (stale) keys, whose result the segment kernel then ignores.
// ====================================================================================================
#include <random>

#include <rocprim/device/device_radix_sort.hpp>

#define PW_PLAN_ERANGE 4  // internal status: a finite key outside the bucket range (pw_planner_run returns PW_ELIMIT)

enum PlanSlot {
  kPStatus = 0, kPRounds, kPExpanded, kPVisited, kPOpen, kPGoal, kPFirst, kPNew, kPMin, kPMaxKey, kPRangeKey, kPSlots = 16
};

static constexpr int kPlanGroups = 1000;         // RandomActionIterator's default number of action groups
static constexpr uint32_t kPlanPad = (1u << 23) - 1u;  // sort key of the padding slots (above every bucket)
static constexpr int kPlanSortBits = 23;
static constexpr uint32_t kPlanRgdBuckets = 1u << 22;  // RGD mode: finite costs 0 .. 2^22 - 1
static constexpr uint32_t kPlanNrgdRange = 1000000u;   // N+RGD: finite costs 0 .. 999 999 per novelty (key = n * 1e6 + cost)
static constexpr int kPlanSyncRounds = 16;             // default rounds enqueued per status read

struct BfsPlanQueue {
  int32_t* head;
  unsigned long long* bits0;
  unsigned long long* bits1;
  unsigned long long* bits2;
  int32_t* seg_start;
  int32_t* seg_len;
  int32_t* seg_next;
  int32_t* ent;
  uint32_t nb;  // buckets: finite ones, then +inf (nb - 2), NaN (nb - 1)
  uint32_t n0, n1, n2;  // words per bitmap level
};

struct BfsPlanArgs {
  unsigned long long* info;         // [kPSlots] (PlanSlot)
  const unsigned long long* sinfo;  // the search's [0] store size, [1] lowest goal index
  BfsPlanQueue q;
  int32_t* plist;
  uint8_t* pperm;
  const uint8_t* groups;  // [kPlanGroups] packed action groups, or NULL (fixed order L R U D)
  int32_t* rsrc;          // [K] pop ranges: one past the newest entry taken, length, first output rank
  int32_t* rlen;
  int32_t* roff;
  int32_t K;
  int32_t mode;
  int64_t max_states;
  const uint32_t* states;  // packed store
  int32_t nw, N;
  int32_t* rows;           // [4 K][N] Position2D of the round's new states
  const float* cost;       // [4 K]
  const uint8_t* state_nov;  // [max_states] (N+RGD)
  uint32_t* keys;          // [4 K] sort in / out
  int32_t* vals;
  const uint32_t* skeys;
  const int32_t* svals;
};

// ---- occupancy bitmap ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t plan_first_at(const BfsPlanQueue& q, uint32_t w1) {  // w1: a non-zero level-1 word
  const uint32_t w0 = (w1 << 6) + static_cast<uint32_t>(__ffsll(static_cast<long long>(q.bits1[w1])) - 1);
  return (w0 << 6) + static_cast<uint32_t>(__ffsll(static_cast<long long>(q.bits0[w0])) - 1);
}

// lowest non-empty bucket >= b, q.nb when there is none
__device__ uint32_t plan_next(const BfsPlanQueue& q, uint32_t b) {
  const uint32_t w0 = b >> 6;
  if (w0 >= q.n0) return q.nb;
  unsigned long long m = q.bits0[w0] & (~0ull << (b & 63u));
  if (m) return (w0 << 6) + static_cast<uint32_t>(__ffsll(static_cast<long long>(m)) - 1);
  const uint32_t c1 = w0 + 1;  // first level-0 word still to look at
  if (c1 >= q.n0) return q.nb;
  const uint32_t w1 = c1 >> 6;
  m = q.bits1[w1] & (~0ull << (c1 & 63u));
  if (m) {
    const uint32_t v0 = (w1 << 6) + static_cast<uint32_t>(__ffsll(static_cast<long long>(m)) - 1);
    return (v0 << 6) + static_cast<uint32_t>(__ffsll(static_cast<long long>(q.bits0[v0])) - 1);
  }
  const uint32_t c2 = w1 + 1;  // first level-1 word still to look at
  for (uint32_t w2 = c2 >> 6; w2 < q.n2 && c2 < q.n1; w2++) {
    m = q.bits2[w2];
    if (w2 == (c2 >> 6)) m &= ~0ull << (c2 & 63u);
    if (m) return plan_first_at(q, (w2 << 6) + static_cast<uint32_t>(__ffsll(static_cast<long long>(m)) - 1));
  }
  return q.nb;
}

__device__ __forceinline__ void plan_clear(const BfsPlanQueue& q, uint32_t b) {
  const uint32_t w0 = b >> 6, w1 = w0 >> 6, w2 = w1 >> 6;
  if ((q.bits0[w0] &= ~(1ull << (b & 63u))) != 0ull) return;
  if ((q.bits1[w1] &= ~(1ull << (w0 & 63u))) != 0ull) return;
  q.bits2[w2] &= ~(1ull << (w1 & 63u));
}

__device__ __forceinline__ void plan_set(const BfsPlanQueue& q, uint32_t b) {
  const uint32_t w0 = b >> 6, w1 = w0 >> 6, w2 = w1 >> 6;
  atomicOr(&q.bits0[w0], 1ull << (b & 63u));
  atomicOr(&q.bits1[w1], 1ull << (w0 & 63u));
  atomicOr(&q.bits2[w2], 1ull << (w1 & 63u));
}

// ---- pop: up to K entries, lowest bucket first, newest first within a bucket ---------------------------------------
__global__ __launch_bounds__(256) void pw_planner_pop_kernel(BfsPlanArgs a) {
  __shared__ int s_n, s_nr;
  __shared__ unsigned long long s_pbase;
  if (threadIdx.x == 0) {
    int n = -1, nr = 0;
    unsigned long long pbase = 0;
    if (a.info[kPStatus] == 0) {
      n = 0;
      const unsigned long long stored = a.sinfo[0];
      const unsigned long long open = a.info[kPOpen];
      if (stored + 4ull * static_cast<unsigned long long>(a.K) > static_cast<unsigned long long>(a.max_states)) {
        a.info[kPStatus] = PW_PLAN_LIMIT;
      } else if (open == 0) {
        a.info[kPStatus] = PW_PLAN_EXHAUSTED;
      } else {
        const int want = static_cast<int>(open < static_cast<unsigned long long>(a.K) ? open : a.K);
        uint32_t b = plan_next(a.q, static_cast<uint32_t>(a.info[kPMin]));
        while (n < want && b < a.q.nb) {
          const int32_t sg = a.q.head[b];
          if (sg < 0) {  // (cannot happen: the occupancy bits follow the heads)
            plan_clear(a.q, b);
            b = plan_next(a.q, b + 1);
            continue;
          }
          const int32_t len = a.q.seg_len[sg];
          const int t = min(want - n, len);
          a.rsrc[nr] = a.q.seg_start[sg] + len;
          a.rlen[nr] = t;
          a.roff[nr] = n;
          nr++;
          n += t;
          if (t < len) {
            a.q.seg_len[sg] = len - t;
          } else {
            const int32_t next = a.q.seg_next[sg];
            a.q.head[b] = next;
            if (next < 0) {
              plan_clear(a.q, b);
              if (n < want) b = plan_next(a.q, b + 1);
            }
          }
        }
        pbase = a.info[kPExpanded];
        a.info[kPMin] = b;
        a.info[kPOpen] = open - static_cast<unsigned long long>(n);
        a.info[kPExpanded] = pbase + static_cast<unsigned long long>(n);
        a.info[kPRounds] += 1;
        a.info[kPFirst] = stored;
      }
    }
    s_n = n;
    s_nr = nr;
    s_pbase = pbase;
  }
  __syncthreads();
  const int n = s_n, nr = s_nr;
  if (n < 0) return;  // done before this round
  for (int o = threadIdx.x; o < a.K; o += blockDim.x) {
    int32_t v = -1;
    uint8_t perm = 0xE4u;  // L R U D
    if (o < n) {
      int lo = 0, hi = nr - 1;  // the last range that starts at or before rank o
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.roff[mid] <= o) lo = mid;
        else hi = mid - 1;
      }
      v = a.q.ent[a.rsrc[lo] - 1 - (o - a.roff[lo])];
      // RandomActionIterator::next() advances before it returns: global pop p takes group (p + 1) mod 1000
      if (a.groups) perm = a.groups[(s_pbase + static_cast<unsigned long long>(o) + 1ull) % kPlanGroups];
    }
    a.plist[o] = v;
    a.pperm[o] = perm;
  }
}

// ---- finish: goal, visited count, the round's new states ------------------------------------------------------------
__global__ void pw_planner_finish_kernel(BfsPlanArgs a) {
  if (a.info[kPStatus]) return;
  const unsigned long long goal = a.sinfo[1], stored = a.sinfo[0];
  if (goal != ~0ull) {  // the first goal in candidate order: everything numbered before it was visited
    a.info[kPStatus] = PW_PLAN_SOLVED;
    a.info[kPGoal] = goal;
    a.info[kPVisited] = goal;
    a.info[kPNew] = 0;
  } else {
    a.info[kPVisited] = stored;
    a.info[kPNew] = stored - a.info[kPFirst];
  }
}

__global__ __launch_bounds__(256) void pw_planner_unpack_kernel(BfsPlanArgs a) {
  if (a.info[kPStatus]) return;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  const int64_t n = static_cast<int64_t>(a.info[kPNew]);
  if (i >= n * a.N) return;
  const int64_t s = i / a.N;
  const int j = static_cast<int>(i - s * a.N);
  const int64_t idx = static_cast<int64_t>(a.info[kPFirst]) + s;
  const uint32_t xy = reinterpret_cast<const uint16_t*>(a.states + idx * a.nw)[j];
  a.rows[i] = static_cast<int32_t>(xy & 0xffu) * PW_POSITION_LIMIT + static_cast<int32_t>(xy >> 8);
}

// ---- key: bucket of every new state; the padding slots sort last -----------------------------------------------------
__global__ __launch_bounds__(256) void pw_planner_key_kernel(BfsPlanArgs a) {
  if (a.info[kPStatus]) return;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (i >= 4ll * a.K) return;
  const int64_t n = static_cast<int64_t>(a.info[kPNew]);
  if (i >= n) {
    a.keys[i] = kPlanPad;
    a.vals[i] = -1;
    return;
  }
  const float r = a.cost[i];
  uint32_t b;
  float key;
  if (r != r) {
    b = a.q.nb - 1;  // NaN: an RGD budget overrun
    key = r;
  } else if (a.mode == PW_PLAN_N_RGD) {
    const uint32_t nov = a.state_nov[a.info[kPFirst] + i];
    key = static_cast<float>(static_cast<float>(nov) * 1e6f) + r * 1.0f;  // WeightedSumHeuristic, weighted_sum.cc:37-48
    if (isinf(key)) {
      b = a.q.nb - 2;
    } else if (r >= static_cast<float>(kPlanNrgdRange) || nov < 1 || nov > 3) {
      b = a.q.nb - 2;
      atomicMax(&a.info[kPRangeKey], static_cast<unsigned long long>(__float_as_uint(r)) + 1ull);
      a.info[kPStatus] = PW_PLAN_ERANGE;
    } else {
      b = (nov - 1) * kPlanNrgdRange + static_cast<uint32_t>(r);
    }
  } else {
    key = r;
    if (isinf(r)) {
      b = a.q.nb - 2;
    } else if (r >= static_cast<float>(kPlanRgdBuckets)) {
      b = a.q.nb - 2;
      atomicMax(&a.info[kPRangeKey], static_cast<unsigned long long>(__float_as_uint(r)) + 1ull);
      a.info[kPStatus] = PW_PLAN_ERANGE;
    } else {
      b = static_cast<uint32_t>(r);
    }
  }
  if (key == key && !isinf(key)) atomicMax(&a.info[kPMaxKey], static_cast<unsigned long long>(__float_as_uint(key)));
  a.keys[i] = b;
  a.vals[i] = static_cast<int32_t>(a.info[kPFirst] + i);
}

// ---- segment: each run of one bucket in the sorted round goes on top of that bucket's stack ---------------------------
__global__ __launch_bounds__(256) void pw_planner_segment_kernel(BfsPlanArgs a) {
  if (a.info[kPStatus]) return;
  const int64_t p = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  const int64_t n = static_cast<int64_t>(a.info[kPNew]);
  if (p >= n) return;
  const int64_t first = static_cast<int64_t>(a.info[kPFirst]);
  const uint32_t b = a.skeys[p];
  a.q.ent[first + p] = a.svals[p];
  if (p == 0) atomicAdd(&a.info[kPOpen], static_cast<unsigned long long>(n));
  if (p > 0 && a.skeys[p - 1] == b) return;
  int64_t lo = p + 1, hi = n;  // the end of the run: first position with a larger bucket
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (a.skeys[mid] == b) lo = mid + 1;
    else hi = mid;
  }
  const int32_t seg = static_cast<int32_t>(first + p);
  a.q.seg_start[seg] = seg;
  a.q.seg_len[seg] = static_cast<int32_t>(lo - p);
  a.q.seg_next[seg] = a.q.head[b];
  a.q.head[b] = seg;
  plan_set(a.q, b);
  atomicMin(&a.info[kPMin], static_cast<unsigned long long>(b));
}

// ---- host ---------------------------------------------------------------------------------------------------------
struct PwPlanner {
  PwEngine* eng;
  int32_t puzzle;
  int32_t mode, K, flags;
  int64_t max_states;
  PwSearch* s;   // store, closed set, candidates (chunk = K); in N+RGD mode also its novelty tables
  PwRgd* rgd;
  BfsPlanQueue q;
  unsigned long long* d_info;
  int32_t* d_plist;
  uint8_t* d_pperm;
  uint8_t* d_groups;
  int32_t* d_rsrc;
  int32_t* d_rlen;
  int32_t* d_roff;
  int32_t* d_rows;
  float* d_cost;
  uint8_t* d_state_nov;
  uint32_t* d_keys[2];
  int32_t* d_vals[2];
  void* d_sort_tmp;
  size_t sort_tmp_bytes;
  int32_t sync_rounds;
  bool begun;
  int64_t status;
};

static void plan_action_groups(uint8_t* out) {  // RandomActionIterator(1000): random_action_iterator.cc
  std::default_random_engine rng(42);
  for (int g = 0; g < kPlanGroups; g++) {
    std::vector<int> grp = {0, 1, 2, 3};
    std::shuffle(grp.begin(), grp.end(), rng);
    for (int k = 0; k < 4; k++) out[4 * g + k] = static_cast<uint8_t>(grp[static_cast<size_t>(k)]);
  }
}

// the groups packed two bits per action, on the device (kPlanGroups bytes)
static hipError_t plan_upload_groups(uint8_t* d_groups) {
  uint8_t packed[kPlanGroups];
  uint8_t raw[4 * kPlanGroups];
  plan_action_groups(raw);
  for (int g = 0; g < kPlanGroups; g++)
    packed[g] = static_cast<uint8_t>(raw[4 * g] | (raw[4 * g + 1] << 2) | (raw[4 * g + 2] << 4) | (raw[4 * g + 3] << 6));
  return hipMemcpy(d_groups, packed, kPlanGroups, hipMemcpyHostToDevice);
}

static BfsPlanArgs plan_args(PwPlanner* p) {
  BfsPlanArgs a;
  a.info = p->d_info;
  a.sinfo = p->s->d_info;
  a.q = p->q;
  a.plist = p->d_plist;
  a.pperm = p->d_pperm;
  a.groups = (p->flags & PW_PLAN_ACTIONS_FIXED) ? nullptr : p->d_groups;
  a.rsrc = p->d_rsrc;
  a.rlen = p->d_rlen;
  a.roff = p->d_roff;
  a.K = p->K;
  a.mode = p->mode;
  a.max_states = p->max_states;
  a.states = p->s->d_states;
  a.nw = p->s->NW;
  a.N = p->s->N;
  a.rows = p->d_rows;
  a.cost = p->d_cost;
  a.state_nov = p->d_state_nov;
  a.keys = p->d_keys[0];
  a.vals = p->d_vals[0];
  a.skeys = p->d_keys[1];
  a.svals = p->d_vals[1];
  return a;
}

// score and push the states [info[kPFirst], + info[kPNew]) (unpack, RGD, key, sort, segment)
static int plan_push(PwPlanner* p, hipStream_t st) {
  const BfsPlanArgs a = plan_args(p);
  const int64_t slots = 4ll * p->K;
  hipLaunchKernelGGL(pw_planner_unpack_kernel, dim3(static_cast<unsigned>((slots * p->s->N + 255) / 256)), dim3(256), 0, st, a);
  RgdEvalArgs r = rgd_eval_args(p->rgd, p->d_rows, p->d_cost, static_cast<int32_t>(slots));
  r.dcount = p->d_info + kPNew;
  r.halt = p->d_info + kPStatus;
  hipLaunchKernelGGL(pw_rgd_eval_kernel, dim3(static_cast<unsigned>((slots + PW_WAVE - 1) / PW_WAVE)), dim3(PW_WAVE),
                     rgd_eval_lds(p->rgd), st, r);
  const unsigned kblocks = static_cast<unsigned>((slots + 255) / 256);
  hipLaunchKernelGGL(pw_planner_key_kernel, dim3(kblocks), dim3(256), 0, st, a);
  size_t tmp = p->sort_tmp_bytes;
  const hipError_t err = rocprim::radix_sort_pairs(p->d_sort_tmp, tmp, p->d_keys[0], p->d_keys[1], p->d_vals[0], p->d_vals[1],
                                                   static_cast<size_t>(slots), 0, kPlanSortBits, st);
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string("pw_planner: radix sort: ") + hipGetErrorString(err));
  hipLaunchKernelGGL(pw_planner_segment_kernel, dim3(kblocks), dim3(256), 0, st, a);
  return check_launch("pw_planner");
}

extern "C" {

void pw_planner_destroy(PwPlanner* p) {
  if (!p) return;
  void* bufs[] = {p->q.head, p->q.bits0, p->q.bits1, p->q.bits2, p->q.seg_start, p->q.seg_len, p->q.seg_next, p->q.ent,
                  p->d_info, p->d_plist, p->d_pperm, p->d_groups, p->d_rsrc, p->d_rlen, p->d_roff, p->d_rows, p->d_cost,
                  p->d_state_nov, p->d_keys[0], p->d_keys[1], p->d_vals[0], p->d_vals[1], p->d_sort_tmp};
  for (void* b : bufs)
    if (b) (void)hipFree(b);
  pw_search_destroy(p->s);
  pw_rgd_destroy(p->rgd);
  delete p;
}

int pw_planner_action_groups(uint8_t* out) try {
  if (!out) return pw_fail(PW_EINVAL, "null argument");
  plan_action_groups(out);
  return kPlanGroups;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_planner_create(PwEngine* e, int32_t puzzle, int32_t mode, int64_t max_states, int32_t batch, int32_t flags,
                      int64_t rgd_budget, PwPlanner** out) try {
  // (the argument checks come first: they need no engine)
  if (mode != PW_PLAN_RGD && mode != PW_PLAN_N_RGD) return pw_fail(PW_EINVAL, "mode must be PW_PLAN_RGD (0) or PW_PLAN_N_RGD (1)");
  if (batch < 1 || batch > (1 << 24)) return pw_fail(PW_EINVAL, "batch (K) must be in 1 .. 2^24");
  if (flags != PW_PLAN_ACTIONS_REFERENCE && flags != PW_PLAN_ACTIONS_FIXED)
    return pw_fail(PW_EINVAL, "flags must be PW_PLAN_ACTIONS_REFERENCE (0) or PW_PLAN_ACTIONS_FIXED (1)");
  if (rgd_budget < 0) return pw_fail(PW_EINVAL, "rgd_budget must be >= 0 (0 = the default)");
  if (max_states < 4ll * batch + 1) return pw_fail(PW_EINVAL, "max_states must be at least 4 * batch + 1");
  if (max_states > (1ll << 30)) return pw_fail(PW_EINVAL, "max_states must be at most 2^30");
  if (!e || !out) return pw_fail(PW_EINVAL, "null argument");
  *out = nullptr;
  if (puzzle < 0 || puzzle >= e->set->count) return pw_fail(PW_EINVAL, "puzzle index out of range");
  PwPlanner* p = new (std::nothrow) PwPlanner();
  if (!p) return pw_fail(PW_ENOMEM, "out of memory");
  std::memset(static_cast<void*>(p), 0, sizeof(*p));
  p->eng = e;
  p->puzzle = puzzle;
  p->mode = mode;
  p->K = batch;
  p->flags = flags;
  p->max_states = max_states;
  p->sync_rounds = kPlanSyncRounds;
  if (int rc = search_create(e, puzzle, max_states, 0, batch, &p->s)) {
    pw_planner_destroy(p);
    return rc;
  }
  if (int rc = pw_rgd_create(e, puzzle, 1, rgd_budget, &p->rgd)) {
    pw_planner_destroy(p);
    return rc;
  }
  const PwPuzzleHeader& h = e->set->headers[puzzle];
  const int64_t slots = 4ll * batch;
  p->q.nb = (mode == PW_PLAN_RGD ? kPlanRgdBuckets : 3u * kPlanNrgdRange) + 2u;
  p->q.n0 = (p->q.nb + 63u) / 64u;
  p->q.n1 = (p->q.n0 + 63u) / 64u;
  p->q.n2 = (p->q.n1 + 63u) / 64u;
  PwDeviceGuard guard(e->set->device);
  PwHipChain c(guard.status());
  const size_t ms = static_cast<size_t>(max_states);
  c.alloc(&p->q.head, static_cast<size_t>(p->q.nb) * 4);
  c.alloc(&p->q.bits0, static_cast<size_t>(p->q.n0) * 8);
  c.alloc(&p->q.bits1, static_cast<size_t>(p->q.n1) * 8);
  c.alloc(&p->q.bits2, static_cast<size_t>(p->q.n2) * 8);
  c.alloc(&p->q.seg_start, ms * 4);
  c.alloc(&p->q.seg_len, ms * 4);
  c.alloc(&p->q.seg_next, ms * 4);
  c.alloc(&p->q.ent, ms * 4);
  c.alloc(&p->d_info, kPSlots * 8);
  c.alloc(&p->d_plist, static_cast<size_t>(batch) * 4);
  c.alloc(&p->d_pperm, static_cast<size_t>(batch));
  c.alloc(&p->d_groups, kPlanGroups);
  c.alloc(&p->d_rsrc, static_cast<size_t>(batch) * 4);
  c.alloc(&p->d_rlen, static_cast<size_t>(batch) * 4);
  c.alloc(&p->d_roff, static_cast<size_t>(batch) * 4);
  c.alloc(&p->d_rows, static_cast<size_t>(slots) * h.N * 4);
  c.alloc(&p->d_cost, static_cast<size_t>(slots) * 4);
  for (int k = 0; k < 2; k++) {
    c.alloc(&p->d_keys[k], static_cast<size_t>(slots) * 4);
    c.alloc(&p->d_vals[k], static_cast<size_t>(slots) * 4);
  }
  c.then([&] {
    return rocprim::radix_sort_pairs(nullptr, p->sort_tmp_bytes, p->d_keys[0], p->d_keys[1], p->d_vals[0], p->d_vals[1],
                                     static_cast<size_t>(slots), 0, kPlanSortBits, nullptr);
  });
  c.alloc(&p->d_sort_tmp, std::max<size_t>(p->sort_tmp_bytes, 16));
  if (mode == PW_PLAN_N_RGD) {
    c.alloc(&p->d_state_nov, ms);
    c.alloc(&p->s->d_cand_moved, static_cast<size_t>(slots) * 4);
    c.alloc(&p->s->d_cand_nov, static_cast<size_t>(slots));
  }
  c.then([&] { return plan_upload_groups(p->d_groups); });
  if (!c.ok()) {
    pw_planner_destroy(p);
    return pw_hip_fail("pw_planner_create", c.err);
  }
  if (mode == PW_PLAN_N_RGD) {
    if (int rc = novelty_alloc(e->set->device, h.N, h.W, h.H, &p->s->nov)) {
      pw_planner_destroy(p);
      return rc;
    }
  }
  *out = p;
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_planner_set_sync_rounds(PwPlanner* p, int32_t rounds) try {
  if (!p) return pw_fail(PW_EINVAL, "null argument");
  if (rounds < 0) return pw_fail(PW_EINVAL, "rounds must be >= 0 (0 = the default)");
  p->sync_rounds = rounds > 0 ? rounds : kPlanSyncRounds;
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_planner_begin(PwPlanner* p, const int32_t* start, void* stream) try {
  if (!p) return pw_fail(PW_EINVAL, "null argument");
  p->begun = false;
  if (int rc = pw_search_begin(p->s, start, stream)) return rc;  // store, closed set, the goal test of the start state
  PwDeviceGuard guard(p->eng->set->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool goal = p->s->goal_index == 0;
  unsigned long long info[kPSlots] = {0};
  info[kPStatus] = goal ? PW_PLAN_SOLVED : PW_PLAN_RUNNING;
  info[kPVisited] = 1;
  info[kPGoal] = goal ? 0ull : ~0ull;
  info[kPFirst] = 0;
  info[kPNew] = goal ? 0 : 1;  // the start state is scored and pushed like a round's new state
  info[kPMin] = p->q.nb;
  hipError_t err = hipMemsetAsync(p->q.head, 0xFF, static_cast<size_t>(p->q.nb) * 4, st);
  if (err == hipSuccess) err = hipMemsetAsync(p->q.bits0, 0, static_cast<size_t>(p->q.n0) * 8, st);
  if (err == hipSuccess) err = hipMemsetAsync(p->q.bits1, 0, static_cast<size_t>(p->q.n1) * 8, st);
  if (err == hipSuccess) err = hipMemsetAsync(p->q.bits2, 0, static_cast<size_t>(p->q.n2) * 8, st);
  if (err == hipSuccess) err = hipMemsetAsync(p->rgd->d_exceeded, 0, 8, st);
  if (err == hipSuccess && p->d_state_nov) err = hipMemsetAsync(p->d_state_nov, 1, 1, st);  // all objects moved: novelty 1
  if (err == hipSuccess) err = hipMemcpyAsync(p->d_info, info, sizeof(info), hipMemcpyHostToDevice, st);
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string("pw_planner_begin: ") + hipGetErrorString(err));
  if (p->s->nov) {  // best_first_search.h:58-67: the start state enters the novelty tables with every object moved
    if (int rc = pw_novelty_reset(p->s->nov, stream)) return rc;
    hipLaunchKernelGGL(pw_search_root_novelty_kernel, dim3(1), dim3(64), 0, st, search_args(p->s));
    if (int rc = check_launch("pw_planner_begin")) return rc;
    p->s->nov->next_id = 1;
  }
  if (!goal)
    if (int rc = plan_push(p, st)) return rc;
  err = hipStreamSynchronize(st);  // (info is a stack variable)
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string("pw_planner_begin: ") + hipGetErrorString(err));
  p->status = info[kPStatus];
  p->begun = true;
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_planner_run(PwPlanner* p, int64_t max_rounds, int64_t info_out[8], void* stream) try {
  if (!p || !info_out) return pw_fail(PW_EINVAL, "null argument");
  if (!p->begun) return pw_fail(PW_EINVAL, "pw_planner_begin has not been called");
  PwDeviceGuard guard(p->eng->set->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  unsigned long long info[kPSlots] = {0};
  hipError_t err = hipSuccess;
  int64_t left = max_rounds;
  for (;;) {  // the status is read once per group of rounds
    err = hipMemcpyAsync(info, p->d_info, sizeof(info), hipMemcpyDeviceToHost, st);
    if (err == hipSuccess) err = hipStreamSynchronize(st);
    if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string("pw_planner_run: ") + hipGetErrorString(err));
    p->status = static_cast<int64_t>(info[kPStatus]);
    if (p->status != PW_PLAN_RUNNING || (max_rounds > 0 && left <= 0)) break;
    const int64_t group = max_rounds > 0 ? std::min<int64_t>(left, p->sync_rounds) : p->sync_rounds;
    const int64_t slots = 4ll * p->K;
    if (p->s->nov && static_cast<uint64_t>(p->s->nov->next_id) + static_cast<uint64_t>(group * slots) >= 0xFFFFFFFFull)
      return pw_fail(PW_ELIMIT, "novelty ids exhausted (2^32 candidates): the search cannot go on");
    const BfsPlanArgs a = plan_args(p);
    SearchArgs sa = search_args(p->s);
    sa.plist = p->d_plist;
    sa.pperm = p->d_pperm;
    sa.halt = p->d_info + kPStatus;
    sa.state_nov = p->d_state_nov;
    sa.first = 0;
    sa.nparents = p->K;
    sa.ncand = static_cast<int32_t>(slots);
    for (int64_t r = 0; r < group; r++) {
      hipLaunchKernelGGL(pw_planner_pop_kernel, dim3(1), dim3(256), 0, st, a);
      sa.epoch = ++p->s->epoch;
      search_pass(p->s, sa, st, false);
      hipLaunchKernelGGL(pw_planner_finish_kernel, dim3(1), dim3(1), 0, st, a);
      if (int rc = plan_push(p, st)) return rc;
    }
    left -= group;
  }
  if (p->status == PW_PLAN_ERANGE) {
    const float r = __builtin_bit_cast(float, static_cast<uint32_t>(info[kPRangeKey] - 1ull));
    return pw_fail(PW_ELIMIT, "pw_planner_run: an RGD cost of " + std::to_string(r) + " does not fit the bucket range (" +
                                  (p->mode == PW_PLAN_RGD ? std::string("0 .. 4194303") : std::string("0 .. 999999 in N+RGD mode")) +
                                  ")");
  }
  unsigned long long stored = 0;
  err = hipMemcpyAsync(&stored, p->s->d_info, 8, hipMemcpyDeviceToHost, st);
  unsigned long long exceeded = 0;
  if (err == hipSuccess) err = hipMemcpyAsync(&exceeded, p->rgd->d_exceeded, 8, hipMemcpyDeviceToHost, st);
  if (err == hipSuccess) err = hipStreamSynchronize(st);
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string("pw_planner_run: ") + hipGetErrorString(err));
  p->s->layer_end = static_cast<int64_t>(stored);
  info_out[0] = static_cast<int64_t>(info[kPStatus]);
  info_out[1] = static_cast<int64_t>(info[kPRounds]);
  info_out[2] = static_cast<int64_t>(info[kPExpanded]);
  info_out[3] = static_cast<int64_t>(info[kPVisited]);
  info_out[4] = static_cast<int64_t>(info[kPOpen]);
  info_out[5] = info[kPGoal] == ~0ull ? -1 : static_cast<int64_t>(info[kPGoal]);
  info_out[6] = static_cast<int64_t>(exceeded);
  info_out[7] = static_cast<int64_t>(stored);
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_planner_max_key(PwPlanner* p, float* out, void* stream) try {
  if (!p || !out) return pw_fail(PW_EINVAL, "null argument");
  PwDeviceGuard guard(p->eng->set->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  unsigned long long v = 0;
  hipError_t err = hipMemcpyAsync(&v, p->d_info + kPMaxKey, 8, hipMemcpyDeviceToHost, st);
  if (err == hipSuccess) err = hipStreamSynchronize(st);
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string("pw_planner_max_key: ") + hipGetErrorString(err));
  *out = __builtin_bit_cast(float, static_cast<uint32_t>(v));
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_planner_plan(PwPlanner* p, uint8_t* actions, int32_t cap, void* stream) try {
  if (!p) return pw_fail(PW_EINVAL, "null argument");
  if (!p->begun) return pw_fail(PW_EINVAL, "pw_planner_begin has not been called");
  PwDeviceGuard guard(p->eng->set->device);
  unsigned long long goal = ~0ull;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t err = hipMemcpyAsync(&goal, p->d_info + kPGoal, 8, hipMemcpyDeviceToHost, st);
  if (err == hipSuccess) err = hipStreamSynchronize(st);
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string("pw_planner_plan: ") + hipGetErrorString(err));
  if (goal == ~0ull) return pw_fail(PW_EINVAL, "pw_planner_plan: no plan (the search has not solved the puzzle)");
  if (p->s->layer_end <= static_cast<int64_t>(goal)) p->s->layer_end = static_cast<int64_t>(goal) + 1;
  return pw_search_plan(p->s, static_cast<int64_t>(goal), actions, cap, stream);
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

}  // extern "C"

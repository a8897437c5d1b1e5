// pw_push_planner.inc -- K17: best-first search over pushes, RGD-ordered, on canonical states.
// Part of the single translation unit pw_kernels.hip, included after pw_push_search.inc: the store, the closed set and the
// pass are K16's (push_search_pass over a pop list), the queue is K8's (BfsPlanQueue, the key and segment kernels of
// pw_planner.inc), the keys are pw_rgd_eval_kernel's.  What is new here is the round that joins them:
//
//   pop       one workgroup: up to K entries off the lowest non-empty buckets, newest first -> plist (store indices, -1 past
//             the end); the popped states' stored push counts -> f_offset (the scan's input) and their sum T; the verdict
//             `limit` when states + T > max_states
//   scan      rocPRIM: f_offset -> row offsets
//   gather    the popped parents' positions -> gpos, contiguous, so that walk_launch reads them as a batch
//   (the host's one wait of the round: status, T and the number popped; the row workspace grows here)
//   pass      push_search_pass: the two floods, candidate, claim, flags, scan, publish (parent = plist[row_item]), finish
//   finish    one lane: a goal row -> solved; otherwise the round's new states are store indices [first, first + new)
//   unpack    new states: int8 pairs -> pw_rgd_eval's int32 rows; the largest region of the new states
//   eval      pw_rgd_eval_kernel, the count in device memory
//   key, sort, segment   as K8 (the sort covers the round's T slots rounded up to 4, padding sorts last)
//
// The info words are K8's PlanSlot layout (the key and segment kernels read it) with four words of this file after it.
// Every kernel of this file returns at once when the status word is not 0.  The shared K16 kernels are never launched with
// the status set: the host reads it before every pass.  Every loop is bounded by K, the rows, the buckets or the store.

enum PushPlanSlot { kPPRows = 11, kPPPopped = 12, kPPPushRows = 13, kPPRegion = 14 };  // (after PlanSlot's kPRangeKey = 10)
#define PW_PP_EINTERNAL 5  // internal status: the store or the table overflowed although states + T <= max_states

struct PushPlanArgs {
  unsigned long long* info;         // [kPSlots]
  const unsigned long long* sinfo;  // the store's info words (PW_PS_I_*)
  BfsPlanQueue q;
  int32_t* plist;   // [K]
  int32_t* rsrc;    // [K] pop ranges, as K8
  int32_t* rlen;
  int32_t* roff;
  int32_t K, N, npad;
  int64_t max_states;
  const int8_t* pos;       // the store
  const int32_t* rsize;
  const int32_t* npush;
  int64_t* f_offset;       // [K + 1]
  int8_t* gpos;            // [K][npad][2]
  int32_t* rows;           // [cap][N] Position2D of the round's new states
};

// ---- pop: up to K entries, lowest bucket first, newest first within a bucket; their push counts and the total ------------
__global__ __launch_bounds__(256) void pw_push_planner_pop_kernel(PushPlanArgs a) {
  __shared__ int s_n, s_nr;
  __shared__ long long s_sum[4];
  if (threadIdx.x == 0) {
    int n = -1, nr = 0;
    if (a.info[kPStatus] == 0) {
      const unsigned long long open = a.info[kPOpen];
      if (open == 0) {
        a.info[kPStatus] = PW_PLAN_EXHAUSTED;
      } else {
        n = 0;
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
        a.info[kPMin] = b;
        a.info[kPOpen] = open - static_cast<unsigned long long>(n);
        a.info[kPExpanded] += static_cast<unsigned long long>(n);
        a.info[kPRounds] += 1;
        a.info[kPFirst] = a.sinfo[PW_PS_I_STATES];
        a.info[kPNew] = 0;
        a.info[kPPPopped] = static_cast<unsigned long long>(n);
      }
    }
    s_n = n;
    s_nr = nr;
  }
  __syncthreads();
  const int n = s_n, nr = s_nr;
  if (n < 0) return;  // done before this round, or exhausted
  long long sum = 0;
  for (int o = threadIdx.x; o < a.K; o += 256) {
    int32_t v = -1;
    int32_t cnt = 0;
    if (o < n) {
      int lo = 0, hi = nr - 1;  // the last range that starts at or before rank o
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.roff[mid] <= o) lo = mid;
        else hi = mid - 1;
      }
      v = a.q.ent[a.rsrc[lo] - 1 - (o - a.roff[lo])];
      cnt = a.npush[v];
    }
    a.plist[o] = v;
    a.f_offset[o] = cnt;
    sum += cnt;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o, PW_WAVE);
  if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long T = static_cast<unsigned long long>(s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3]);
    a.f_offset[a.K] = 0;  // the scan's last input: f_offset[K] becomes the total
    a.info[kPPRows] = T;
    a.info[kPPPushRows] += T;
    if (a.sinfo[PW_PS_I_STATES] + T > static_cast<unsigned long long>(a.max_states)) a.info[kPStatus] = PW_PLAN_LIMIT;
  }
}

// ---- gather: the popped parents' positions, contiguous in pop order -------------------------------------------------------
__global__ __launch_bounds__(256) void pw_push_planner_gather_kernel(PushPlanArgs a) {
  if (a.info[kPStatus]) return;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  const int words = a.npad / 2;
  const int64_t n = static_cast<int64_t>(a.info[kPPPopped]);
  if (i >= n * words) return;
  const int64_t r = i / words;
  const int k = static_cast<int>(i - r * words);
  const int64_t idx = a.plist[r];
  reinterpret_cast<uint32_t*>(a.gpos)[i] = reinterpret_cast<const uint32_t*>(a.pos + idx * a.npad * 2)[k];
}

// ---- finish: the goal, or the round's new states ---------------------------------------------------------------------------
__global__ void pw_push_planner_finish_kernel(PushPlanArgs a) {
  if (blockIdx.x != 0 || threadIdx.x != 0 || a.info[kPStatus]) return;
  const unsigned long long goal = a.sinfo[PW_PS_I_GOAL];
  if (a.sinfo[PW_PS_I_OVERFLOW] != 0ull) {
    a.info[kPStatus] = PW_PP_EINTERNAL;
  } else if (goal != PW_PS_NOGOAL) {  // the successor of the first goal row: the last state of the store
    a.info[kPStatus] = PW_PLAN_SOLVED;
    a.info[kPGoal] = goal;
    a.info[kPNew] = 0;
  } else {
    a.info[kPNew] = a.sinfo[PW_PS_I_STATES] - a.info[kPFirst];
  }
}

// ---- unpack: the new states as pw_rgd_eval's rows; the largest region among them -----------------------------------------------
__global__ __launch_bounds__(256) void pw_push_planner_unpack_kernel(PushPlanArgs a) {
  if (a.info[kPStatus]) return;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  const int64_t n = static_cast<int64_t>(a.info[kPNew]);
  int rs = 0;
  if (i < n * a.N) {
    const int64_t s = i / a.N;
    const int j = static_cast<int>(i - s * a.N);
    const int64_t idx = static_cast<int64_t>(a.info[kPFirst]) + s;
    const int8_t* xy = a.pos + (idx * a.npad + j) * 2;  // (a stored state lies inside its grid: no negative coordinate)
    a.rows[i] = static_cast<int32_t>(xy[0]) * PW_POSITION_LIMIT + static_cast<int32_t>(xy[1]);
    if (j == 0) rs = a.rsize[idx];
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) rs = max(rs, __shfl_xor(rs, o, PW_WAVE));  // one atomic per wavefront
  if ((threadIdx.x & 63) == 0 && rs > 0) atomicMax(&a.info[kPPRegion], static_cast<unsigned long long>(rs));
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
struct PwPushPlanner {
  PwEngine* eng;
  int32_t puzzle, K;
  int64_t max_states;
  PwPushSearch* s;  // store, closed set, row workspace (parents per pass = K)
  PwRgd* rgd;
  BfsPlanQueue q;
  unsigned long long* d_info;
  int32_t* d_plist;
  int32_t* d_rsrc;
  int32_t* d_rlen;
  int32_t* d_roff;
  int8_t* d_gpos;
  // per new state of a round (grown with the row workspace)
  int64_t eval_cap;  // a multiple of 4
  int32_t* d_rows;
  float* d_cost;
  uint32_t* d_keys[2];
  int32_t* d_vals[2];
  void* d_sort_tmp;
  size_t sort_tmp_bytes;
  bool begun;
  int64_t status, states;
};

static void push_planner_free_eval(PwPushPlanner* p) {
  void* bufs[] = {p->d_rows, p->d_cost, p->d_keys[0], p->d_keys[1], p->d_vals[0], p->d_vals[1], p->d_sort_tmp};
  for (void* b : bufs)
    if (b) (void)hipFree(b);
  p->d_rows = nullptr;
  p->d_cost = nullptr;
  p->d_keys[0] = p->d_keys[1] = nullptr;
  p->d_vals[0] = p->d_vals[1] = nullptr;
  p->d_sort_tmp = nullptr;
  p->eval_cap = 0;
}

// the buffers of `rows` new states (the caller has waited for the stream: nothing in flight reads the old ones)
static int push_planner_reserve_eval(PwPushPlanner* p, int64_t rows, const char* what) {
  if (rows <= p->eval_cap) return PW_OK;
  push_planner_free_eval(p);
  const int64_t cap = (std::max<int64_t>(rows + rows / 2, 4096) + 3) & ~3ll;
  PwHipChain c;
  const size_t n = static_cast<size_t>(cap);
  c.alloc(&p->d_rows, n * p->s->N * 4);
  c.alloc(&p->d_cost, n * 4);
  for (int k = 0; k < 2; k++) {
    c.alloc(&p->d_keys[k], n * 4);
    c.alloc(&p->d_vals[k], n * 4);
  }
  c.then([&] {
    return rocprim::radix_sort_pairs(nullptr, p->sort_tmp_bytes, p->d_keys[0], p->d_keys[1], p->d_vals[0], p->d_vals[1], n, 0,
                                     kPlanSortBits, nullptr);
  });
  c.alloc(&p->d_sort_tmp, std::max<size_t>(p->sort_tmp_bytes, 16));
  if (!c.ok()) {
    push_planner_free_eval(p);
    return pw_hip_fail(what, c.err);
  }
  p->eval_cap = cap;
  return PW_OK;
}

static PushPlanArgs push_planner_args(PwPushPlanner* p) {
  PushPlanArgs a{};
  a.info = p->d_info;
  a.sinfo = p->s->d_info;
  a.q = p->q;
  a.plist = p->d_plist;
  a.rsrc = p->d_rsrc;
  a.rlen = p->d_rlen;
  a.roff = p->d_roff;
  a.K = p->K;
  a.N = p->s->N;
  a.npad = p->s->npad;
  a.max_states = p->max_states;
  a.pos = p->s->d_pos;
  a.rsize = p->s->d_rsize;
  a.npush = p->s->d_npush;
  a.f_offset = p->s->d_f_offset;
  a.gpos = p->d_gpos;
  a.rows = p->d_rows;
  return a;
}

// score and push the states [info[kPFirst], + info[kPNew]), at most `slots` of them (unpack, RGD, key, sort, segment)
static int push_planner_push(PwPushPlanner* p, int64_t slots, hipStream_t st) {
  const int64_t slots4 = (slots + 3) & ~3ll;  // K8's key kernel covers 4 K slots
  const PushPlanArgs a = push_planner_args(p);
  BfsPlanArgs b{};
  b.info = p->d_info;
  b.q = p->q;
  b.K = static_cast<int32_t>(slots4 / 4);
  b.mode = PW_PLAN_RGD;
  b.max_states = p->max_states;
  b.cost = p->d_cost;
  b.keys = p->d_keys[0];
  b.vals = p->d_vals[0];
  b.skeys = p->d_keys[1];
  b.svals = p->d_vals[1];
  hipLaunchKernelGGL(pw_push_planner_unpack_kernel, dim3(static_cast<unsigned>((slots * a.N + 255) / 256)), dim3(256), 0, st, a);
  RgdEvalArgs r = rgd_eval_args(p->rgd, p->d_rows, p->d_cost, static_cast<int32_t>(slots));
  r.dcount = p->d_info + kPNew;
  r.halt = p->d_info + kPStatus;
  hipLaunchKernelGGL(pw_rgd_eval_kernel, dim3(static_cast<unsigned>((slots + PW_WAVE - 1) / PW_WAVE)), dim3(PW_WAVE),
                     rgd_eval_lds(p->rgd), st, r);
  const unsigned kblocks = static_cast<unsigned>((slots4 + 255) / 256);
  hipLaunchKernelGGL(pw_planner_key_kernel, dim3(kblocks), dim3(256), 0, st, b);
  size_t tmp = p->sort_tmp_bytes;
  const hipError_t err = rocprim::radix_sort_pairs(p->d_sort_tmp, tmp, p->d_keys[0], p->d_keys[1], p->d_vals[0], p->d_vals[1],
                                                   static_cast<size_t>(slots4), 0, kPlanSortBits, st);
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string("pw_push_planner: radix sort: ") + hipGetErrorString(err));
  hipLaunchKernelGGL(pw_planner_segment_kernel, dim3(kblocks), dim3(256), 0, st, b);
  return check_launch("pw_push_planner");
}

extern "C" {

void pw_push_planner_destroy(PwPushPlanner* p) {
  if (!p) return;
  void* bufs[] = {p->q.head, p->q.bits0, p->q.bits1, p->q.bits2, p->q.seg_start, p->q.seg_len, p->q.seg_next, p->q.ent,
                  p->d_info, p->d_plist, p->d_rsrc, p->d_rlen, p->d_roff, p->d_gpos};
  for (void* b : bufs)
    if (b) (void)hipFree(b);
  push_planner_free_eval(p);
  pw_push_search_destroy(p->s);
  pw_rgd_destroy(p->rgd);
  delete p;
}

int pw_push_planner_create(PwEngine* e, int32_t puzzle, int64_t max_states, int32_t batch, int64_t rgd_budget,
                           PwPushPlanner** out) try {
  if (!e) return pw_fail(PW_EINVAL, "pw_push_planner_create: null engine");
  if (!out) return pw_fail(PW_EINVAL, "pw_push_planner_create: null out");
  if (max_states < 1 || max_states >= (1ll << 31))
    return pw_fail(PW_EINVAL, "pw_push_planner_create: max_states must be in 1 .. 2^31 - 1");
  if (batch < 1 || batch > 65536) return pw_fail(PW_EINVAL, "pw_push_planner_create: batch (K) must be in 1 .. 65536");
  if (rgd_budget < 0) return pw_fail(PW_EINVAL, "pw_push_planner_create: rgd_budget must be >= 0 (0 = the default)");
  if (puzzle < 0 || puzzle >= e->set->count) return pw_fail(PW_EINVAL, "pw_push_planner_create: puzzle index out of range");
  *out = nullptr;
  PwPushPlanner* p = new (std::nothrow) PwPushPlanner();
  if (!p) return pw_fail(PW_ENOMEM, "pw_push_planner_create: out of memory");
  std::memset(static_cast<void*>(p), 0, sizeof(*p));
  p->eng = e;
  p->puzzle = puzzle;
  p->K = batch;
  p->max_states = max_states;
  if (int rc = push_search_create(e, puzzle, max_states, batch, &p->s)) {
    pw_push_planner_destroy(p);
    return rc;
  }
  if (int rc = pw_rgd_create(e, puzzle, 1, rgd_budget, &p->rgd)) {
    pw_push_planner_destroy(p);
    return rc;
  }
  p->q.nb = kPlanRgdBuckets + 2u;
  p->q.n0 = (p->q.nb + 63u) / 64u;
  p->q.n1 = (p->q.n0 + 63u) / 64u;
  p->q.n2 = (p->q.n1 + 63u) / 64u;
  PwDeviceGuard guard(e->set->device);
  PwHipChain c(guard.status());
  const size_t ms = static_cast<size_t>(max_states), k = static_cast<size_t>(batch);
  c.alloc(&p->q.head, static_cast<size_t>(p->q.nb) * 4);
  c.alloc(&p->q.bits0, static_cast<size_t>(p->q.n0) * 8);
  c.alloc(&p->q.bits1, static_cast<size_t>(p->q.n1) * 8);
  c.alloc(&p->q.bits2, static_cast<size_t>(p->q.n2) * 8);
  c.alloc(&p->q.seg_start, ms * 4);
  c.alloc(&p->q.seg_len, ms * 4);
  c.alloc(&p->q.seg_next, ms * 4);
  c.alloc(&p->q.ent, ms * 4);
  c.alloc(&p->d_info, kPSlots * 8);
  c.alloc(&p->d_plist, k * 4);
  c.alloc(&p->d_rsrc, k * 4);
  c.alloc(&p->d_rlen, k * 4);
  c.alloc(&p->d_roff, k * 4);
  c.alloc(&p->d_gpos, k * p->s->npad * 2);
  if (!c.ok()) {
    pw_push_planner_destroy(p);
    return pw_hip_fail("pw_push_planner_create", c.err);
  }
  *out = p;
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_push_planner_begin(PwPushPlanner* p, const int8_t* start, void* stream) try {
  if (!p) return pw_fail(PW_EINVAL, "pw_push_planner_begin: null planner");
  p->begun = false;
  const PwPuzzleHeader& h = p->eng->set->headers[p->puzzle];
  for (int j = 0; start && j < p->s->N; j++) {
    const int x = start[2 * j], y = start[2 * j + 1];
    if (x < 0 || y < 0 || x + h.objtab[j].w > h.W || y + h.objtab[j].h > h.H)
      return pw_fail(PW_EINVAL, "pw_push_planner_begin: start has a movable outside its grid");
  }
  // the store: the table cleared, the start flooded and published as state 0, its goal test (synchronises)
  if (int rc = pw_push_search_begin(p->s, start, 1, stream)) return rc;
  PwDeviceGuard guard(p->eng->set->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const bool goal = p->s->goal_index == 0;
  unsigned long long info[kPSlots] = {0};
  info[kPStatus] = goal ? PW_PLAN_SOLVED : PW_PLAN_RUNNING;
  info[kPGoal] = goal ? 0ull : ~0ull;
  info[kPNew] = goal ? 0 : 1;  // the start state is scored and pushed like a round's new state
  info[kPMin] = p->q.nb;
  hipError_t err = hipMemsetAsync(p->q.head, 0xFF, static_cast<size_t>(p->q.nb) * 4, st);
  if (err == hipSuccess) err = hipMemsetAsync(p->q.bits0, 0, static_cast<size_t>(p->q.n0) * 8, st);
  if (err == hipSuccess) err = hipMemsetAsync(p->q.bits1, 0, static_cast<size_t>(p->q.n1) * 8, st);
  if (err == hipSuccess) err = hipMemsetAsync(p->q.bits2, 0, static_cast<size_t>(p->q.n2) * 8, st);
  if (err == hipSuccess) err = hipMemsetAsync(p->rgd->d_exceeded, 0, 8, st);
  if (err == hipSuccess) err = hipMemcpyAsync(p->d_info, info, sizeof(info), hipMemcpyHostToDevice, st);
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string("pw_push_planner_begin: ") + hipGetErrorString(err));
  if (!goal) {
    if (int rc = push_planner_reserve_eval(p, 1, "pw_push_planner_begin")) return rc;
    if (int rc = push_planner_push(p, 1, st)) return rc;
  }
  err = hipStreamSynchronize(st);  // (info is a stack variable)
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string("pw_push_planner_begin: ") + hipGetErrorString(err));
  p->status = static_cast<int64_t>(info[kPStatus]);
  p->states = 1;
  p->begun = true;
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_push_planner_run(PwPushPlanner* p, int64_t max_rounds, int64_t info_out[10], void* stream) try {
  if (!p) return pw_fail(PW_EINVAL, "pw_push_planner_run: null planner");
  if (!info_out) return pw_fail(PW_EINVAL, "pw_push_planner_run: null info");
  if (!p->begun) return pw_fail(PW_EINVAL, "pw_push_planner_run: pw_push_planner_begin has not been called");
  PwDeviceGuard guard(p->eng->set->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  PwPushSearch* s = p->s;
  unsigned long long info[kPSlots] = {0}, sinfo[PW_PS_I_WORDS] = {0}, exceeded = 0;
  const dim3 ggrid(static_cast<unsigned>((static_cast<int64_t>(p->K) * (s->npad / 2) + 255) / 256));
  for (int64_t done = 0;; done++) {
    const bool more = max_rounds <= 0 || done < max_rounds;
    if (more) {
      const PushPlanArgs a = push_planner_args(p);
      hipLaunchKernelGGL(pw_push_planner_pop_kernel, dim3(1), dim3(256), 0, st, a);
      size_t tmp = s->f_scan_bytes;
      const hipError_t serr = rocprim::exclusive_scan(s->d_f_scan, tmp, s->d_f_offset, s->d_f_offset, static_cast<int64_t>(0),
                                                      static_cast<size_t>(p->K) + 1, rocprim::plus<int64_t>(), st);
      if (serr != hipSuccess) {
        p->begun = false;
        return pw_fail(PW_EDEVICE, std::string("pw_push_planner_run: scan: ") + hipGetErrorString(serr));
      }
      hipLaunchKernelGGL(pw_push_planner_gather_kernel, ggrid, dim3(256), 0, st, a);
    }
    // the round's one wait: the status (the verdict of the round before, or of this pop) and the row count T together
    hipError_t err = hipGetLastError();
    if (err == hipSuccess) err = hipMemcpyAsync(info, p->d_info, sizeof(info), hipMemcpyDeviceToHost, st);
    if (err == hipSuccess) err = hipMemcpyAsync(sinfo, s->d_info, sizeof(sinfo), hipMemcpyDeviceToHost, st);
    if (err == hipSuccess) err = hipMemcpyAsync(&exceeded, p->rgd->d_exceeded, 8, hipMemcpyDeviceToHost, st);
    if (err == hipSuccess) err = hipStreamSynchronize(st);
    if (err != hipSuccess) {
      p->begun = false;
      return pw_fail(PW_EDEVICE, std::string("pw_push_planner_run: ") + hipGetErrorString(err));
    }
    p->status = static_cast<int64_t>(info[kPStatus]);
    if (p->status != PW_PLAN_RUNNING || !more) break;
    const int64_t T = static_cast<int64_t>(info[kPPRows]);
    if (T == 0) continue;  // no push from the popped states: nothing new (the pop left info[kPNew] = 0)
    if (T >= (1ll << 31) - 4) {
      p->begun = false;
      return pw_fail(PW_ELIMIT, "pw_push_planner_run: 2^31 push rows in one round (lower the batch)");
    }
    int rc = push_search_reserve_rows(s, T, st, "pw_push_planner_run");
    if (rc == PW_OK) rc = push_planner_reserve_eval(p, T, "pw_push_planner_run");
    if (rc != PW_OK) {
      p->begun = false;
      return rc;
    }
    PushSearchArgs a = push_search_args(s);
    a.stop = 1;
    a.first = 0;
    a.parents = static_cast<int32_t>(info[kPPPopped]);
    a.rows = static_cast<int32_t>(T);
    a.plist = p->d_plist;
    err = push_search_pass(s, a, p->d_gpos, st);
    if (err != hipSuccess) {
      p->begun = false;
      return pw_fail(PW_EDEVICE, std::string("pw_push_planner_run: ") + hipGetErrorString(err));
    }
    hipLaunchKernelGGL(pw_push_planner_finish_kernel, dim3(1), dim3(64), 0, st, push_planner_args(p));
    if ((rc = push_planner_push(p, T, st)) != PW_OK) {
      p->begun = false;
      return rc;
    }
  }
  p->states = static_cast<int64_t>(sinfo[PW_PS_I_STATES]);
  s->layer_end = p->states;  // (the bound of the store's read functions)
  if (p->status == PW_PLAN_ERANGE) {
    const float r = __builtin_bit_cast(float, static_cast<uint32_t>(info[kPRangeKey] - 1ull));
    return pw_fail(PW_ELIMIT, "pw_push_planner_run: an RGD cost of " + std::to_string(r) +
                                  " does not fit the bucket range (0 .. 4194303)");
  }
  if (p->status == PW_PP_EINTERNAL)
    return pw_fail(PW_EDEVICE, "pw_push_planner_run: the store overflowed below max_states (an internal error)");
  const float maxkey = __builtin_bit_cast(float, static_cast<uint32_t>(info[kPMaxKey]));
  info_out[0] = p->status;
  info_out[1] = static_cast<int64_t>(info[kPRounds]);
  info_out[2] = static_cast<int64_t>(info[kPExpanded]);
  info_out[3] = p->states;
  info_out[4] = static_cast<int64_t>(info[kPOpen]);
  info_out[5] = info[kPGoal] == ~0ull ? -1 : static_cast<int64_t>(info[kPGoal]);
  info_out[6] = static_cast<int64_t>(exceeded);
  info_out[7] = static_cast<int64_t>(info[kPPPushRows]);
  info_out[8] = static_cast<int64_t>(info[kPPRegion]);
  // (a pushed state is no goal state, so its finite key is at least 1: the word still 0 means that none was pushed)
  info_out[9] = info[kPMaxKey] == 0ull ? -1 : static_cast<int64_t>(maxkey);
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_push_planner_read_states(PwPushPlanner* p, int64_t first, int64_t count, int8_t* pos, int8_t* canon, void* stream) try {
  if (!p) return pw_fail(PW_EINVAL, "pw_push_planner_read_states: null planner");
  if (!p->begun) return pw_fail(PW_EINVAL, "pw_push_planner_read_states: pw_push_planner_begin has not been called");
  if (first < 0 || count < 0 || first + count > p->states)
    return pw_fail(PW_EINVAL, "pw_push_planner_read_states: state range out of bounds");
  p->s->layer_end = p->states;
  return pw_push_search_read_states(p->s, first, count, pos, canon, stream);
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_push_planner_read_links(PwPushPlanner* p, int64_t first, int64_t count, int32_t* parent, int8_t* from, uint8_t* action,
                               int32_t* walk, uint8_t* goal, void* stream) try {
  if (!p) return pw_fail(PW_EINVAL, "pw_push_planner_read_links: null planner");
  if (!p->begun) return pw_fail(PW_EINVAL, "pw_push_planner_read_links: pw_push_planner_begin has not been called");
  if (first < 0 || count < 0 || first + count > p->states)
    return pw_fail(PW_EINVAL, "pw_push_planner_read_links: state range out of bounds");
  p->s->layer_end = p->states;
  return pw_push_search_read_links(p->s, first, count, parent, from, action, walk, goal, stream);
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_push_planner_plan(PwPushPlanner* p, uint8_t* actions, int32_t cap, int32_t* pushes, void* stream) try {
  if (!p) return pw_fail(PW_EINVAL, "pw_push_planner_plan: null planner");
  if (!actions && cap > 0) return pw_fail(PW_EINVAL, "pw_push_planner_plan: null actions");
  if (cap < 0) return pw_fail(PW_EINVAL, "pw_push_planner_plan: cap must be >= 0");
  if (!p->begun) return pw_fail(PW_EINVAL, "pw_push_planner_plan: pw_push_planner_begin has not been called");
  if (p->status != PW_PLAN_SOLVED) return pw_fail(PW_EINVAL, "pw_push_planner_plan: no plan (the search has not solved the puzzle)");
  // the chain of parents is bounded by the number of states, not by a depth
  return push_search_plan(p->s, p->states - 1, p->states, actions, cap, pushes, stream);
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

}  // extern "C"

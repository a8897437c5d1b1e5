// pw_engine_obs.inc -- the render tuner (TuneScope, tune_render_impl, pw_engine_tune_render) and the observation buffers the
// library owns: address ranges never used twice, pw_obs_alloc / pw_obs_free, and pw_obs_alloc_tuned with its candidate screen.
// Part of the single translation unit pw_kernels.hip, included after pw_engine_render.inc: uses page_path, ensure_rec,
// live_build, the retained_* rules and launch_render from there, fill_render_args, release_obs_buf and pw_zero_kernel from
// pw_engine.inc, and check_launch.

extern "C" {

// Restores the engine's tuning flag and profiling events when the tuner leaves, whichever way
struct TuneScope {
  PwEngine* e;
  std::vector<hipEvent_t> saved;
  explicit TuneScope(PwEngine* eng) : e(eng), saved(std::move(eng->prof_events)) {
    e->prof_events.clear();  // the tuner's launches are not profiled
    e->tuning = true;
  }
  ~TuneScope() {
    e->tuning = false;
    e->prof_events = std::move(saved);
  }
};

// (order, log2 run, KiB of LDS padding, every page loads); the first entry is the default
static const int kTuneCand[][4] = {{2, 6, 7, 0}, {2, 6, 8, 0}, {2, 6, 6, 0}, {2, 6, 5, 0}, {2, 5, 7, 0}, {2, 7, 7, 0},
                                   {0, 0, 7, 0}, {0, 0, 8, 0}, {0, 0, 6, 0}, {0, 0, 0, 0}, {1, 0, 0, 0}, {1, 0, 4, 0},
                                   {1, 0, 7, 0}, {2, 6, 0, 0}, {1, 1, 7, 0}, {1, 1, 5, 0}, {2, 6, 7, 1}, {2, 6, 6, 1},
                                   {2, 6, 8, 1}, {1, 1, 7, 1}};
static const int kNumTuneCand = static_cast<int>(sizeof(kTuneCand) / sizeof(kTuneCand[0]));

static void apply_tune_cand(PwEngine* e, int c) {
  e->page_order = kTuneCand[c][0];
  e->page_run_log2 = kTuneCand[c][1];
  e->page_lds_pad_kb = kTuneCand[c][2];
  e->page_load_all = kTuneCand[c][3];
}

// The tuner proper (device guard held by the caller, `ra` filled for `obs`): leaves the fastest launch configuration
// in the engine, its index in *best_out and its time in e->tuned_ns.  `obs` holds the observations on return.
static int tune_render_impl(PwEngine* e, const RenderArgs& ra, int32_t batch, hipStream_t st, int* best_out) {
  *best_out = 0;
  if (!page_path(e, ra.env_stride)) {  // other kernels have no launch variants: plain render
    launch_render(e, ra, batch, st);
    return check_launch("pw_engine_tune_render");
  }
  hipEvent_t ev0, ev1;
  if (hipEventCreate(&ev0) != hipSuccess) return pw_fail(PW_EDEVICE, "pw_engine_tune_render: hipEventCreate failed");
  if (hipEventCreate(&ev1) != hipSuccess) {
    (void)hipEventDestroy(ev0);
    return pw_fail(PW_EDEVICE, "pw_engine_tune_render: hipEventCreate failed");
  }
  hipError_t err = hipSuccess;
  int best = 0;
  float best_ms = 0.0f;
  {
    TuneScope scope(e);
    // the every-page-loads instances exist for the ppc-3 page kernel only
    const int n_cand = (e->rowpage && !(e->d_simg && e->simg_cached)) ? 16 : kNumTuneCand;
    // milliseconds per launch of candidate c over `reps` launches (after one warm launch, which also writes the records)
    auto measure = [&](int c, int reps) {
      apply_tune_cand(e, c);
      launch_render(e, ra, batch, st);
      if (err == hipSuccess) err = hipEventRecord(ev0, st);
      for (int k = 0; k < reps; k++) launch_render(e, ra, batch, st, true);
      if (err == hipSuccess) err = hipEventRecord(ev1, st);
      if (err == hipSuccess) err = hipEventSynchronize(ev1);
      float ms = 0.0f;
      if (err == hipSuccess) err = hipEventElapsedTime(&ms, ev0, ev1);
      return ms / static_cast<float>(reps);
    };
    // first pass over all candidates, then the three best again with more launches (run-to-run noise is 1-2 %,
    // the candidates differ by up to 15 %)
    std::vector<std::pair<float, int>> first;
    for (int c = 0; c < n_cand && err == hipSuccess; c++) first.push_back({measure(c, 5), c});
    std::sort(first.begin(), first.end());
    best = first.empty() ? 0 : first[0].second;
    for (int k = 0; k < 3 && k < static_cast<int>(first.size()) && err == hipSuccess; k++) {
      const float ms = measure(first[k].second, 12);
      if (k == 0 || ms < best_ms) {
        best = first[k].second;
        best_ms = ms;
      }
    }
  }
  // Second pass (PW_OPT_OBS_PADDING_ONCE): the same candidates for the launch of the live pages only -- a third of the pages in
  // a sparser write front need not like the order and the occupancy cap of the full sweep -- and, in the configuration that
  // wins, the early-exit form against the list.  `obs` is fully rendered here, so these launches write the same bytes again.
  PwRetained& rt = e->ret;
  if (rt.option && err == hipSuccess && live_applies(e, ra.env_stride, batch) && live_build(e, ra.puzzle_id, batch, st, true)) {
    uint32_t n_live = 0;
    err = hipMemcpyAsync(&n_live, rt.d_count, 4, hipMemcpyDeviceToHost, st);
    if (err == hipSuccess) err = hipStreamSynchronize(st);
    if (err == hipSuccess) {
      rt.n_live = n_live;
      TuneScope scope(e);
      const int n_cand = kNumTuneCand;  // (live_applies: the ppc-3 page kernel)
      auto measure_live = [&](int c, int reps, int form) {
        apply_tune_cand(e, c);
        launch_render(e, ra, batch, st, true, form);
        if (err == hipSuccess) err = hipEventRecord(ev0, st);
        for (int k = 0; k < reps; k++) launch_render(e, ra, batch, st, true, form);
        if (err == hipSuccess) err = hipEventRecord(ev1, st);
        if (err == hipSuccess) err = hipEventSynchronize(ev1);
        float ms = 0.0f;
        if (err == hipSuccess) err = hipEventElapsedTime(&ms, ev0, ev1);
        return ms / static_cast<float>(reps);
      };
      std::vector<std::pair<float, int>> first;
      for (int c = 0; c < n_cand && err == hipSuccess; c++) first.push_back({measure_live(c, 5, 1), c});
      std::sort(first.begin(), first.end());
      int lbest = first.empty() ? 0 : first[0].second;
      float lbest_ms = 0.0f;
      for (int k = 0; k < 3 && k < static_cast<int>(first.size()) && err == hipSuccess; k++) {
        const float ms = measure_live(first[k].second, 12, 1);
        if (k == 0 || ms < lbest_ms) {
          lbest = first[k].second;
          lbest_ms = ms;
        }
      }
      // the early exits keep the grid of the full render: in the list's configuration and in the full render's
      int ebest = lbest;
      float exit_ms = err == hipSuccess ? measure_live(lbest, 12, 2) : 0.0f;
      if (err == hipSuccess && best != lbest) {
        const float ms = measure_live(best, 12, 2);
        if (ms < exit_ms) {
          ebest = best;
          exit_ms = ms;
        }
      }
      if (err == hipSuccess) {
        rt.form = exit_ms < lbest_ms ? 2 : 1;
        const int keep = rt.form == 2 ? ebest : lbest;
        rt.tuned = true;
        rt.order = kTuneCand[keep][0];
        rt.run_log2 = kTuneCand[keep][1];
        rt.lds_pad_kb = kTuneCand[keep][2];
        rt.load_all = kTuneCand[keep][3];
        rt.list_ns = static_cast<int64_t>(lbest_ms * 1.0e6f);
        rt.exit_ns = static_cast<int64_t>(exit_ms * 1.0e6f);
      }
    }
  }
  (void)hipEventDestroy(ev0);
  (void)hipEventDestroy(ev1);
  apply_tune_cand(e, best);
  e->tuned_ns = static_cast<int64_t>(best_ms * 1.0e6f);
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string("pw_engine_tune_render: ") + hipGetErrorString(err));
  if (int rc2 = check_launch("pw_engine_tune_render")) return rc2;
  *best_out = best;
  return PW_OK;
}

int pw_engine_tune_render(PwEngine* e, const int32_t* puzzle_id, const int8_t* pos, void* obs, int64_t env_stride_bytes,
                          int32_t batch, void* stream) try {
  if (!e) return pw_fail(PW_EINVAL, "null engine");
  if (batch <= 0) return PW_OK;
  RenderArgs ra;
  int rc = fill_render_args(e, puzzle_id, pos, obs, env_stride_bytes, batch, &ra);
  if (rc != PW_OK) return rc;
  PwDeviceGuard guard(e->set->device);
  int best = 0;
  rc = tune_render_impl(e, ra, batch, static_cast<hipStream_t>(stream), &best);
  if (rc == PW_OK) {
    retained_after_full_render(e, ra, batch);
    e->ret.shown_valid = false;
    if (retained_tracks(e, ra, batch, 0)) {  // `obs` shows `pos`: say so in `shown` (the records are the ones the tuner left)
      PageRecArgs pa{ra.hdrs, ra.puzzle_id, ra.pos, static_cast<PageRec*>(e->d_rec), batch, ra.np, e->set->count, e->ret.d_shown, e->ret.d_changed};
      hipLaunchKernelGGL(pw_page_records_kernel, dim3((batch + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), pa);
      if (int rc2 = check_launch("pw_engine_tune_render")) return rc2;
      e->ret.shown_valid = true;
    }
  }
  return rc != PW_OK ? rc : best;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

// ------------------------------------------------------------------------------------
// Observation buffers owned by the library (HIP virtual-memory API)
// ------------------------------------------------------------------------------------
// Address ranges of library-owned buffers are never used twice in a process: a range that was freed and handed out
// again by the runtime showed stale contents on this runtime (tests/test_gpu_obs_alloc.py, profiles/r02_vmm_lottery.txt:
// faults), as if translations of the old mapping survived.  Every reservation therefore asks for an address above all
// earlier ones (a hint; far away from where the runtime reserves by itself), and a range the runtime returns although it
// overlaps one this process has freed before is parked -- kept reserved, never mapped -- and another one requested.
static std::mutex g_obs_va_mutex;
static uintptr_t g_obs_va_next = 0x200000000000ull;  // 32 TiB: free in a 47-bit Linux address space; also the WATERMARK: every
                                                     // range handed out so far lies below it, so a range at or above it is fresh
struct PwParkedRange {
  void* ptr;
  size_t bytes;
};
static std::vector<PwParkedRange> g_obs_va_parked;   // reservations the runtime placed below the watermark: kept (so that it cannot
                                                     // hand them out again), never mapped, given back when the process exits
static void release_parked_ranges() {
  std::lock_guard<std::mutex> lock(g_obs_va_mutex);
  for (const PwParkedRange& r : g_obs_va_parked) (void)hipMemAddressFree(r.ptr, r.bytes);
  g_obs_va_parked.clear();
}

// ranges handed out BELOW the hinted region (a runtime that ignores the address hint): they cannot be told apart by the watermark
static constexpr uintptr_t kObsVaBase = 0x200000000000ull;
static std::vector<PwParkedRange> g_obs_va_low_used;
static constexpr size_t kObsVaParkedMax = 64;  // parked reservations kept at most (beyond: the oldest go back to the runtime)

static hipError_t reserve_fresh_range(size_t total, void** out) {
  std::lock_guard<std::mutex> lock(g_obs_va_mutex);
  // (O(1) per request and bounded state while the runtime honours the address hint: one watermark instead of a list of every
  // range ever handed out.  A runtime that ignores the hint places ranges below the hinted region: such a range is accepted when
  // it overlaps none handed out there before -- recorded in a list -- instead of being parked for ever.)
  const size_t parked_before = g_obs_va_parked.size();
  for (int attempt = 0; attempt < 8; attempt++) {
    void* p = nullptr;
    const hipError_t err = hipMemAddressReserve(&p, total, 0, reinterpret_cast<void*>(g_obs_va_next), 0);
    if (err != hipSuccess) return err;
    const uintptr_t lo = reinterpret_cast<uintptr_t>(p), hi = lo + total;
    if (lo >= g_obs_va_next) {
      g_obs_va_next = (hi + (size_t(1) << 30)) & ~((uintptr_t(1) << 30) - 1);  // next GiB boundary
      *out = p;
      return hipSuccess;
    }
    if (hi <= kObsVaBase) {  // outside the hinted region altogether
      bool seen = false;
      for (const PwParkedRange& u : g_obs_va_low_used) {
        const uintptr_t ulo = reinterpret_cast<uintptr_t>(u.ptr), uhi = ulo + u.bytes;
        seen = seen || (lo < uhi && ulo < hi);
      }
      if (!seen) {
        g_obs_va_low_used.push_back({p, total});
        *out = p;
        return hipSuccess;
      }
    }
    if (g_obs_va_parked.empty()) std::atexit(release_parked_ranges);
    g_obs_va_parked.push_back({p, total});
  }
  // the request failed: what it parked goes back (nothing was mapped there), and the list stays bounded
  while (g_obs_va_parked.size() > parked_before) {
    (void)hipMemAddressFree(g_obs_va_parked.back().ptr, g_obs_va_parked.back().bytes);
    g_obs_va_parked.pop_back();
  }
  while (g_obs_va_parked.size() > kObsVaParkedMax) {
    (void)hipMemAddressFree(g_obs_va_parked.front().ptr, g_obs_va_parked.front().bytes);
    g_obs_va_parked.erase(g_obs_va_parked.begin());
  }
  return hipErrorOutOfMemory;
}

// device guard held by the caller
static int obs_alloc_impl(PwEngine* e, int32_t batch, PwObsBuf* out) {
  const int64_t stride = (e->obs_bytes + 511) & ~int64_t(511);
  const size_t want = static_cast<size_t>(batch) * static_cast<size_t>(stride);
  hipMemAllocationProp prop = {};
  prop.type = hipMemAllocationTypePinned;
  prop.location.type = hipMemLocationTypeDevice;
  prop.location.id = e->set->device;
  size_t gran = 0;
  if (hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityMinimum) != hipSuccess || gran == 0)
    return pw_fail(PW_EDEVICE, "pw_obs_alloc: hipMemGetAllocationGranularity failed");
  // 32 MiB chunks by default: the class statistics are the same from 2 MiB to 512 MiB chunks
  // (profiles/r02_vmm_lottery.txt), and ~120 mappings per 3.8 GB buffer are made and torn down in milliseconds
  size_t chunk = static_cast<size_t>(e->obs_chunk_mb > 0 ? e->obs_chunk_mb : 32) << 20;
  chunk = (chunk + gran - 1) / gran * gran;
  const size_t n = (want + chunk - 1) / chunk, total = n * chunk;
  PwObsBuf b;
  b.ptr = nullptr;
  b.bytes = 0;
  b.reserved = 0;
  b.chunk = chunk;
  hipError_t err = reserve_fresh_range(total, &b.ptr);
  if (err != hipSuccess) return pw_fail(PW_ENOMEM, std::string("pw_obs_alloc: hipMemAddressReserve: ") + hipGetErrorString(err));
  b.reserved = total;
  b.handles.reserve(n);
  hipMemAccessDesc acc = {};
  acc.location.type = hipMemLocationTypeDevice;
  acc.location.id = e->set->device;
  acc.flags = hipMemAccessFlagsProtReadWrite;
  size_t mapped = 0;
  for (size_t i = 0; i < n && err == hipSuccess; i++) {
    hipMemGenericAllocationHandle_t h;
    err = hipMemCreate(&h, chunk, &prop, 0);
    if (err != hipSuccess) break;
    b.handles.push_back(h);
    err = hipMemMap(static_cast<char*>(b.ptr) + i * chunk, chunk, 0, h, 0);
    if (err == hipSuccess) mapped += chunk;
    if (err == hipSuccess) err = hipMemSetAccess(static_cast<char*>(b.ptr) + i * chunk, chunk, &acc, 1);  // per mapping
  }
  if (err != hipSuccess) {
    const bool oom = err == hipErrorOutOfMemory;
    std::string msg = std::string("pw_obs_alloc: ") + hipGetErrorString(err);
    b.bytes = mapped;
    release_obs_buf(b);
    return pw_fail(oom ? PW_ENOMEM : PW_EDEVICE, msg);
  }
  b.bytes = total;
  *out = std::move(b);
  return PW_OK;
}

int pw_obs_alloc(PwEngine* e, int32_t batch, void** obs) try {
  if (!e || !obs) return pw_fail(PW_EINVAL, "null argument");
  *obs = nullptr;
  if (batch <= 0) return pw_fail(PW_EINVAL, "pw_obs_alloc: batch must be > 0");
  PwDeviceGuard guard(e->set->device);
  PwObsBuf b;
  if (int rc = obs_alloc_impl(e, batch, &b)) return rc;
  // (an own kernel: the runtime's memset walks a virtual-memory range mapping by mapping)
  hipLaunchKernelGGL(pw_zero_kernel, dim3(4096), dim3(256), 0, nullptr, static_cast<uint4*>(b.ptr), b.bytes / 16);
  hipError_t err = hipGetLastError();
  if (err == hipSuccess) err = hipDeviceSynchronize();
  if (err != hipSuccess || !ensure_rec(e, batch)) {
    release_obs_buf(b);
    return err != hipSuccess ? pw_fail(PW_EDEVICE, std::string("pw_obs_alloc: ") + hipGetErrorString(err))
                             : pw_fail(PW_ENOMEM, "pw_obs_alloc: cannot allocate the page records");
  }
  *obs = b.ptr;
  e->obs_bufs.push_back(std::move(b));
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_obs_free(PwEngine* e, void* obs) try {
  if (!e) return pw_fail(PW_EINVAL, "null engine");
  if (!obs) return PW_OK;
  for (size_t i = 0; i < e->obs_bufs.size(); i++) {
    if (e->obs_bufs[i].ptr != obs) continue;
    PwDeviceGuard guard(e->set->device);
    (void)hipDeviceSynchronize();  // nothing in flight may still write the buffer
    if (e->ret.obs == obs) {
      e->ret.valid = e->ret.shown_valid = false;
      e->ret.obs = nullptr;
    }
    release_obs_buf(e->obs_bufs[i]);
    e->obs_bufs.erase(e->obs_bufs.begin() + static_cast<std::ptrdiff_t>(i));
    return PW_OK;
  }
  return pw_fail(PW_EINVAL, "pw_obs_free: not a buffer of this engine's pw_obs_alloc");
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

// A quick look at a candidate buffer (device guard held by the caller): the best of five launch configurations, three
// timed launches each (~10 ms at 3.8 GB) -- the contiguous-part orders, where the classes show (C3: 0.53 ms on a fast-class
// buffer, 0.60+ on a slow-class one), and the two a slow-class buffer ends up with.  The full tuner runs on the kept
// candidate only, so a dozen candidates cost little more than their allocation.
static int screen_candidate(PwEngine* e, const RenderArgs& ra, int32_t batch, hipStream_t st, int64_t* ns_out) {
  *ns_out = 0;
  if (!page_path(e, ra.env_stride)) return PW_OK;
  static const int kScreen[] = {14, 19, 10, 16, 0};  // quarters + 7 KB, the same with every page loading, eighths, defaults
  const bool has_load_all = !(e->rowpage && !(e->d_simg && e->simg_cached));
  hipEvent_t ev0, ev1;
  if (hipEventCreate(&ev0) != hipSuccess) return pw_fail(PW_EDEVICE, "pw_obs_alloc_tuned: hipEventCreate failed");
  if (hipEventCreate(&ev1) != hipSuccess) {
    (void)hipEventDestroy(ev0);
    return pw_fail(PW_EDEVICE, "pw_obs_alloc_tuned: hipEventCreate failed");
  }
  hipError_t err = hipSuccess;
  float best = 0.0f;
  {
    TuneScope scope(e);
    for (int c : kScreen) {
      if (c >= 16 && !has_load_all) continue;
      apply_tune_cand(e, c);
      launch_render(e, ra, batch, st);  // warm; writes the page records
      if (err == hipSuccess) err = hipEventRecord(ev0, st);
      for (int k = 0; k < 3; k++) launch_render(e, ra, batch, st, true);
      if (err == hipSuccess) err = hipEventRecord(ev1, st);
      if (err == hipSuccess) err = hipEventSynchronize(ev1);
      float ms = 0.0f;
      if (err == hipSuccess) err = hipEventElapsedTime(&ms, ev0, ev1);
      ms /= 3.0f;
      if (best == 0.0f || ms < best) best = ms;
    }
  }
  (void)hipEventDestroy(ev0);
  (void)hipEventDestroy(ev1);
  apply_tune_cand(e, 0);
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string("pw_obs_alloc_tuned: ") + hipGetErrorString(err));
  if (int rc = check_launch("pw_obs_alloc_tuned")) return rc;
  *ns_out = static_cast<int64_t>(best * 1.0e6f);
  return PW_OK;
}

int pw_obs_alloc_tuned(PwEngine* e, const int32_t* puzzle_id, const int8_t* pos, int32_t batch, int32_t max_candidates,
                       void** obs, float* candidate_ms, int32_t* tried, void* stream) try {
  if (!e || !obs) return pw_fail(PW_EINVAL, "null argument");
  *obs = nullptr;
  if (tried) *tried = 0;
  if (batch <= 0) return pw_fail(PW_EINVAL, "pw_obs_alloc_tuned: batch must be > 0");
  if (!puzzle_id || !pos) return pw_fail(PW_EINVAL, "null device pointer");
  if (max_candidates < 1) max_candidates = 1;
  PwDeviceGuard guard(e->set->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int64_t stride = (e->obs_bytes + 511) & ~int64_t(511);
  if (!page_path(e, stride)) max_candidates = 1;  // no launch variants, no allocation classes measured
  if (!ensure_rec(e, batch)) return pw_fail(PW_ENOMEM, "pw_obs_alloc_tuned: cannot allocate the page records");
  struct Cand {
    PwObsBuf buf;
    int idx;
    int64_t ns;
  };
  std::vector<Cand> cands;  // all alive until the choice is made: every new one lands on other physical memory
  cands.reserve(static_cast<size_t>(max_candidates));  // no reallocation (nothing that could throw) while candidates are alive
  int rc = PW_OK;
  int64_t slowest = 0;
  size_t best = 0;
  const double bytes = static_cast<double>(batch) * static_cast<double>(e->obs_bytes);
  // the wall-clock budget of the screen (PW_OPT_OBS_TUNE_MS, default 10 s): a candidate costs 40-100 ms alone, but eight ranks of
  // one node screening at once share the driver's memory-mapping path -- whatever that costs, the constructor stays bounded
  const auto t_start = std::chrono::steady_clock::now();
  const int64_t budget_ms = e->obs_tune_ms > 0 ? e->obs_tune_ms : 10000;
  e->obs_screen_ms = 0;
  for (int k = 0; k < max_candidates; k++) {
    if (k > 0 && std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t_start).count() >= budget_ms) break;
    Cand c;
    c.idx = 0;
    c.ns = 0;
    rc = obs_alloc_impl(e, batch, &c.buf);
    if (rc != PW_OK) {
      if (!cands.empty()) rc = PW_OK;  // out of memory: choose among the candidates there are
      break;
    }
    hipLaunchKernelGGL(pw_zero_kernel, dim3(4096), dim3(256), 0, st, static_cast<uint4*>(c.buf.ptr), c.buf.bytes / 16);
    hipError_t err = hipGetLastError();
    RenderArgs ra;
    if (err == hipSuccess) rc = fill_render_args(e, puzzle_id, pos, c.buf.ptr, stride, batch, &ra);
    else rc = pw_fail(PW_EDEVICE, std::string("pw_obs_alloc_tuned: ") + hipGetErrorString(err));
    if (rc == PW_OK) rc = screen_candidate(e, ra, batch, st, &c.ns);  // (the full tuner runs on the kept one only)
    if (rc == PW_OK && hipStreamSynchronize(st) != hipSuccess) rc = pw_fail(PW_EDEVICE, "pw_obs_alloc_tuned: stream error");
    if (rc != PW_OK) {
      release_obs_buf(c.buf);
      break;
    }
    if (candidate_ms) candidate_ms[k] = static_cast<float>(c.ns) * 1.0e-6f;
    cands.push_back(std::move(c));
    if (tried) *tried = static_cast<int32_t>(cands.size());
    slowest = std::max(slowest, cands.back().ns);
    if (cands.back().ns < cands[best].ns) best = cands.size() - 1;
    // good enough: the fast class by its absolute rate (C3: 0.529-0.535 ms; medium 0.547-0.57, slow 0.58-0.61) -- or, once 16
    // candidates have been looked at without one, >= 8 % under the slowest seen.  (Until round 5 the relative rule applied from
    // the first candidate on: after 0.562 / 0.554 / 0.603 ms it kept the 0.554 one -- a medium candidate, 2.5 % short of the fast
    // class, because the third happened to be very slow; where the fast class turns up it does so late as often as early -- the
    // 6th, the 14th candidate in the sessions on record -- and a candidate costs ~40 ms of constructor time.)
    const double gbs = cands[best].ns > 0 ? bytes / static_cast<double>(cands[best].ns) : 0.0;  // bytes / ns = GB/s
    if (gbs >= static_cast<double>(e->obs_accept_gbs)) break;
    if (cands.size() >= 16 && static_cast<double>(cands[best].ns) <= 0.92 * static_cast<double>(slowest)) break;
  }
  if (rc != PW_OK || cands.empty()) {
    (void)hipDeviceSynchronize();
    for (Cand& c : cands) release_obs_buf(c.buf);
    return rc != PW_OK ? rc : pw_fail(PW_ENOMEM, "pw_obs_alloc_tuned: no candidate buffer");
  }
  (void)hipDeviceSynchronize();
  for (size_t i = 0; i < cands.size(); i++)
    if (i != best) release_obs_buf(cands[i].buf);  // the losers go back to the device
  e->obs_screen_ms = std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t_start).count();
  {  // the full tuner on the kept candidate; it leaves the observations of (puzzle_id, pos) in it
    RenderArgs ra;
    rc = fill_render_args(e, puzzle_id, pos, cands[best].buf.ptr, stride, batch, &ra);
    if (rc == PW_OK) rc = tune_render_impl(e, ra, batch, st, &cands[best].idx);
    if (rc == PW_OK && hipStreamSynchronize(st) != hipSuccess) rc = pw_fail(PW_EDEVICE, "pw_obs_alloc_tuned: stream error");
    if (rc != PW_OK) {
      release_obs_buf(cands[best].buf);
      return rc;
    }
  }
  *obs = cands[best].buf.ptr;
  const int tuned_index = cands[best].idx;
  e->obs_bufs.push_back(std::move(cands[best].buf));
  {  // the tuner left the buffer fully rendered: a bound batch may retain it from here on
    RenderArgs ra;
    if (fill_render_args(e, puzzle_id, pos, *obs, stride, batch, &ra) == PW_OK) retained_after_full_render(e, ra, batch);
  }
  return tuned_index;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

}  // extern "C"

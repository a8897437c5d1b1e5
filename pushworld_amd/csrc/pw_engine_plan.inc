// pw_engine_plan.inc -- the engine's small reads and the single-state API: pw_engine_bad_actions, pw_counters / _reset, the
// latency path (a stream, a pinned result block and its completion word; pw_cpu_relax), plan_launch, pw_next_state,
// pw_plan_states and pw_validate_state.  Part of the single translation unit pw_kernels.hip, included after pw_engine.inc:
// uses the kernels of pw_step_kernels.inc and check_launch, nothing of the other engine files.

extern "C" {

int64_t pw_engine_bad_actions(PwEngine* e, void* stream) try {
  if (!e) return pw_fail(PW_EINVAL, "null engine");
  PwDeviceGuard guard(e->set->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  uint32_t n = 0;
  hipError_t err = hipMemcpyAsync(&n, e->d_scratch + 4, 4, hipMemcpyDeviceToHost, st);
  if (err == hipSuccess) err = hipMemsetAsync(e->d_scratch + 4, 0, 4, st);
  if (err == hipSuccess) err = hipStreamSynchronize(st);
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string("pw_engine_bad_actions: ") + hipGetErrorString(err));
  e->bad_total += static_cast<int64_t>(n);
  return static_cast<int64_t>(n);
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_counters(PwEngine* e, int64_t out[PW_NUM_COUNTERS], void* stream) try {
  if (!e || !out) return pw_fail(PW_EINVAL, "null argument");
  PwDeviceGuard guard(e->set->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  std::vector<unsigned long long> host(static_cast<size_t>(PW_COUNTER_SLOTS) * 8, 0ull);
  uint32_t bad = 0;
  hipError_t err = hipMemcpyAsync(host.data(), e->d_counters, host.size() * 8, hipMemcpyDeviceToHost, st);
  if (err == hipSuccess) err = hipMemcpyAsync(&bad, e->d_scratch + 4, 4, hipMemcpyDeviceToHost, st);
  if (err == hipSuccess) err = hipStreamSynchronize(st);
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string("pw_counters: ") + hipGetErrorString(err));
  for (int k = 0; k < PW_NUM_COUNTERS; k++) out[k] = 0;
  for (int sl = 0; sl < PW_COUNTER_SLOTS; sl++)
    for (int k = 0; k < 3; k++) out[k] += static_cast<int64_t>(host[static_cast<size_t>(sl) * 8 + k]);
  out[3] = e->bad_total + static_cast<int64_t>(bad);
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_counters_reset(PwEngine* e, void* stream) try {
  if (!e) return pw_fail(PW_EINVAL, "null engine");
  PwDeviceGuard guard(e->set->device);
  if (hipMemsetAsync(e->d_counters, 0, PW_COUNTER_SLOTS * 64, static_cast<hipStream_t>(stream)) != hipSuccess)
    return pw_fail(PW_EDEVICE, "pw_counters_reset: hipMemsetAsync failed");
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

// ------------------------------------------------------------------------------------
// Latency path of the single-state API (pw_next_state / pw_plan_states)
// ------------------------------------------------------------------------------------
// (device guard held by the caller) stream, pinned + mapped result buffer of at least `bytes`
static int lat_prepare(PwEngine* e, size_t bytes) {
  if (!e->lat_stream && hipStreamCreateWithFlags(&e->lat_stream, hipStreamNonBlocking) != hipSuccess) {
    e->lat_stream = nullptr;
    return pw_fail(PW_EDEVICE, "pw_next_state: hipStreamCreate failed");
  }
  if (e->lat_bytes >= bytes) return PW_OK;
  if (e->lat_host) (void)hipHostFree(e->lat_host);
  e->lat_host = nullptr;
  e->lat_dev = nullptr;
  e->lat_bytes = 0;
  const size_t want = std::max<size_t>(bytes, size_t(1) << 16);
  if (hipHostMalloc(&e->lat_host, want, hipHostMallocMapped) != hipSuccess) {
    e->lat_host = nullptr;
    return pw_fail(PW_ENOMEM, "pw_next_state: cannot allocate pinned host memory");
  }
  if (hipHostGetDevicePointer(&e->lat_dev, e->lat_host, 0) != hipSuccess) {
    (void)hipHostFree(e->lat_host);
    e->lat_host = nullptr;
    return pw_fail(PW_EDEVICE, "pw_next_state: hipHostGetDevicePointer failed");
  }
  memset(e->lat_host, 0, 64);
  e->lat_bytes = want;
  return PW_OK;
}

static inline void pw_cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
  __builtin_ia32_pause();
#elif defined(__aarch64__)
  asm volatile("yield" ::: "memory");
#else
  std::this_thread::yield();
#endif
}

// waits for the completion word of launch `seq` (the kernel's last store, system scope, after everything else it wrote)
static int lat_wait(PwEngine* e, uint32_t seq, const char* what) {
  volatile uint32_t* word = static_cast<volatile uint32_t*>(e->lat_host);
  const auto t0 = std::chrono::steady_clock::now();
  for (uint32_t spins = 0;; spins++) {
    if (*word == seq) return PW_OK;
    pw_cpu_relax();
    if ((spins & 0xfffu) == 0xfffu) {
      // a kernel that has not answered within two seconds has failed (or the launch was lost): ask the runtime
      if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) {
        const hipError_t err = hipStreamSynchronize(e->lat_stream);
        if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string(what) + ": " + hipGetErrorString(err));
        if (*word == seq) return PW_OK;
        return pw_fail(PW_EDEVICE, std::string(what) + ": the kernel finished without reporting");
      }
    }
  }
}

static int plan_launch(PwEngine* e, int32_t puzzle, const int8_t* xy_start, const uint8_t* actions, int32_t num_actions,
                       int32_t single_action, int8_t* states_out, uint8_t* goal_out, int8_t* dev_states, int32_t* info,
                       const char* what) {
  const PwPuzzleHeader& h = e->set->headers[static_cast<size_t>(puzzle)];
  const int N = h.N;
  const size_t T = static_cast<size_t>(num_actions);
  const size_t off_actions = 64, off_states = off_actions + ((T + 63) & ~size_t(63));
  const size_t off_goals = off_states + (((T + 1) * N * 2 + 63) & ~size_t(63));
  const size_t total = off_goals + ((T + 1 + 63) & ~size_t(63));
  // (ctypes releases the GIL: two host threads may call the single-state API of one engine at once)
  std::lock_guard<std::mutex> lat_lock(e->lat_mu);
  PwDeviceGuard guard(e->set->device);
  if (int rc = lat_prepare(e, total)) return rc;
  uint8_t* host = static_cast<uint8_t*>(e->lat_host);
  PlanArgs a;
  a.hdrs = e->set->d_headers;
  a.blob = e->set->d_blob;
  a.puzzle = puzzle;
  a.num_actions = num_actions;
  a.action = single_action;
  a.out = static_cast<uint8_t*>(e->lat_dev);
  a.off_actions = static_cast<uint32_t>(off_actions);
  a.off_states = static_cast<uint32_t>(off_states);
  a.off_goals = static_cast<uint32_t>(off_goals);
  a.dev_states = reinterpret_cast<uint16_t*>(dev_states);
  a.np = e->np;
  for (int j = 0; j < 32; j++) {
    int x = 0, y = 0;
    if (j < N) {
      x = xy_start ? xy_start[2 * j] : h.init[j][0];
      y = xy_start ? xy_start[2 * j + 1] : h.init[j][1];
    }
    a.xy[j] = static_cast<uint16_t>((x & 0xff) | ((y & 0xff) << 8));
  }
  if (actions) memcpy(host + off_actions, actions, T);
  a.seq = ++e->lat_seq;
  if (a.seq == 0u) a.seq = ++e->lat_seq;  // (0 is what a fresh buffer holds)
  hipLaunchKernelGGL(pw_plan_kernel, dim3(1), dim3(64), 0, e->lat_stream, a);
  if (int rc = check_launch(what)) return rc;
  if (int rc = lat_wait(e, a.seq, what)) return rc;
  if (states_out) memcpy(states_out, host + off_states, (T + 1) * N * 2);
  if (goal_out) memcpy(goal_out, host + off_goals, T + 1);
  if (info) memcpy(info, host + 16, 16);
  return PW_OK;
}

int pw_next_state(PwEngine* e, int32_t puzzle, const int8_t* xy_in, int32_t action, int8_t* xy_out, int32_t* info) try {
  if (!e) return pw_fail(PW_EINVAL, "null engine");
  if (puzzle < 0 || puzzle >= e->set->count) return pw_fail(PW_EINVAL, "puzzle index out of range");
  if (!xy_in || !xy_out) return pw_fail(PW_EINVAL, "null argument");
  if (action < 0 || action > 3) return pw_fail(PW_EINVAL, "action must be one of 0 (L), 1 (R), 2 (U), 3 (D)");
  const int N = e->set->headers[static_cast<size_t>(puzzle)].N;
  int8_t both[2 * 32 * 2];
  const int rc = plan_launch(e, puzzle, xy_in, nullptr, 1, action, both, nullptr, nullptr, info, "pw_next_state");
  if (rc != PW_OK) return rc;
  memcpy(xy_out, both + 2 * N, static_cast<size_t>(2 * N));
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_plan_states(PwEngine* e, int32_t puzzle, const int8_t* xy_start, const uint8_t* actions, int32_t num_actions,
                   int8_t* states_out, uint8_t* goal_out, int8_t* dev_states) try {
  if (!e) return pw_fail(PW_EINVAL, "null engine");
  if (puzzle < 0 || puzzle >= e->set->count) return pw_fail(PW_EINVAL, "puzzle index out of range");
  if (num_actions < 0 || num_actions > PW_PLAN_MAX_ACTIONS) return pw_fail(PW_EINVAL, "num_actions must be 0 .. PW_PLAN_MAX_ACTIONS");
  if (num_actions > 0 && !actions) return pw_fail(PW_EINVAL, "null argument");
  for (int32_t t = 0; t < num_actions; t++)
    if (actions[t] > 3) return pw_fail(PW_EINVAL, "action must be one of 0 (L), 1 (R), 2 (U), 3 (D)");
  return plan_launch(e, puzzle, xy_start, actions, num_actions, -1, states_out, goal_out, dev_states, nullptr, "pw_plan_states");
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int64_t pw_validate_state(PwEngine* e, const int32_t* puzzle_id, const int8_t* pos, int32_t batch, int32_t* first_bad,
                          void* stream) try {
  if (!e) return pw_fail(PW_EINVAL, "null engine");
  if (first_bad) *first_bad = -1;
  if (batch <= 0) return 0;
  if (!puzzle_id) return pw_fail(PW_EINVAL, "null argument");
  PwDeviceGuard guard(e->set->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  uint32_t init[2] = {0u, 0xFFFFFFFFu};
  hipError_t err = hipMemcpyAsync(e->d_scratch, init, sizeof(init), hipMemcpyHostToDevice, st);
  if (err == hipSuccess) err = hipStreamSynchronize(st);  // `init` is a stack variable
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string("pw_validate_state: ") + hipGetErrorString(err));
  ValidateArgs a{e->set->d_headers, puzzle_id, pos, e->d_scratch, batch, e->np, e->set->count};
  hipLaunchKernelGGL(pw_validate_kernel, dim3((batch + 255) / 256), dim3(256), 0, st, a);
  if (int rc = check_launch("pw_validate_state")) return rc;
  uint32_t res[2] = {0u, 0u};
  err = hipMemcpyAsync(res, e->d_scratch, sizeof(res), hipMemcpyDeviceToHost, st);
  if (err == hipSuccess) err = hipStreamSynchronize(st);
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string("pw_validate_state: ") + hipGetErrorString(err));
  if (first_bad && res[0]) *first_bad = static_cast<int32_t>(res[1]);
  return static_cast<int64_t>(res[0]);
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

}  // extern "C"

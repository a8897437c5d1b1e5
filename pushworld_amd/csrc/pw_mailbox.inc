// pw_mailbox_*: host side of the resident step kernel (pw_mailbox_kernel, K1f in pw_mailbox_kernels.inc).
// Included by pw_kernels.hip after the engine files it uses: pw_engine_step.inc (fill_step_args, attach_binding, bound_all) and
// pw_engine_plan.inc (pw_cpu_relax); before pw_engine_options.inc, which asks mailbox_form_of.

struct PwMailbox {
  PwEngine* e;
  hipStream_t stream;
  uint8_t* host;        // pinned block: [0, 64) done + status | slots | action staging | results
  uint8_t* dev;         // the device's address of it
  size_t bytes;
  uint32_t* d_arrive;
  int32_t batch;
  uint32_t ring;
  size_t off_slots, off_stage, stage_stride, off_results, result_stride, off_term, off_trunc;
  uint64_t posted;      // steps posted so far
  int32_t idle_ms;
  std::chrono::steady_clock::time_point last_post;
  bool expired;         // the kernel has ended (or is about to) without pw_mailbox_close
  bool seg_form;        // the resident kernel runs the segments of a bound batch (pw_mailbox_seg_kernel)
  int clock_khz;        // the device's constant clock (wall_clock64)
};

static int mailbox_form_of(const PwEngine* e) { return e->mailbox ? (static_cast<const PwMailbox*>(e->mailbox)->seg_form ? 2 : 1) : 0; }

static volatile unsigned long long* mailbox_done(const PwMailbox* m) { return reinterpret_cast<volatile unsigned long long*>(m->host); }

static void mailbox_stop(PwMailbox* m) {
  volatile unsigned long long* slots = reinterpret_cast<volatile unsigned long long*>(m->host + m->off_slots);
  for (uint32_t i = 0; i < m->ring; i++) slots[i] = PW_MAILBOX_STOP;
  __atomic_thread_fence(__ATOMIC_SEQ_CST);
}

// waits until `seq` steps are complete; PW_EDEVICE when the kernel ended first / does not answer
static int mailbox_wait(PwMailbox* m, uint64_t seq, const char* what) {
  volatile unsigned long long* done = mailbox_done(m);
  if (done[0] >= seq) return PW_OK;
  const auto t0 = std::chrono::steady_clock::now();
  for (uint32_t spins = 0;; spins++) {
    if (done[0] >= seq) return PW_OK;
    pw_cpu_relax();
    if ((spins & 0x3ffu) == 0x3ffu) {
      if (done[1] != 0ull) {  // the kernel has ended
        if (done[0] >= seq) return PW_OK;
        m->expired = true;
        return pw_fail(PW_EDEVICE, std::string(what) + (done[1] == 3ull ? ": the mailbox kernel gave up waiting (idle limit) before this step"
                                                                         : ": the mailbox kernel was stopped before this step"));
      }
      if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(m->idle_ms) + std::chrono::seconds(2)) {
        m->expired = true;
        mailbox_stop(m);
        return pw_fail(PW_EDEVICE, std::string(what) + ": the mailbox kernel does not answer");
      }
    }
  }
}

int pw_mailbox_open(PwEngine* e, const int32_t* puzzle_id, int8_t* pos, int32_t* steps, double* reward, int8_t* dgoals,
                    uint8_t* terminated, uint8_t* truncated, int32_t batch, uint32_t flags, int32_t ring, int32_t idle_ms,
                    PwMailbox** out) try {
  if (!e || !out) return pw_fail(PW_EINVAL, "null argument");
  *out = nullptr;
  if (e->mailbox) return pw_fail(PW_EINVAL, "pw_mailbox_open: this engine has an open mailbox");
  if (batch <= 0 || batch > 65536) return pw_fail(PW_EINVAL, "pw_mailbox_open: batch must be 1 .. 65536 (every workgroup must be resident)");
  if (ring == 0) ring = 8;
  if (ring < 2 || ring > 64 || (ring & (ring - 1)) != 0) return pw_fail(PW_EINVAL, "pw_mailbox_open: ring must be a power of two, 2 .. 64");
  if (idle_ms == 0) idle_ms = 1000;
  if (idle_ms < 10 || idle_ms > 60000) return pw_fail(PW_EINVAL, "pw_mailbox_open: idle_ms must be 10 .. 60000");
  StepArgs a;
  if (int rc = fill_step_args(e, puzzle_id, reinterpret_cast<const uint8_t*>(pos) /* (not used: not NULL) */, pos, steps, reward, dgoals,
                              terminated, truncated, batch, flags, &a))
    return rc;
  a.actions = nullptr;
  attach_binding(e, &a);  // (a bound batch: the segment form below)
  PwDeviceGuard guard(e->set->device);
  std::unique_ptr<PwMailbox> m(new PwMailbox());
  m->e = e;
  m->stream = nullptr;
  m->host = nullptr;
  m->d_arrive = nullptr;
  m->batch = batch;
  m->ring = static_cast<uint32_t>(ring);
  m->posted = 0;
  m->idle_ms = idle_ms;
  m->expired = false;
  const size_t B64 = (static_cast<size_t>(batch) + 63) & ~size_t(63);
  m->off_slots = 64;
  m->off_stage = m->off_slots + ((static_cast<size_t>(ring) * 8 + 63) & ~size_t(63));
  m->stage_stride = B64;
  m->off_results = m->off_stage + m->stage_stride * static_cast<size_t>(ring);
  m->off_term = B64 * 8;
  m->off_trunc = B64 * 9;
  m->result_stride = B64 * 10;
  m->bytes = m->off_results + m->result_stride * static_cast<size_t>(ring);
  auto fail = [&](int code, const std::string& msg) {
    if (m->d_arrive) (void)hipFree(m->d_arrive);
    if (m->host) (void)hipHostFree(m->host);
    if (m->stream) (void)hipStreamDestroy(m->stream);
    return pw_fail(code, msg);
  };
  if (hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking) != hipSuccess) {
    m->stream = nullptr;
    return fail(PW_EDEVICE, "pw_mailbox_open: hipStreamCreate failed");
  }
  void* hp = nullptr;
  if (hipHostMalloc(&hp, m->bytes, hipHostMallocMapped) != hipSuccess) return fail(PW_ENOMEM, "pw_mailbox_open: cannot allocate pinned host memory");
  m->host = static_cast<uint8_t*>(hp);
  void* dp = nullptr;
  if (hipHostGetDevicePointer(&dp, hp, 0) != hipSuccess) return fail(PW_EDEVICE, "pw_mailbox_open: hipHostGetDevicePointer failed");
  m->dev = static_cast<uint8_t*>(dp);
  memset(m->host, 0, m->bytes);
  // the segment form (a bound batch whose every environment sits in a segment, the pipelined mode): workgroup = segment; all of them
  // -- and the relay's and the publisher's -- must be resident at once
  const bool boards = e->d_boards != nullptr && e->np <= 8 && e->step_boards != 2;
  bool seg_form = (e->mailbox_mode & 15) == 11 && bound_all(e, a) && !boards && e->mailbox_seg != 2;
  unsigned nseg = 0;
  size_t seg_lds = 0;
  if (seg_form) {
    nseg = static_cast<unsigned>(e->bind->seg_grid);
    seg_lds = (e->bind->lds_bytes + 15u) & ~size_t(15);
    int per_cu = 0, cus = 0;
    const void* fn = e->np <= 4 ? reinterpret_cast<const void*>(pw_mailbox_seg_kernel<4>)
                     : e->np <= 8 ? reinterpret_cast<const void*>(pw_mailbox_seg_kernel<8>)
                     : e->np <= 16 ? reinterpret_cast<const void*>(pw_mailbox_seg_kernel<16>)
                                   : reinterpret_cast<const void*>(pw_mailbox_seg_kernel<32>);
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, PW_SEG_ENVS, seg_lds) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, e->set->device) != hipSuccess ||
        static_cast<long long>(per_cu) * cus < static_cast<long long>(nseg) + 2 || nseg == 0 || nseg > 4096)
      seg_form = false;
  }
  const size_t prog_words = seg_form ? static_cast<size_t>(nseg) * 4 : 1024;
  const size_t dev_bytes = 64 * sizeof(uint32_t) + 64 * 8 + (prog_words + 1) * 8;
  if (hipMalloc(reinterpret_cast<void**>(&m->d_arrive), dev_bytes) != hipSuccess) {
    m->d_arrive = nullptr;
    return fail(PW_ENOMEM, "pw_mailbox_open: hipMalloc failed");
  }
  // ON THE KERNEL'S STREAM: a fill queued on the null stream is not ordered against m->stream (a non-blocking stream), and what
  // hipMalloc hands out may hold the relay words of an earlier mailbox -- of this process or of one before it --, numbers and stale
  // action addresses included: a wavefront that met such a word before the fill read its actions from an address that is gone
  // (a memory access fault in one bench run of this round, at a host address)
  if (hipMemsetAsync(m->d_arrive, 0, dev_bytes, m->stream) != hipSuccess) return fail(PW_EDEVICE, "pw_mailbox_open: hipMemsetAsync failed");
  m->clock_khz = pw_wall_clock_khz(e->set->device);
  MailboxArgs k;
  k.s = a;
  k.slots = reinterpret_cast<const unsigned long long*>(m->dev + m->off_slots);
  k.done = reinterpret_cast<unsigned long long*>(m->dev);
  k.arrive = m->d_arrive;
  k.results = m->dev + m->off_results;
  k.result_stride = static_cast<uint32_t>(m->result_stride);
  k.off_term = static_cast<uint32_t>(m->off_term);
  k.off_trunc = static_cast<uint32_t>(m->off_trunc);
  k.ring = m->ring;
  k.relay = reinterpret_cast<unsigned long long*>(m->d_arrive + 64);
  k.prog = k.relay + 64;  // [prog_words]: one word per stepping wavefront (65 536 environments one lane each = 1 024; the segment form: 4 per segment)
  k.prog_end = k.prog + prog_words;
  k.mode = static_cast<uint32_t>(e->mailbox_mode);
  const unsigned groups = seg_form ? nseg : static_cast<unsigned>((batch + 255) / 256);
  k.waves = groups * 4u;
  k.groups = groups;
  const unsigned grid = groups + ((k.mode & 3u) == 3u ? 1u : 0u) + ((k.mode & 11u) == 11u ? 1u : 0u);  // (+ the relay, + the publisher)
  k.idle_ticks = static_cast<unsigned long long>(m->clock_khz) * static_cast<unsigned long long>(idle_ms);
  // (the caller's stream order ends here: what it queued on its stream for these arrays must be complete -- the wrappers
  // synchronise their stream before they open a mailbox)
  // sets of 8 x 8 puzzles: the whole-grid boards (what pw_step launches for them); any other set: one lane per environment
  // over its overlap tables where every puzzle has them, over the row bitboards otherwise
  const dim3 g(grid), b(256);
  const bool tables = e->ovl_puzzles > 0 && e->ovl_puzzles == e->set->count;
#define PW_MB(NP)                                                                                          \
  do {                                                                                                     \
    if (tables) hipLaunchKernelGGL((pw_mailbox_kernel<NP, MailboxLanes<NP, 2>>), g, b, 0, m->stream, k);   \
    else hipLaunchKernelGGL((pw_mailbox_kernel<NP, MailboxLanes<NP, 0>>), g, b, 0, m->stream, k);          \
  } while (0)
  m->seg_form = seg_form;
  if (seg_form) {
    if (e->np <= 4) hipLaunchKernelGGL(pw_mailbox_seg_kernel<4>, g, b, seg_lds, m->stream, k);
    else if (e->np <= 8) hipLaunchKernelGGL(pw_mailbox_seg_kernel<8>, g, b, seg_lds, m->stream, k);
    else if (e->np <= 16) hipLaunchKernelGGL(pw_mailbox_seg_kernel<16>, g, b, seg_lds, m->stream, k);
    else hipLaunchKernelGGL(pw_mailbox_seg_kernel<32>, g, b, seg_lds, m->stream, k);
  } else if (boards && e->np <= 4) hipLaunchKernelGGL((pw_mailbox_kernel<4, MailboxBoards<4>>), g, b, 0, m->stream, k);
  else if (boards) hipLaunchKernelGGL((pw_mailbox_kernel<8, MailboxBoards<8>>), g, b, 0, m->stream, k);
  else if (e->np <= 4) PW_MB(4);
  else if (e->np <= 8) PW_MB(8);
  else if (e->np <= 16) PW_MB(16);
  else PW_MB(32);
#undef PW_MB
  if (int rc = check_launch("pw_mailbox_open")) {
    (void)fail(rc, pw_last_error());
    return rc;
  }
  m->last_post = std::chrono::steady_clock::now();
  e->mailbox = m.get();
  *out = m.release();
  return PW_OK;
} catch (...) {
  return pw_current_exception();
}

int pw_mailbox_post(PwMailbox* m, const uint8_t* actions, int32_t actions_on_host, uint64_t* seq) try {
  if (!m || !actions) return pw_fail(PW_EINVAL, "null argument");
  if (m->expired) return pw_fail(PW_EDEVICE, "pw_mailbox_post: this mailbox has expired (close it and open a new one)");
  const auto now = std::chrono::steady_clock::now();
  if (now - m->last_post > std::chrono::milliseconds(m->idle_ms / 2)) {
    // the kernel gives up after idle_ms without a post: from half of that on nothing more is posted, so the two cannot race
    m->expired = true;
    mailbox_stop(m);
    return pw_fail(PW_EDEVICE, "pw_mailbox_post: more than half of the idle limit has passed since the last post; the mailbox has expired");
  }
  const uint64_t k = m->posted + 1;
  if (k > mailbox_done(m)[0] + m->ring) {  // the slot (and its result slot) is still in use by step k - ring
    if (int rc = mailbox_wait(m, k - m->ring, "pw_mailbox_post")) return rc;
  }
  const uint32_t slot = static_cast<uint32_t>((k - 1) & (m->ring - 1));
  uint64_t addr;
  if (actions_on_host) {
    memcpy(m->host + m->off_stage + slot * m->stage_stride, actions, static_cast<size_t>(m->batch));
    addr = reinterpret_cast<uint64_t>(m->dev + m->off_stage + slot * m->stage_stride);
  } else {
    addr = reinterpret_cast<uint64_t>(actions);
  }
  if (addr >> 48) return pw_fail(PW_EINVAL, "pw_mailbox_post: address beyond 48 bits");
  __atomic_thread_fence(__ATOMIC_RELEASE);
  reinterpret_cast<volatile unsigned long long*>(m->host + m->off_slots)[slot] = ((k & 0xffffull) << 48) | addr;
  __atomic_thread_fence(__ATOMIC_SEQ_CST);
  m->posted = k;
  m->last_post = now;
  if (seq) *seq = k;
  return PW_OK;
} catch (...) {
  return pw_current_exception();
}

int pw_mailbox_wait(PwMailbox* m, uint64_t seq, const double** reward, const uint8_t** terminated, const uint8_t** truncated) try {
  if (!m) return pw_fail(PW_EINVAL, "null argument");
  if (seq == 0 || seq > m->posted) return pw_fail(PW_EINVAL, "pw_mailbox_wait: no such step");
  if (int rc = mailbox_wait(m, seq, "pw_mailbox_wait")) return rc;
  __atomic_thread_fence(__ATOMIC_ACQUIRE);
  const uint8_t* rs = m->host + m->off_results + ((seq - 1) & (m->ring - 1)) * m->result_stride;
  if (reward) *reward = reinterpret_cast<const double*>(rs);
  if (terminated) *terminated = rs + m->off_term;
  if (truncated) *truncated = rs + m->off_trunc;
  return PW_OK;
} catch (...) {
  return pw_current_exception();
}

// post + wait in one call (a foreign-function call costs the Python wrappers ~1 us each)
int pw_mailbox_step(PwMailbox* m, const uint8_t* actions, int32_t actions_on_host, uint64_t* seq) try {
  uint64_t k = 0;
  if (int rc = pw_mailbox_post(m, actions, actions_on_host, &k)) return rc;
  if (seq) *seq = k;
  return mailbox_wait(m, k, "pw_mailbox_step");
} catch (...) {
  return pw_current_exception();
}

// where the verdicts of step `seq` are: base + ((seq - 1) mod ring) * stride; reward float64 [B] at 0, terminated / truncated uint8 [B]
int pw_mailbox_layout(PwMailbox* m, const uint8_t** base, int64_t* stride, int64_t* off_terminated, int64_t* off_truncated, int32_t* ring) {
  if (!m) return pw_fail(PW_EINVAL, "null argument");
  if (base) *base = m->host + m->off_results;
  if (stride) *stride = static_cast<int64_t>(m->result_stride);
  if (off_terminated) *off_terminated = static_cast<int64_t>(m->off_term);
  if (off_truncated) *off_truncated = static_cast<int64_t>(m->off_trunc);
  if (ring) *ring = static_cast<int32_t>(m->ring);
  return PW_OK;
}

// T steps from one [T][B] action array: at most `ahead` steps in flight (0 or 1: every step waits for the one before -- the
// cadence of a host that needs a step's verdicts to choose the next actions); returns when all are complete
int pw_mailbox_run(PwMailbox* m, const uint8_t* actions, int32_t num_steps, int32_t actions_on_host, int32_t ahead, uint64_t* last_seq) try {
  if (!m || !actions) return pw_fail(PW_EINVAL, "null argument");
  if (num_steps < 0) return pw_fail(PW_EINVAL, "pw_mailbox_run: num_steps must be >= 0");
  if (ahead < 1) ahead = 1;
  uint64_t seq = m->posted;
  for (int32_t t = 0; t < num_steps; t++) {
    if (int rc = pw_mailbox_post(m, actions + static_cast<size_t>(t) * static_cast<size_t>(m->batch), actions_on_host, &seq)) return rc;
    if (seq >= static_cast<uint64_t>(ahead))
      if (int rc = mailbox_wait(m, seq - static_cast<uint64_t>(ahead) + 1, "pw_mailbox_run")) return rc;
  }
  if (num_steps > 0)
    if (int rc = mailbox_wait(m, seq, "pw_mailbox_run")) return rc;
  if (last_seq) *last_seq = seq;
  return PW_OK;
} catch (...) {
  return pw_current_exception();
}

// profile (optional, int64 [8]): [0] steps completed, [1] how the kernel ended (2 stop word, 3 idle limit), [2..6] ticks of the
// device's constant clock that wavefront 0 spent waiting for the word / reading its actions / stepping / storing / counting
// itself in, [7] that clock's kHz
int pw_mailbox_close_profile(PwMailbox* m, int64_t* profile) try {
  if (!m) return PW_OK;
  PwDeviceGuard guard(m->e->set->device);
  int rc = PW_OK;
  if (!m->expired && m->posted > 0) rc = mailbox_wait(m, m->posted, "pw_mailbox_close");  // (every posted step ends in every wavefront)
  mailbox_stop(m);
  const hipError_t err = hipStreamSynchronize(m->stream);  // (at most the idle limit)
  if (err != hipSuccess && rc == PW_OK) rc = pw_fail(PW_EDEVICE, std::string("pw_mailbox_close: ") + hipGetErrorString(err));
  if (profile) {
    volatile unsigned long long* d = mailbox_done(m);
    for (int i = 0; i < 7; i++) profile[i] = static_cast<int64_t>(d[i]);
    profile[7] = m->clock_khz;
  }
  (void)hipStreamDestroy(m->stream);
  (void)hipFree(m->d_arrive);
  (void)hipHostFree(m->host);
  m->e->mailbox = nullptr;
  delete m;
  return rc;
} catch (...) {
  return pw_current_exception();
}

int pw_mailbox_close(PwMailbox* m) { return pw_mailbox_close_profile(m, nullptr); }

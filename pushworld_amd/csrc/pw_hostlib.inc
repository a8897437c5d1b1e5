// pw_hostlib.inc -- the host plumbing that the search, table and planner handles share: how a HIP error becomes a library
// error, chained allocations, the argument checks several entry points make in the same words, the engine-owned search slab,
// and the parts of a handle that owns its slabs (slab pool, cancel word, wall-clock rate).  Host code only: nothing here is
// __global__ or __device__.  Part of the single translation unit pw_kernels.hip, included before every file that launches.
//
// What is NOT here: the slab layouts (the chains of off_* fields mirror each kernel's argument struct and stay next to it)
// and whatever differs between two handles (that stays at the call sites, in plain sight).
#include "pw_hostlib_pure.h"

static int check_launch(const char* what) {
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string(what) + ": " + hipGetErrorString(err));
  return PW_OK;
}

// a failed allocation or a chain with one in it: PW_ENOMEM when the device ran out of memory, else PW_EDEVICE
static int pw_hip_code(hipError_t err) { return err == hipErrorOutOfMemory ? PW_ENOMEM : PW_EDEVICE; }
static int pw_hip_fail(const std::string& fn, hipError_t err) {
  return pw_fail(pw_hip_code(err), fn + ": " + hipGetErrorString(err));
}

// a failed copy, fill or synchronisation: PW_EDEVICE whatever the error
static int pw_hip_fail_device(const std::string& fn, hipError_t err) {
  return pw_fail(PW_EDEVICE, fn + ": " + hipGetErrorString(err));
}

// A chain of HIP calls that stops at the first error: every link is skipped once one has failed, and `err` says which.
//   PwHipChain c(guard.status());
//   c.alloc(&p, bytes);                          (hipMalloc, a zero size included: the policy is the caller's expression)
//   c.then([&] { return hipMemcpy(...); });      (any other call; not made after a failure)
//   if (!c.ok()) { release; return pw_hip_fail("fn", c.err); }
struct PwHipChain {
  hipError_t err;
  explicit PwHipChain(hipError_t first = hipSuccess) : err(first) {}
  bool ok() const { return err == hipSuccess; }
  template <class T>
  void alloc(T** p, size_t bytes) {
    if (ok()) err = hipMalloc(reinterpret_cast<void**>(p), bytes);
  }
  template <class T>
  void alloc_nonzero(T** p, size_t bytes) {  // nothing to do for an empty array: *p stays as it is
    if (bytes) alloc(p, bytes);
  }
  template <class F>
  void then(F&& call) {
    if (ok()) err = call();
  }
};

// prefix: what the message starts with ("pw_x: ", or "" where the entry point's messages carry no name)
static int pw_check_npad(const std::string& prefix, int32_t npad) {
  if (!pw_npad_ok(npad)) return pw_fail(PW_EINVAL, prefix + "npad must be 4, 8, 16 or 32");
  return PW_OK;
}

// every entry of a create call's `puzzles` list (NULL: 0 .. n - 1) names a puzzle of the engine's set
static bool pw_puzzles_ok(const PwEngine* e, const int32_t* puzzles, int32_t n) {
  for (int32_t i = 0; i < n; i++) {
    const int32_t pid = puzzles ? puzzles[i] : i;
    if (pid < 0 || pid >= e->set->count) return false;
  }
  return true;
}

// the handle item of each set index for the states forms, -1 = not prepared; of a puzzle listed twice the first wins
template <class Item>
static std::vector<int32_t> pw_slot_of(const std::vector<Item>& items, int32_t set_count) {
  std::vector<int32_t> slot_of(static_cast<size_t>(set_count), -1);
  for (size_t i = items.size(); i-- > 0;) slot_of[static_cast<size_t>(items[i].pid)] = static_cast<int32_t>(i);
  return slot_of;
}

// ticks per millisecond of wall_clock64() on `device`; 100 MHz where the runtime does not say
static uint32_t pw_wall_clock_khz(int device) {
  int khz = 0;
  if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device) != hipSuccess || khz <= 0) khz = 100000;
  return static_cast<uint32_t>(khz);
}

// ---- the engine-owned search slab (pw_search_batch, pw_solve_batch_run, pw_push_solve_batch_run) ---------------------------
// Persistent workgroups of a launch over n items with slab_bytes each: two per CU or PW_OPT_SEARCH_BATCH_GROUPS_PER_CU, fewer
// when there are fewer items or the slabs would not fit a quarter of the free memory.  The slabs are the engine's: grown on
// demand (after `st` has drained: an earlier launch on it may still use the old ones) and kept for the next call.
// *next is the item counter in front of the slabs.
static int engine_search_slab(PwEngine* e, int64_t n, uint64_t slab_bytes, hipStream_t st, const char* fn, int64_t* groups,
                              uint8_t** slab, uint32_t** next) {
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b == 0) free_b = total_b / 2;
  int64_t g = std::min<int64_t>(n, static_cast<int64_t>(e->search_batch_groups_per_cu > 0 ? e->search_batch_groups_per_cu : 2) * e->num_cus);
  const int64_t avail = static_cast<int64_t>(free_b / 4 + e->search_slab_bytes);
  g = std::max<int64_t>(1, std::min<int64_t>(g, avail / static_cast<int64_t>(slab_bytes)));
  const size_t want = static_cast<size_t>(g) * static_cast<size_t>(slab_bytes) + 256;
  if (e->search_slab_bytes < want) {
    if (hipStreamSynchronize(st) != hipSuccess) return pw_fail(PW_EDEVICE, std::string(fn) + ": stream error");
    if (e->d_search_slab) (void)hipFree(e->d_search_slab);
    e->d_search_slab = nullptr;
    e->search_slab_bytes = 0;
    if (hipMalloc(reinterpret_cast<void**>(&e->d_search_slab), want) != hipSuccess)
      return pw_fail(PW_ENOMEM, std::string(fn) + ": cannot allocate the search slabs");
    e->search_slab_bytes = want;
  }
  *groups = g;
  *slab = e->d_search_slab + 256;
  *next = reinterpret_cast<uint32_t*>(e->d_search_slab);
  return PW_OK;
}

// ---- handles that own their slabs (PwPlanBatch, PwPushPlanBatch) -------------------------------------------------------------
// One allocation: the item counter (256 B), then `groups` slabs of persistent workgroups.  Zero-filled: tag 0 is no item's, so
// the closed sets start empty.
struct PwSlabPool {
  uint8_t* d_slab;
  int64_t groups;
  uint64_t slab_bytes;
  uint8_t* slabs() const { return d_slab + 256; }
  uint32_t* counter() const { return reinterpret_cast<uint32_t*>(d_slab); }
  size_t bytes() const { return 256 + static_cast<size_t>(groups) * static_cast<size_t>(slab_bytes); }
};

// one workgroup per item up to two per CU, fewer when the slabs would not fit a quarter of the free memory
static void slab_pool_create(PwSlabPool* p, PwHipChain& c, int64_t n, int num_cus, uint64_t slab_bytes) {
  size_t free_b = 0, total_b = 0;
  if (c.ok() && (hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b == 0)) free_b = total_b / 2;
  p->slab_bytes = slab_bytes;
  p->groups = std::min<int64_t>(n, 2ll * num_cus);
  p->groups = std::max<int64_t>(1, std::min<int64_t>(p->groups, static_cast<int64_t>(free_b / 4 / slab_bytes)));
  c.alloc(&p->d_slab, p->bytes());
  c.then([&] { return hipMemset(p->d_slab, 0, p->bytes()); });
}

// A run of the states form may hold more items than the handle prepared puzzles: up to two workgroups per CU as memory allows.
// Replacing the slabs waits for the device once (a launch in flight on any stream still uses the old ones).  *replaced: the
// slabs are new and empty, and the caller resets what it keeps about the old ones.  A pool that cannot grow stays as it is
// (the launch runs on the workgroups it has).
static int slab_pool_grow(PwSlabPool* p, int64_t n, int num_cus, const char* fn, bool* replaced) {
  *replaced = false;
  const int64_t want = std::min<int64_t>(n, 2ll * num_cus);
  if (want <= p->groups) return PW_OK;
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return PW_OK;
  const int64_t fit = static_cast<int64_t>((free_b + static_cast<uint64_t>(p->groups) * p->slab_bytes) / 4 / p->slab_bytes);
  PwSlabPool fresh = {nullptr, std::min<int64_t>(want, fit), p->slab_bytes};
  if (fresh.groups <= p->groups) return PW_OK;
  if (hipMalloc(reinterpret_cast<void**>(&fresh.d_slab), fresh.bytes()) != hipSuccess) {
    (void)hipGetLastError();
    return PW_OK;
  }
  PwHipChain c(hipDeviceSynchronize());
  c.then([&] { return hipMemset(fresh.d_slab, 0, fresh.bytes()); });
  c.then([&] { return hipFree(p->d_slab); });
  if (!c.ok()) {
    (void)hipFree(fresh.d_slab);
    return pw_hip_fail_device(fn, c.err);
  }
  *p = fresh;
  *replaced = true;
  return PW_OK;
}

// The cancel word of a handle: 64 bytes of pinned host memory mapped into the device.  Word 0: every launch numbered up to it
// is cancelled (`seq` numbers the launches); word 1 is the push planner's generation.  Both start at 0.
struct PwCancelWord {
  int64_t* h;
  int64_t* d;  // the device's address of h
  int64_t seq;
};

static void cancel_word_create(PwCancelWord* w, PwHipChain& c) {
  c.then([&] { return hipHostMalloc(reinterpret_cast<void**>(&w->h), 64, hipHostMallocMapped); });
  c.then([&] {
    w->h[0] = w->h[1] = 0;
    return hipHostGetDevicePointer(reinterpret_cast<void**>(&w->d), w->h, 0);
  });
}

// every launch made so far, queued ones included
static void cancel_word_cancel(PwCancelWord* w) { __atomic_store_n(w->h, w->seq, __ATOMIC_RELEASE); }

static void cancel_word_destroy(PwCancelWord* w) {
  if (w->h) (void)hipHostFree(w->h);
  w->h = nullptr;
}

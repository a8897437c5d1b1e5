// pw_engine_render.inc -- the render launches of the engine: the profiling bracket of a launch (RenderProfScope), the page
// path and its records, the retained observation and its live-page list (PwRetained), launch_rowpage / launch_render, and the
// entry points that only render (pw_render, pw_render_retained).  Part of the single translation unit pw_kernels.hip, included
// after pw_engine.inc: uses fill_render_args from there, the kernels of pw_render_kernels.inc and check_launch.

extern "C" {

// PW_OPT_PROFILE_RENDER: one HIP event pair per render launch, recorded on the launch stream
struct RenderProfScope {
  PwEngine* e;
  hipStream_t st;
  int slot;
  RenderProfScope(PwEngine* eng, hipStream_t s) : e(eng), st(s), slot(-1) {
    if (e->prof_used < static_cast<int>(e->prof_events.size() / 2)) {
      slot = e->prof_used++;
      (void)hipEventRecord(e->prof_events[2 * slot], st);
    }
  }
  void close() {
    if (slot >= 0) (void)hipEventRecord(e->prof_events[2 * slot + 1], st);
    slot = -1;
  }
  ~RenderProfScope() { close(); }
};

static bool page_path(const PwEngine* e, int64_t env_stride) {
  // page kernel: a 4 KiB page may hold the tail of one environment and the head of the next, not
  // more -- observations smaller than a page take the per-environment LDS kernel
  if (e->force_lds_render || env_stride < 4096) return false;
  return (e->d_simg && e->simg_cached) || e->rowpage;
}

// Page records of `batch` environments (device guard held by the caller); false when out of memory.  Engine-owned
// scratch written by the step / record kernels and read by the page kernel of the SAME call: all calls on one engine
// go to one stream or are event-ordered by the caller (header contract).  Allocated by pw_obs_alloc for its batch, or
// here by the first render call of a batch size; a larger batch later re-allocates (hipFree synchronises the device,
// so nothing in flight still reads the old records) -- never inside a steady-state step loop.
static bool ensure_rec(PwEngine* e, int32_t batch) {
  if (e->rec_cap >= batch) return true;
  if (e->d_rec) (void)hipFree(e->d_rec);
  e->d_rec = nullptr;
  e->rec_cap = 0;
  if (hipMalloc(&e->d_rec, static_cast<size_t>(batch) * sizeof(PageRec)) != hipSuccess) return false;
  e->rec_cap = batch;
  return true;
}

// ---- the retained observation (PW_OPT_OBS_PADDING_ONCE, PwRetained) ---------------------------------------------------
static int64_t owned_obs_stride(const PwEngine* e) { return (e->obs_bytes + 511) & ~int64_t(511); }

// the ppc-3 page kernel renders such a batch in ONE launch, into a buffer with the stride of the library's own
static bool live_applies(const PwEngine* e, int64_t env_stride, int32_t batch) {
  if (!page_path(e, env_stride) || e->rowpage || e->force_fused || e->page_slice_envs > 0) return false;
  if (env_stride != owned_obs_stride(e)) return false;
  const uint64_t cpe = static_cast<uint64_t>(env_stride / 16);
  return static_cast<uint64_t>(batch) <= std::max<uint64_t>(1, ((1ull << 31) - 512) / cpe);
}

// Builds the live-page list of (puzzle_id, batch) on `st` (device guard held by the caller).  The length stays on the device
// (n_live = -1) until a caller that synchronises anyway copies it from d_count.  may_alloc: the caller is no steady-state
// path (hipFree of a smaller list synchronises the device, so nothing in flight still reads it).
static bool live_build(PwEngine* e, const int32_t* puzzle_id, int32_t batch, hipStream_t st, bool may_alloc) {
  PwRetained& r = e->ret;
  r.list_pid = nullptr;
  r.n_live = -1;
  const int64_t stride = owned_obs_stride(e);
  if (!live_applies(e, stride, batch)) return false;
  const uint32_t cpe = static_cast<uint32_t>(stride / 16);
  const uint32_t n_pages = static_cast<uint32_t>((static_cast<uint64_t>(batch) * cpe + 255) / 256);
  if (r.list_cap < static_cast<int64_t>(n_pages)) {
    if (!may_alloc) return false;
    if (r.d_live) (void)hipFree(r.d_live);
    r.d_live = nullptr;
    r.list_cap = 0;
    const size_t blk_cap = (static_cast<size_t>(n_pages) + 1023) / 1024;
    if (hipMalloc(reinterpret_cast<void**>(&r.d_live), (static_cast<size_t>(n_pages) + blk_cap + 4) * 4) != hipSuccess) {
      (void)hipGetLastError();  // no list: pw_step_render keeps rendering in full
      return false;
    }
    r.d_blk = r.d_live + n_pages;
    r.d_count = r.d_blk + blk_cap;
    r.list_cap = n_pages;
  }
  // the arrays of the changed-page launch live and die with the list (PW_OPT_OBS_CHANGED_PAGES): one allocation, changed [batch]
  // then shown [batch][N_pad][2].  Without them pw_step_render keeps the live launch.
  if (r.shown_cap < batch && may_alloc) {
    if (r.d_changed) (void)hipFree(r.d_changed);
    r.d_changed = nullptr;
    r.d_shown = nullptr;
    r.shown_cap = 0;
    r.shown_valid = false;
    const size_t bytes = static_cast<size_t>(batch) * (8 + static_cast<size_t>(e->np) * 2);
    if (hipMalloc(reinterpret_cast<void**>(&r.d_changed), bytes) == hipSuccess && hipMemsetAsync(r.d_changed, 0, bytes, st) == hipSuccess) {
      r.d_shown = reinterpret_cast<int8_t*>(r.d_changed + batch);
      r.shown_cap = batch;
    } else {
      (void)hipGetLastError();
      if (r.d_changed) (void)hipFree(r.d_changed);
      r.d_changed = nullptr;
    }
  }
  LiveArgs a;
  a.hdrs = e->set->d_headers;
  a.puzzle_id = puzzle_id;
  a.num_puzzles = e->set->count;
  a.batch = batch;
  a.pad_h = e->pad_h;
  a.pad_w = e->pad_w;
  a.chunks_per_env = cpe;
  a.n_chunks = static_cast<uint32_t>((e->obs_bytes + 15) / 16);
  a.n_pages = n_pages;
  a.n_blk = (n_pages + 1023u) / 1024u;
  a.blk = r.d_blk;
  a.live = r.d_live;
  a.count = r.d_count;
  if (e->page_f32) {
    hipLaunchKernelGGL(pw_live_count_kernel<4>, dim3(a.n_blk), dim3(256), 0, st, a);
    hipLaunchKernelGGL(pw_live_scan_kernel, dim3(1), dim3(1024), 0, st, a);
    hipLaunchKernelGGL(pw_live_fill_kernel<4>, dim3(a.n_blk), dim3(256), 0, st, a);
  } else {
    hipLaunchKernelGGL(pw_live_count_kernel<1>, dim3(a.n_blk), dim3(256), 0, st, a);
    hipLaunchKernelGGL(pw_live_scan_kernel, dim3(1), dim3(1024), 0, st, a);
    hipLaunchKernelGGL(pw_live_fill_kernel<1>, dim3(a.n_blk), dim3(256), 0, st, a);
  }
  r.list_pid = puzzle_id;
  r.list_batch = batch;
  r.n_pages = n_pages;
  return true;
}

static bool bound_to(const PwEngine* e, const int32_t* puzzle_id, int32_t batch) {
  return e->bind && e->bind->puzzle_id == puzzle_id && e->bind->batch == batch;
}

// something other than a render of the retained (puzzle_id, batch) wrote into [ra.obs, + batch * stride): where that meets the
// retained buffer, its padding is no longer known
static void retained_overwritten(PwEngine* e, const RenderArgs& ra, int32_t batch) {
  PwRetained& r = e->ret;
  if (!r.valid) return;
  const uintptr_t lo = reinterpret_cast<uintptr_t>(ra.obs), hi = lo + static_cast<uint64_t>(batch) * static_cast<uint64_t>(ra.env_stride);
  const uintptr_t rlo = reinterpret_cast<uintptr_t>(r.obs), rhi = rlo + static_cast<uint64_t>(r.batch) * static_cast<uint64_t>(r.stride);
  if (lo < rhi && rlo < hi) r.valid = r.shown_valid = false;
}

// a full render of (ra.puzzle_id, batch) into ra.obs establishes (or keeps) the retained observation
static bool retained_establishes(const PwEngine* e, const RenderArgs& ra, int32_t batch) {
  const PwRetained& r = e->ret;
  bool owned = false;
  for (const PwObsBuf& b : e->obs_bufs)
    owned = owned || (b.ptr == ra.obs && static_cast<uint64_t>(batch) * static_cast<uint64_t>(ra.env_stride) <= b.bytes);
  return r.option && owned && live_applies(e, ra.env_stride, batch) && bound_to(e, ra.puzzle_id, batch) && r.list_pid == ra.puzzle_id &&
         r.list_batch == batch;
}

// A full render of (ra.puzzle_id, batch) into ra.obs has been launched: it establishes the retained observation where the
// rule allows one (header, PW_OPT_OBS_PADDING_ONCE), and ends the validity of a retained buffer it wrote other bytes into.
static void retained_after_full_render(PwEngine* e, const RenderArgs& ra, int32_t batch) {
  PwRetained& r = e->ret;
  if (retained_establishes(e, ra, batch)) {
    if (!(r.valid && r.obs == ra.obs && r.stride == ra.env_stride && r.batch == batch && r.puzzle_id == ra.puzzle_id))
      r.shown_valid = false;  // (another buffer than `shown` speaks of; the caller sets it when this render's records filled `shown`)
    r.valid = true;
    r.obs = ra.obs;
    r.stride = ra.env_stride;
    r.batch = batch;
    r.puzzle_id = ra.puzzle_id;
    return;
  }
  retained_overwritten(e, ra, batch);
}

// pw_step_render may launch the live pages only: 0 no, 1 the list form, 2 the early-exit form
static int retained_live_form(const PwEngine* e, const RenderArgs& ra, int32_t batch) {
  const PwRetained& r = e->ret;
  if (!r.valid || !r.option || r.obs != ra.obs || r.stride != ra.env_stride || r.batch != batch || r.puzzle_id != ra.puzzle_id ||
      !bound_to(e, ra.puzzle_id, batch) || r.list_pid != ra.puzzle_id || r.list_batch != batch || !live_applies(e, ra.env_stride, batch))
    return 0;
  return r.option == 2 ? 2 : (r.option == 3 ? 1 : r.form);
}

// PW_OPT_OBS_CHANGED_PAGES: the record writers of a call compare its new state with PwRetained::d_shown (and leave it there) exactly
// when the call's render goes into the retained buffer of the retained (puzzle_id, batch), or establishes it -- so that `shown` is
// what that buffer shows after every such call, whatever happened to `pos` in between.
static bool retained_tracks(const PwEngine* e, const RenderArgs& ra, int32_t batch, int live_form) {
  const PwRetained& r = e->ret;
  return r.chg_option && r.d_changed && r.shown_cap >= batch && (live_form != 0 || retained_establishes(e, ra, batch));
}

// the launch of a call whose record writer compared the new state with a valid `shown`: the changed pages (3), or with
// pw_engine_set_obs_changed_rows the changed pixel rows (4)
static int retained_changed_form(const PwEngine* e) { return e->ret.rows_option ? 4 : 3; }

static void launch_rowpage(PwEngine* e, const RenderArgs& ra, int32_t batch, hipStream_t st) {
  const uint32_t cpe = static_cast<uint32_t>(ra.env_stride / 16);
  int32_t max_envs = static_cast<int32_t>(std::max<uint64_t>(1, ((1ull << 31) - 512) / cpe));
  if (e->page_slice_envs > 0) max_envs = static_cast<int32_t>(std::min<int64_t>(max_envs, e->page_slice_envs));
  for (int32_t first = 0; first < batch; first += max_envs) {
    const int32_t nb = std::min(max_envs, batch - first);
    RenderArgs rp = ra;
    rp.puzzle_id = ra.puzzle_id + first;
    rp.pos = ra.pos + static_cast<int64_t>(first) * ra.np * 2;
    rp.obs = ra.obs + static_cast<int64_t>(first) * ra.env_stride;
    rp.batch = nb;
    RowPageArgs pa;
    pa.srow = e->d_srow;
    pa.srow_stride = e->srow_stride;
    pa.pitch = static_cast<uint32_t>(e->srow_pitch);
    pa.zero_row = static_cast<uint32_t>(3 * e->set->max_h);
    pa.rec = static_cast<const PageRec*>(e->d_rec) + first;
    pa.chunks_per_env = cpe;
    pa.n_chunks = static_cast<uint32_t>((e->obs_bytes + 15) / 16);
    pa.inv_cpe = 1.0f / static_cast<float>(cpe);
    pa.row_bytes = static_cast<uint32_t>(e->row_bytes);
    pa.cpr = static_cast<uint32_t>(e->row_bytes / 16);
    pa.magic_cpr = pa.cpr ? static_cast<uint32_t>(((1ull << 32) + pa.cpr - 1) / pa.cpr) : 0u;
    pa.magic_row = ~0ull / static_cast<uint64_t>(e->row_bytes) + 1ull;  // ceil(2^64 / row bytes): row bytes is no power of two >= 2^64
    const uint64_t ppc = static_cast<uint64_t>(e->cfg.pixels_per_cell);
    pa.magic_ppc = static_cast<uint32_t>(((1ull << 32) + ppc - 1) / ppc);
    pa.n_pages = static_cast<uint32_t>((static_cast<uint64_t>(nb) * cpe + 255) / 256);
    pa.order = static_cast<uint32_t>(e->page_order);
    pa.run_log2 = static_cast<uint32_t>(pa.order == 1u ? std::min(e->page_run_log2, 3) : e->page_run_log2);
    const dim3 grid(page_grid(pa.n_pages, pa.order, pa.run_log2));
    const size_t lds_pad = static_cast<size_t>(e->page_lds_pad_kb) * 1024;
    const int variant = (e->cfg.obs_dtype == PW_OBS_F32 ? 4 : 0) | (e->rowpage_aligned ? 2 : 0) | (e->tuning ? 1 : 0);
    switch (variant) {
      case 0: hipLaunchKernelGGL((pw_render_rowpage_kernel<uint8_t, false, 0>), grid, dim3(64), lds_pad, st, rp, pa); break;
      case 1: hipLaunchKernelGGL((pw_render_rowpage_kernel<uint8_t, false, 1>), grid, dim3(64), lds_pad, st, rp, pa); break;
      case 2: hipLaunchKernelGGL((pw_render_rowpage_kernel<uint8_t, true, 0>), grid, dim3(64), lds_pad, st, rp, pa); break;
      case 3: hipLaunchKernelGGL((pw_render_rowpage_kernel<uint8_t, true, 1>), grid, dim3(64), lds_pad, st, rp, pa); break;
      case 4: hipLaunchKernelGGL((pw_render_rowpage_kernel<float, false, 0>), grid, dim3(64), lds_pad, st, rp, pa); break;
      case 5: hipLaunchKernelGGL((pw_render_rowpage_kernel<float, false, 1>), grid, dim3(64), lds_pad, st, rp, pa); break;
      case 6: hipLaunchKernelGGL((pw_render_rowpage_kernel<float, true, 0>), grid, dim3(64), lds_pad, st, rp, pa); break;
      default: hipLaunchKernelGGL((pw_render_rowpage_kernel<float, true, 1>), grid, dim3(64), lds_pad, st, rp, pa); break;
    }
  }
}

// rec_ready: the group step kernel of this call already left the page records of (puzzle_id, pos) in e->d_rec
// live_form: the caller checked (retained_live_form) that only the live pages need rendering: 1 the list, 2 the early exits, 3 the
// list and of it the pages whose rows changed (PwRetained::d_changed, filled by the record writer of this call), 4 the changed
// pixel rows of every environment (pw_render_rows_kernel; retained_changed_form)
// track: the records of this call are compared with PwRetained::d_shown (retained_tracks); a pre-pass here does it then
static void launch_render(PwEngine* e, const RenderArgs& ra, int32_t batch, hipStream_t st, bool rec_ready, int live_form, bool track) {
  const bool paged = page_path(e, ra.env_stride) && !ra.do_step && !ra.skip_movables && ensure_rec(e, batch);
  if (paged && !rec_ready) {
    PageRecArgs pa{ra.hdrs, ra.puzzle_id, ra.pos, static_cast<PageRec*>(e->d_rec), batch, ra.np, e->set->count,
                   track ? e->ret.d_shown : nullptr, track ? e->ret.d_changed : nullptr};
    hipLaunchKernelGGL(pw_page_records_kernel, dim3((batch + 255) / 256), dim3(256), 0, st, pa);
  }
  RenderProfScope prof(e, st);
  if (paged && e->rowpage) {
    launch_rowpage(e, ra, batch, st);
    return;
  }
  if (paged) {
    // The kernel numbers 16-byte chunks with 32 bits: batches whose buffer exceeds 2^31 chunks (32 GiB) are
    // rendered in consecutive slices of whole environments (each slice starts on an environment boundary;
    // a page at a slice boundary is written by the slice owning its bytes).
    const uint32_t cpe = static_cast<uint32_t>(ra.env_stride / 16);
    int32_t max_envs = static_cast<int32_t>(std::max<uint64_t>(1, ((1ull << 31) - 512) / cpe));
    if (e->page_slice_envs > 0) max_envs = static_cast<int32_t>(std::min<int64_t>(max_envs, e->page_slice_envs));  // tests
    for (int32_t first = 0; first < batch; first += max_envs) {
      const int32_t nb = std::min(max_envs, batch - first);
      RenderArgs rp = ra;
      rp.puzzle_id = ra.puzzle_id + first;
      rp.pos = ra.pos + static_cast<int64_t>(first) * ra.np * 2;
      rp.obs = ra.obs + static_cast<int64_t>(first) * ra.env_stride;
      rp.batch = nb;
      CopyArgs ca;
      ca.simg = e->d_simg;
      ca.puzzle_id = rp.puzzle_id;
      ca.obs = rp.obs;
      ca.simg_stride = e->simg_stride;
      ca.batch = nb;
      ca.chunks_per_env = cpe;
      ca.n_chunks = static_cast<uint32_t>((e->obs_bytes + 15) / 16);
      ca.inv_cpe = 1.0f / static_cast<float>(cpe);
      ca.rec = static_cast<const PageRec*>(e->d_rec) + first;
      const uint64_t d = 27ull * static_cast<uint64_t>(e->pad_w);
      ca.magic_cellrow = static_cast<uint32_t>(((1ull << 32) + d - 1) / d);
      const uint64_t total = static_cast<uint64_t>(nb) * cpe;
      ca.n_pages = static_cast<uint32_t>((total + 255) / 256);
      // the live launch has a configuration of its own once the tuner has measured one (its trial launches set the engine's)
      const PwRetained& rt = e->ret;
      const bool own_cfg = live_form && rt.tuned && !e->tuning;
      const int order = own_cfg ? rt.order : e->page_order, run_log2 = own_cfg ? rt.run_log2 : e->page_run_log2;
      const int load_all = own_cfg ? rt.load_all : e->page_load_all;
      ca.order = static_cast<uint32_t>(order);
      ca.run_log2 = static_cast<uint32_t>(ca.order == 1u ? std::min(run_log2, 3) : run_log2);
      ca.zero_page = reinterpret_cast<const uint8_t*>(e->d_scratch) + 4096;
      ca.live = nullptr;
      ca.live_n = nullptr;
      ca.n_live = 0;
      // (the live forms run only where one launch covers the batch (live_applies), so `first` is 0 for them: form 3 passes
      // `changed` as it is; form 4 indexes it by the environment inside the slice, like `rec`, and keeps the offset written out)
      ca.changed = live_form == 3 ? rt.d_changed : nullptr;
      if (live_form == 4) {
        // the changed rows, environment by environment: a fixed grid, no page order, no list, no LDS padding (an occupancy cap
        // only costs here, profiles/obs_changed.txt section 4)
        ca.changed = rt.d_changed + first;
        const dim3 rows_grid(static_cast<unsigned>((nb + PW_ROWS_WAVES - 1) / PW_ROWS_WAVES)), rows_block(64 * PW_ROWS_WAVES);
        if (e->page_f32) {
          rp.estat = e->d_estat_page;
          rp.estat_off = e->d_estat_page_off;
          hipLaunchKernelGGL((pw_render_rows_kernel<float, PW_ROWS_STORE_NT != 0>), rows_grid, rows_block, 0, st, rp, ca);
        } else {
          hipLaunchKernelGGL((pw_render_rows_kernel<uint8_t, PW_ROWS_STORE_NT != 0>), rows_grid, rows_block, 0, st, rp, ca);
        }
        continue;
      }
      unsigned grid = page_grid(ca.n_pages, ca.order, ca.run_log2);
      if (live_form == 1 || live_form == 3) {
        ca.live = rt.d_live;
        ca.live_n = rt.n_live < 0 ? rt.d_count : nullptr;  // list rebuilt in-stream: the upper bound, the surplus workgroups return
        ca.n_live = rt.n_live < 0 ? ca.n_pages : static_cast<uint32_t>(rt.n_live);
        grid = page_grid(ca.n_live, ca.order, ca.run_log2);
        if (grid == 0) continue;
      }
      const size_t lds_pad = static_cast<size_t>(own_cfg ? rt.lds_pad_kb : e->page_lds_pad_kb) * 1024;
      if (e->page_f32) {
        rp.estat = e->d_estat_page;  // the page kernels index the frame-layout zone table
        rp.estat_off = e->d_estat_page_off;
        launch_page<float>(e->tuning, load_all != 0, live_form, grid, lds_pad, st, rp, ca);
      } else {
        launch_page<uint8_t>(e->tuning, load_all != 0, live_form, grid, lds_pad, st, rp, ca);
      }
    }
    return;
  }
  const dim3 block(PW_RENDER_THREADS);
  if (e->fast_u8_ppc3) {
    hipLaunchKernelGGL(pw_render_u8_ppc3_kernel, dim3(static_cast<unsigned>(batch)), block, e->render_lds, st, ra);
    return;
  }
  // One workgroup streams 10 GB/s at best, so a small batch of big frames (the reference's default 10 MB
  // float32 observation, 64 environments: 1.1 ms -> 0.13 ms) is split into bands of >= 16 KiB, ~8 k workgroups
  // in all.  From 1 024 environments on one workgroup each is enough, and more concurrent streams only lower
  // the HBM write efficiency (1 024 envs lose 10 % with 8 bands).
  RenderArgs rb = ra;
  if (!ra.do_step && !ra.dirty_rows) {
    const int64_t n_chunks = (e->obs_bytes + 15) / 16;
    const int64_t by_size = std::max<int64_t>(1, n_chunks / 1024);
    const int64_t by_batch = batch >= 1024 ? 1 : (8192 + batch - 1) / std::max(batch, 1);
    rb.bands = static_cast<int32_t>(std::min(by_size, by_batch));
  }
  const dim3 grid(static_cast<unsigned>(static_cast<int64_t>(batch) * rb.bands));
  if (e->cfg.obs_dtype == PW_OBS_U8)
    hipLaunchKernelGGL(pw_render_generic_kernel<uint8_t>, grid, block, e->render_lds, st, rb);
  else
    hipLaunchKernelGGL(pw_render_generic_kernel<float>, grid, block, e->render_lds, st, rb);
}

int pw_render(PwEngine* e, const int32_t* puzzle_id, const int8_t* pos, void* obs, int64_t env_stride_bytes,
              int32_t batch, void* stream) try {
  if (!e) return pw_fail(PW_EINVAL, "null engine");
  if (batch <= 0) return PW_OK;
  PwDeviceGuard guard(e->set->device);
  RenderArgs ra;
  int rc = fill_render_args(e, puzzle_id, pos, obs, env_stride_bytes, batch, &ra);
  if (rc != PW_OK) return rc;
  const bool track = retained_tracks(e, ra, batch, 0);
  launch_render(e, ra, batch, static_cast<hipStream_t>(stream), false, 0, track);
  retained_after_full_render(e, ra, batch);  // (every byte is written: the repair path of a retained buffer)
  if (track) e->ret.shown_valid = true;
  return check_launch("pw_render");
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

// pw_render for a state that something other than a step of this engine's pw_step_render left (K27: a start-state draw behind a
// state-only step): pw_step_render's render half with the record pre-pass in place of the step kernel's records.  Into the
// retained buffer of the retained (puzzle_id, batch) it writes the live pages only, and with PW_OPT_OBS_CHANGED_PAGES of those
// the pages whose rows differ from what the buffer shows; into any other buffer it is pw_render.
int pw_render_retained(PwEngine* e, const int32_t* puzzle_id, const int8_t* pos, void* obs, int64_t env_stride_bytes,
                       int32_t batch, void* stream) try {
  if (!e) return pw_fail(PW_EINVAL, "pw_render_retained: null engine");
  if (batch <= 0) return PW_OK;
  PwDeviceGuard guard(e->set->device);
  RenderArgs ra;
  int rc = fill_render_args(e, puzzle_id, pos, obs, env_stride_bytes, batch, &ra);
  if (rc != PW_OK) return rc;
  const int live_form = retained_live_form(e, ra, batch);
  const bool track = retained_tracks(e, ra, batch, live_form);
  launch_render(e, ra, batch, static_cast<hipStream_t>(stream), false, (live_form && track && e->ret.shown_valid) ? retained_changed_form(e) : live_form,
                track);
  if (!live_form) retained_after_full_render(e, ra, batch);
  if (track) e->ret.shown_valid = true;  // (whichever form: the pre-pass left the new positions in `shown`)
  return check_launch("pw_render_retained");
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

// The changed-row switch: no engine option (the option table is closed), one setter and one getter.  Both forms leave the
// retained buffer equal to `shown`, so the switch may change between any two calls.
int pw_engine_set_obs_changed_rows(PwEngine* e, int32_t on) try {
  if (!e) return pw_fail(PW_EINVAL, "pw_engine_set_obs_changed_rows: null engine");
  e->ret.rows_option = on != 0 ? 1 : 0;
  return PW_OK;
} catch (...) {
  return pw_current_exception();
}

int32_t pw_engine_get_obs_changed_rows(const PwEngine* e) try {
  if (!e) return pw_fail(PW_EINVAL, "pw_engine_get_obs_changed_rows: null engine");
  return e->ret.rows_option;
} catch (...) {
  return pw_current_exception();
}

}  // extern "C"

// pw_engine_step_render.inc -- the entry points that step and render in one call: pw_step_render, pw_step_render_delta and the
// completion word / host copy of its batch of one (pw_engine_set_step_signal, pw_engine_set_step_host_copy).  Part of the
// single translation unit pw_kernels.hip, included after pw_engine_render.inc and pw_engine_step.inc: uses fill_step_args,
// attach_binding, launch_one_step and launch_group of the step file, page_path, ensure_rec, the retained_* rules and launch_render
// of the render file, and fill_render_args from pw_engine.inc.

extern "C" {

// Step + observation.  With the page-ordered render the step kernel and the render kernel are two
// launches on the caller's stream (splitting the batch over two streams to hide the 26 us step
// kernel behind the render of the other half measured 2 % SLOWER); otherwise ONE launch: wave 0
// of every per-environment workgroup advances its environment, the workgroup then draws it.
int pw_step_render(PwEngine* e, const int32_t* puzzle_id, const uint8_t* actions, int8_t* pos, int32_t* steps,
                   double* reward, int8_t* dgoals, uint8_t* terminated, uint8_t* truncated, void* obs,
                   int64_t env_stride_bytes, int32_t batch, uint32_t flags, void* stream) try {
  if (!e) return pw_fail(PW_EINVAL, "null engine");
  RenderArgs ra;
  int rc = fill_step_args(e, puzzle_id, actions, pos, steps, reward, dgoals, terminated, truncated, batch, flags,
                          &ra.step);
  if (rc != PW_OK) return rc;
  if (batch <= 0) return PW_OK;
  PwDeviceGuard guard(e->set->device);
  const StepArgs sa = ra.step;
  rc = fill_render_args(e, puzzle_id, pos, obs, env_stride_bytes, batch, &ra);
  if (rc != PW_OK) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  // two launches (lane-group step kernel, then the render): measured faster than the single fused launch
  // for every engine -- the wavefront formulation of the step sits on each workgroup's critical path there
  if (!e->force_fused) {
    // the lane-group step kernel leaves the page records of the new state for the page-ordered render (no pre-pass);
    // the other step kernels (PW_OPT_STEP_KERNEL) do not, the render then runs its record pre-pass
    StepArgs s1 = sa;
    attach_binding(e, &s1);
    if (page_path(e, env_stride_bytes) && ensure_rec(e, batch)) s1.rec = static_cast<PageRec*>(e->d_rec);
    // a retained buffer (PW_OPT_OBS_PADDING_ONCE) holds its frame padding already: the pages with anything else only -- and of
    // those (PW_OPT_OBS_CHANGED_PAGES) only the ones whose rows differ from the positions the buffer is known to show
    const int live_form = retained_live_form(e, ra, batch);
    const bool track = retained_tracks(e, ra, batch, live_form);
    if (track) {
      s1.shown = e->ret.d_shown;
      s1.changed = e->ret.d_changed;
    }
    const bool rec_ready = launch_one_step(e, s1, batch, st);
    launch_render(e, ra, batch, st, rec_ready, (live_form && track && e->ret.shown_valid) ? retained_changed_form(e) : live_form, track);
    if (!live_form) retained_after_full_render(e, ra, batch);
    if (track) e->ret.shown_valid = true;  // (whichever form: the record writer left the new positions in `shown`)
    return check_launch("pw_step_render");
  }
  ra.step = sa;
  ra.do_step = 1;
  launch_render(e, ra, batch, st);
  retained_after_full_render(e, ra, batch);
  return check_launch("pw_step_render");
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_engine_set_step_signal(PwEngine* e, void* word) try {
  if (!e) return pw_fail(PW_EINVAL, "null engine");
  if (reinterpret_cast<uintptr_t>(word) & 7) return pw_fail(PW_EINVAL, "pw_engine_set_step_signal: the word must be 8-byte aligned");
  e->step_signal = static_cast<unsigned long long*>(word);
  e->step_signal_seq = 0ull;
  return PW_OK;
} catch (...) {
  return pw_current_exception();
}

int pw_engine_set_step_host_copy(PwEngine* e, void* block) try {
  if (!e) return pw_fail(PW_EINVAL, "null engine");
  if (reinterpret_cast<uintptr_t>(block) & 7) return pw_fail(PW_EINVAL, "pw_engine_set_step_host_copy: the block must be 8-byte aligned");
  e->step_host_copy = static_cast<uint8_t*>(block);
  return PW_OK;
} catch (...) {
  return pw_current_exception();
}

int pw_step_render_delta(PwEngine* e, const int32_t* puzzle_id, const uint8_t* actions, int8_t* pos, int32_t* steps,
                         double* reward, int8_t* dgoals, uint8_t* terminated, uint8_t* truncated, void* obs,
                         int64_t env_stride_bytes, int32_t batch, uint32_t flags, void* stream) try {
  if (!e) return pw_fail(PW_EINVAL, "null engine");
  // uint8 / ppc 3 engines patch from their static images, every other engine redraws the changed rows with
  // the generic LDS kernel; both need the group step kernel (it reports the rows).  Otherwise: full render.
  // float32 / ppc 3 also has static images, but its changed rows are 4x the bytes: one wavefront walking them
  // 4 KiB at a time (0.29 ms) loses to the 256-thread generic redraw (0.27 ms), so only uint8 patches from images
  const bool page_path = e->fast_u8_ppc3 && e->d_simg;
  if ((e->fast_u8_ppc3 && !e->d_simg) || e->step_kernel != 0 || e->force_fused)
    return pw_step_render(e, puzzle_id, actions, pos, steps, reward, dgoals, terminated, truncated, obs, env_stride_bytes,
                          batch, flags, stream);
  RenderArgs ra;
  int rc = fill_step_args(e, puzzle_id, actions, pos, steps, reward, dgoals, terminated, truncated, batch, flags, &ra.step);
  if (rc != PW_OK) return rc;
  if (batch <= 0) return PW_OK;
  PwDeviceGuard guard(e->set->device);
  StepArgs sa = ra.step;
  rc = fill_render_args(e, puzzle_id, pos, obs, env_stride_bytes, batch, &ra);
  if (rc != PW_OK) return rc;
  // (the redraw of the retained batch stays inside its puzzles' own rows; that of other ids or another layout need not)
  if (!(e->ret.obs == obs && e->ret.stride == env_stride_bytes && e->ret.batch == batch && e->ret.puzzle_id == puzzle_id)) retained_overwritten(e, ra, batch);
  else e->ret.shown_valid = false;  // (pixels change here that `shown` is not told about: the next pw_step_render takes the live launch)
  if (e->dirty_cap < batch) {
    if (e->d_dirty) (void)hipFree(e->d_dirty);
    e->d_dirty = nullptr;
    e->dirty_cap = 0;
    if (hipMalloc(reinterpret_cast<void**>(&e->d_dirty), static_cast<size_t>(batch) * sizeof(uint32_t)) != hipSuccess)
      return pw_fail(PW_ENOMEM, "pw_step_render_delta: cannot allocate the dirty-row buffer");
    e->dirty_cap = batch;
  }
  hipStream_t st = static_cast<hipStream_t>(stream);
  // (not inside a stream capture: a replayed launch would carry the number its capture baked in, and the other workgroups would take the
  // hand-over words of the replay before -- the two launches below are what a graph may hold)
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  const bool one_launch = batch == 1 && !page_path && e->step_signal != nullptr && e->step_one_fused && e->obs_bytes >= (64 << 10) &&
                          (hipStreamIsCapturing(st, &cap) != hipSuccess || cap == hipStreamCaptureStatusNone);
  if (one_launch) {
    // the single-environment adapters' step as ONE launch: pw_step_render_one_kernel (pw_render_kernels.inc)
    ra.step = sa;
    ra.signal = e->step_signal;
    ra.signal_seq = ++e->step_signal_seq;
    ra.signal_count = e->d_scratch + 32;
    ra.bands = 8;
    const unsigned long long one_seq = ++e->step_one_seq;  // (never starts again: the hand-over word of a launch must differ from every earlier one's)
    const dim3 grid(8u), block(PW_RENDER_THREADS);
    if (e->cfg.obs_dtype == PW_OBS_U8)
      hipLaunchKernelGGL(pw_step_render_one_kernel<uint8_t>, grid, block, e->render_lds, st, ra, e->d_scratch + 64, one_seq, e->step_one_fused == 1 ? 1 : 0, e->step_host_copy);  // (bytes 256 .. 399 of the scratch page)
    else
      hipLaunchKernelGGL(pw_step_render_one_kernel<float>, grid, block, e->render_lds, st, ra, e->d_scratch + 64, one_seq, e->step_one_fused == 1 ? 1 : 0, e->step_host_copy);  // (bytes 256 .. 399 of the scratch page)
    if (int rc2 = check_launch("pw_step_render_delta")) return rc2;
    return 2;  // (the completion word will be written; 2: by a launch that must not be captured into a graph and replayed)
  }
  sa.dirty = e->d_dirty;
  RolloutArgs r;
  r.s = sa;
  r.num_steps = 1;
  r.reward_hist = nullptr;
  r.term_hist = nullptr;
  r.trunc_hist = nullptr;
  launch_group(e, r, batch, st);
  if (!page_path) {
    ra.dirty_rows = e->d_dirty;
    const bool signalled = e->step_signal != nullptr && batch == 1;
    if (signalled) {
      ra.signal = e->step_signal;
      ra.signal_seq = ++e->step_signal_seq;
      ra.signal_count = e->d_scratch + 32;
    }
    // a batch of one (the gym / dm_env adapters: observation in pinned host memory): the changed rows go out through several
    // workgroups -- one alone writes ~10 GB/s across the link
    if (batch == 1 && e->obs_bytes >= (64 << 10)) ra.bands = 8;
    const dim3 grid(static_cast<unsigned>(batch) * static_cast<unsigned>(ra.bands)), block(PW_RENDER_THREADS);
    if (e->cfg.obs_dtype == PW_OBS_U8)
      hipLaunchKernelGGL(pw_render_generic_kernel<uint8_t>, grid, block, e->render_lds, st, ra);
    else
      hipLaunchKernelGGL(pw_render_generic_kernel<float>, grid, block, e->render_lds, st, ra);
    if (int rc2 = check_launch("pw_step_render_delta")) return rc2;
    return signalled ? 1 : PW_OK;
  }
  CopyArgs ca;
  ca.simg = e->d_simg;
  ca.puzzle_id = puzzle_id;
  ca.obs = ra.obs;
  ca.simg_stride = e->simg_stride;
  ca.batch = batch;
  ca.chunks_per_env = static_cast<uint32_t>(env_stride_bytes / 16);
  ca.n_chunks = static_cast<uint32_t>((e->obs_bytes + 15) / 16);
  ca.inv_cpe = 1.0f / static_cast<float>(ca.chunks_per_env);
  hipLaunchKernelGGL(pw_render_delta_kernel<uint8_t>, dim3(static_cast<unsigned>(batch)), dim3(64), 0, st, ra, ca, e->d_dirty);
  return check_launch("pw_step_render_delta");
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

}  // extern "C"

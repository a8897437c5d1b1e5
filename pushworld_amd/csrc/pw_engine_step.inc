// pw_engine_step.inc -- the state-only half of the engine: the binding of a batch (bind_launch, rebind_async, pw_batch_bind /
// _unbind), pw_reset, pw_resample, fill_step_args, the choice of the step kernel (launch_group / _board / _bound,
// launch_one_step), pw_step and pw_rollout.  Part of the single translation unit pw_kernels.hip, included after
// pw_engine_render.inc: uses live_build and RenderProfScope from there, release_bind from pw_engine.inc, the kernels of
// pw_step_kernels.inc / pw_seg_kernels.inc and check_launch.

extern "C" {

// ---- pw_batch_bind: the segment list of a batch, built on the device (pw_seg_kernels.inc: count / plan / fill)
static void bind_launch(PwEngine* e, hipStream_t st) {
  PwBind* b = e->bind;
  const int P = e->set->count;
  (void)hipMemsetAsync(b->cnt, 0, static_cast<size_t>(P) * 4, st);
  (void)hipMemsetAsync(b->mn, 0x7f, static_cast<size_t>(P) * 4, st);
  (void)hipMemsetAsync(b->mx, 0xff, static_cast<size_t>(P) * 4, st);
  BindArgs a{b->puzzle_id, e->d_seg_dir, b->cnt, b->mn, b->mx, b->seg_base, b->perm_base, b->rank, b->perm, b->d_bound,
             b->d_segs, b->meta, b->mlist, b->batch, P, b->min_envs, b->seg_cap, (e->bind_max_kb > 0 ? e->bind_max_kb : 48) * 1024, e->bind_lanes - 1, b->epw_log2, b->mepw_log2};
  const dim3 grid(static_cast<unsigned>((b->batch + 255) / 256));
  hipLaunchKernelGGL(pw_bind_count_kernel, grid, dim3(256), 0, st, a);
  hipLaunchKernelGGL(pw_bind_plan_kernel, dim3(1), dim3(1024), 0, st, a);
  hipLaunchKernelGGL(pw_bind_fill_kernel, grid, dim3(256), 0, st, a);
  hipLaunchKernelGGL(pw_bind_multi_kernel, grid, dim3(256), 0, st, a);
  hipLaunchKernelGGL(pw_bind_mslot_kernel, grid, dim3(256), 0, st, a);
}

// pw_resample / pw_reset on the bound buffer: the ids may have changed -- the list is rebuilt behind them on the same stream,
// without a host round trip (the segment role is launched with the upper bound of the segment count from here on)
static void rebind_async(PwEngine* e, const int32_t* puzzle_id, int32_t batch, hipStream_t st) {
  PwBind* b = e->bind;
  if (!b || b->puzzle_id != puzzle_id || b->batch != batch) return;
  e->ret.valid = e->ret.shown_valid = false;  // other puzzles, other padding: the next render is a full one
  if (e->ret.list_pid == puzzle_id && e->ret.list_batch == batch) (void)live_build(e, puzzle_id, batch, st, false);
  bind_launch(e, st);
  b->seg_grid = b->seg_cap;
  b->lds_bytes = e->seg_max_bytes;
  b->lds_bytes0 = e->seg_max_bytes;
  b->multi_envs = -1;  // (unknown until the next pw_batch_bind reads the counts back)
}

int pw_reset(PwEngine* e, const int32_t* puzzle_id, const uint8_t* mask, int8_t* pos, int32_t* steps,
             uint8_t* terminated, uint8_t* truncated, int32_t batch, void* stream) try {
  if (!e) return pw_fail(PW_EINVAL, "null engine");
  if (e->mailbox) return pw_fail(PW_EINVAL, "pw_reset: this engine has an open mailbox (pw_mailbox_close first)");
  if (batch <= 0) return PW_OK;  // an empty batch is a no-op whatever the pointers (an empty tensor's is null)
  if (!puzzle_id || !pos || !steps) return pw_fail(PW_EINVAL, "null argument");
  PwDeviceGuard guard(e->set->device);
  ResetArgs a{e->set->d_headers, e->set->d_blob, puzzle_id, mask, pos, steps, terminated, truncated, batch, e->np, e->set->count};
  const int64_t threads = static_cast<int64_t>(batch) * e->np;
  const unsigned blocks = static_cast<unsigned>((threads + 255) / 256);
  hipLaunchKernelGGL(pw_reset_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  rebind_async(e, puzzle_id, batch, static_cast<hipStream_t>(stream));  // (a caller may have written new ids before the reset)
  return check_launch("pw_reset");
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

uint64_t pw_mix64(uint64_t seed, uint64_t env, uint64_t episode) { return mix64(seed, env, episode); }

int pw_resample(PwEngine* e, int32_t* puzzle_id, const uint8_t* terminated, const uint8_t* truncated,
                const int32_t* table, int32_t table_len, uint64_t seed, uint32_t* episode, int32_t batch,
                void* stream) try {
  if (!e) return pw_fail(PW_EINVAL, "null engine");
  const int n = e->set->count;
  if (table ? table_len <= 0 : (table_len != 0 && table_len != n))
    return pw_fail(PW_EINVAL, "pw_resample: table_len must be > 0 with a table, 0 or the set size without");
  if (batch <= 0) return PW_OK;
  if (!puzzle_id || !episode) return pw_fail(PW_EINVAL, "null argument");
  PwDeviceGuard guard(e->set->device);
  ResampleArgs a{puzzle_id, terminated, truncated, table, episode, seed, table ? table_len : n, batch};
  hipLaunchKernelGGL(pw_resample_kernel, dim3((batch + 255) / 256), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  rebind_async(e, puzzle_id, batch, static_cast<hipStream_t>(stream));
  return check_launch("pw_resample");
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

static int fill_step_args(PwEngine* e, const int32_t* puzzle_id, const uint8_t* actions, int8_t* pos, int32_t* steps,
                          double* reward, int8_t* dgoals, uint8_t* terminated, uint8_t* truncated, int32_t batch,
                          uint32_t flags, StepArgs* a) {
  if (!e) return pw_fail(PW_EINVAL, "null engine");
  if (e->mailbox) return pw_fail(PW_EINVAL, "this engine has an open mailbox (pw_mailbox_open): its environments live in the resident kernel until pw_mailbox_close");
  // (the callers return PW_OK for an empty batch before anything is launched: no pointer is looked at then)
  if (batch > 0 && (!puzzle_id || !actions || !pos || !steps || !terminated || !truncated))
    return pw_fail(PW_EINVAL, "null argument");
  *a = StepArgs{e->set->d_headers, e->set->d_blob, puzzle_id, actions, pos, steps, reward, dgoals,
                terminated, truncated, batch, e->cfg.max_steps, flags, e->np, nullptr, e->d_scratch + 4, nullptr,
                e->d_ovl, e->d_ovl_dir, e->step_reverse, e->set->count, e->d_boards, e->d_counters,
                (e->step_quad16 != 2 && e->ovl_puzzles == e->set->count) ? e->d_qdesc : nullptr,
                nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, e->d_scratch + 8, 0, 0};
  return PW_OK;
}

// a bound batch (pw_batch_bind): pw_step / pw_rollout / pw_step_render calls on the bound puzzle_id buffer and batch size carry the
// segment list (the other users of StepArgs -- pw_step_render_delta, the mailbox, the fused render -- never see it)
static void attach_binding(const PwEngine* e, StepArgs* a) {
  // (a binding that is known to hold no segment -- a Level-0 pool: two environments per puzzle -- changes nothing: the plain launches)
  if (const PwBind* b = e->bind; b && b->puzzle_id == a->puzzle_id && b->batch == a->batch && e->step_kernel == 0 &&
                                 !(b->seg_grid != b->seg_cap && b->info[0] == 0 && b->multi_envs <= 0)) {
    a->segs = b->d_segs;
    a->bind_meta = b->meta;
    a->perm = b->perm;
    a->mlist = b->mlist;
    a->bound = b->d_bound;
    a->seg_dir = e->d_seg_dir;
    a->seg_grid = b->seg_grid;
  }
}

static void launch_group(PwEngine* e, const RolloutArgs& r, int32_t batch, hipStream_t st) {
  // overlap tables (PW_OPT_STEP_TABLES): 0 the set has none, 2 every puzzle has them (the table-only instance: no row
  // loops, nothing left to stage in LDS), 1 some have
  const int tab = e->ovl_puzzles == 0 ? 0 : (e->ovl_puzzles == e->set->count ? 2 : 1);
  // Row tables staged in LDS: since the movables that fit into 8 x 8 cells carry their shape in a register, only
  // the pools with big objects and many movables (N_pad 32) still gain from it, and only when a launch runs several
  // steps (64-step rollouts: C4 +7 %; C3 -8 %, C2 -2 %; one step per launch: slower) -- profiles/r02_step_xp.txt
  const bool lds = tab != 2 && (e->step_lds_tables == 1 ||
                                (e->step_lds_tables == 0 && e->lds_tables_fit && r.num_steps >= 4 && e->np > 16));
  const bool single = r.num_steps == 1 && !r.reward_hist && !r.term_hist && !r.trunc_hist;
  const dim3 g8(static_cast<unsigned>((batch + 31) / 32)), g16(static_cast<unsigned>((batch + 15) / 16)),
      g32(static_cast<unsigned>((batch + 7) / 8)), block(256);
#define PW_LAUNCH_GROUP(GS, TWO, GRID)                                                                                  \
  do {                                                                                                                  \
    const int v = tab == 2 ? (single ? 9 : 8) : ((lds ? 4 : 0) | (single ? 2 : 0) | tab);                               \
    switch (v) {                                                                                                        \
      case 0: hipLaunchKernelGGL((pw_step_group_kernel<GS, false, false, TWO, 0>), GRID, block, 0, st, r); break;       \
      case 1: hipLaunchKernelGGL((pw_step_group_kernel<GS, false, false, TWO, 1>), GRID, block, 0, st, r); break;       \
      case 2: hipLaunchKernelGGL((pw_step_group_kernel<GS, false, true, TWO, 0>), GRID, block, 0, st, r); break;        \
      case 3: hipLaunchKernelGGL((pw_step_group_kernel<GS, false, true, TWO, 1>), GRID, block, 0, st, r); break;        \
      case 4: hipLaunchKernelGGL((pw_step_group_kernel<GS, true, false, TWO, 0>), GRID, block, 0, st, r); break;        \
      case 5: hipLaunchKernelGGL((pw_step_group_kernel<GS, true, false, TWO, 1>), GRID, block, 0, st, r); break;        \
      case 6: hipLaunchKernelGGL((pw_step_group_kernel<GS, true, true, TWO, 0>), GRID, block, 0, st, r); break;         \
      case 7: hipLaunchKernelGGL((pw_step_group_kernel<GS, true, true, TWO, 1>), GRID, block, 0, st, r); break;         \
      case 8: hipLaunchKernelGGL((pw_step_group_kernel<GS, false, false, TWO, 2>), GRID, block, 0, st, r); break;       \
      default: hipLaunchKernelGGL((pw_step_group_kernel<GS, false, true, TWO, 2>), GRID, block, 0, st, r); break;       \
    }                                                                                                                   \
  } while (0)
  // N_pad 8 / 16 sets with tables for every puzzle: the lanes per environment are chosen per workgroup of 32 environments
  // (pw_step_group_mixed_kernel<., true>: 4 lanes where none has more than 4 movables, 8 lanes with one movable each up to
  // 8, two beyond) -- 64-step rollouts of the C3 set: see profiles/r04_bench.json -> state_only_rollout
  if (e->np <= 16 && tab == 2 && e->step_narrow_groups == 0 && !e->step_wide_groups && e->step_mixed != 2) {
    const unsigned nb = static_cast<unsigned>((batch + 31) / 32);
    if (single) hipLaunchKernelGGL((pw_step_group_mixed_kernel<true, true>), dim3(nb), block, 0, st, r);
    else hipLaunchKernelGGL((pw_step_group_mixed_kernel<false, true>), dim3(nb), block, 0, st, r);
  }
  else if (e->np <= 8) PW_LAUNCH_GROUP(8, false, g8);  // Level-0 pools (N <= 8): 8 environments per wavefront
  // N_pad 16 sets in 8-lane groups, two movables per lane (8 environments per wavefront) with the table-only kernels:
  // 64-step rollouts of the C3 set 1.09 -> 1.33e10 env-steps/s, one step per launch 13.9 -> 12.3 us (rocprofv3 kernel time,
  // profiles/r03_step_tables.txt); slower with the row-loop kernels
  else if (e->np <= 16 && (e->step_narrow_groups == 1 || (e->step_narrow_groups == 0 && tab == 2)))
    PW_LAUNCH_GROUP(8, true, g8);
  else if (e->np <= 16) PW_LAUNCH_GROUP(16, false, g16);
  // N_pad 32 sets with tables for every puzzle: workgroups of 32 environments that run 8-lane groups (two movables per lane,
  // 8 environments per wavefront) unless one of their environments has more than 16 movables (pw_step_group_mixed_kernel);
  // PW_OPT_STEP_NARROW_GROUPS 2 = never
  else if (tab == 2 && !e->step_wide_groups && e->step_narrow_groups != 2) {
    const unsigned nb = static_cast<unsigned>((batch + 31) / 32);
    if (single) hipLaunchKernelGGL(pw_step_group_mixed_kernel<true>, dim3(nb), block, 0, st, r);
    else hipLaunchKernelGGL(pw_step_group_mixed_kernel<false>, dim3(2 * nb), block, 0, st, r);
  }
  else if (!e->step_wide_groups) PW_LAUNCH_GROUP(16, true, g16);  // N_pad 32: two movables per lane, 4 environments per wavefront
  else PW_LAUNCH_GROUP(32, false, g32);
#undef PW_LAUNCH_GROUP
}

// PW_OPT_STEP_LANE_BATCH: from this many environments on a state-only launch runs one lane per environment.  Measured
// (profiles/r03_lane_xp.txt; Level-1 set, one step per launch / 64-step rollouts): 65 536 envs 17.7 vs 17.5 us, 1.38e10 vs
// 0.84e10 env-steps/s (lane groups win: 1 024 wavefronts do not hide a single latency); 262 144 envs 34.8 vs 20.5 us,
// 1.65e10 vs 3.1e10; 1 048 576 envs 123 vs 34 us, 1.75e10 vs 4.95e10.
// The crossover (profiles/r03_lane_xp.txt, batch sweeps): N_pad <= 16 sets 131 072 (one step 21.5 vs 19.3 us, rollouts 1.45 vs
// 1.70e10).  N_pad 32 sets, against the lane groups that run 8 lanes wherever N <= 16 (pw_step_group_mixed_kernel): one step
// per launch 327 680 (262 144: 46.8 vs 43.9 us; 393 216: 65.6 vs 50.6), launches of several steps 1 048 576 (196 VGPRs, 2
// wavefronts per SIMD: the lane groups stay ahead up to there, 1.62 vs 1.69e10 at 1 M).
// Re-measured with the per-workgroup choice of lanes (round 4, profiles/r04_lane_threshold.txt): launches of several steps,
// N_pad <= 16: the groups are ahead at 131 072 (1.80 vs 1.55e10 env-steps/s), the lanes at 262 144 (2.99 vs 1.96e10) ->
// 196 608; N_pad 32: the groups stay ahead at 1 M (1.71 vs 1.51e10) -> 2 M.  One step per launch: as before.
static int64_t step_lane_batch_default(const PwEngine* e, bool multi_step) {
  return e->np <= 16 ? (multi_step ? 196608 : 131072) : (multi_step ? 2097152 : 327680);
}
static bool lane_per_env(const PwEngine* e, int32_t batch, bool needs_group_outputs, bool multi_step) {
  if (e->step_kernel == 2) return true;
  if (e->step_kernel != 0 || needs_group_outputs) return false;
  const bool all_tables = e->ovl_puzzles > 0 && e->ovl_puzzles == e->set->count;
  return all_tables && batch >= (e->step_lane_batch == 0 ? step_lane_batch_default(e, multi_step) : e->step_lane_batch);
}

// PW_OPT_STEP_BOARDS: state-only launches of sets of 8 x 8 puzzles run pw_step_board_kernel (registers only, one lane per
// environment) unless another kernel was asked for.
static bool board_kernel(const PwEngine* e, bool needs_group_outputs) {
  return e->d_boards != nullptr && e->step_kernel == 0 && e->step_boards != 2 && !needs_group_outputs;
}
// ... unless EVERY environment of the batch sits in a segment of a bound batch (C2: 4 096 copies of one puzzle): the segments -- one lane
// per environment as well, the puzzle's tables in LDS instead of whole-grid boards in registers -- are the faster kernel there
// (4 096 environments: 5.5 -> 4.8 us per step, 87.5 -> 76 us per 64 steps; 65 536: 6.6 -> 5.5 us, 89.6 -> 76 us)
static bool bound_all(const PwEngine* e, const StepArgs& a) {
  return a.segs && e->bind && e->bind->seg_grid != e->bind->seg_cap && e->bind->info[1] == a.batch;
}
static void launch_board(PwEngine* e, const RolloutArgs& r, int32_t batch, hipStream_t st) {
  const dim3 grid(static_cast<unsigned>((batch + 255) / 256)), block(256);
  if (e->np <= 4) hipLaunchKernelGGL(pw_step_board_kernel<4>, grid, block, 0, st, r);
  else hipLaunchKernelGGL(pw_step_board_kernel<8>, grid, block, 0, st, r);
}

// A bound batch: the segments (one lane per environment, tables in LDS) and, for the environments no segment holds, the lane
// groups -- in ONE launch where the per-workgroup kernel applies (the segment role at the front of its grid), else in two.
static void launch_bound(PwEngine* e, RolloutArgs r, int32_t batch, hipStream_t st) {
  const bool single = r.num_steps == 1 && !r.reward_hist && !r.term_hist && !r.trunc_hist;
  const int tab = e->ovl_puzzles == 0 ? 0 : (e->ovl_puzzles == e->set->count ? 2 : 1);
  const bool narrow = e->np <= 16 && tab == 2 && e->step_narrow_groups == 0 && !e->step_wide_groups && e->step_mixed != 2;
  const bool wide = e->np > 16 && tab == 2 && !e->step_wide_groups && e->step_narrow_groups != 2;
  const unsigned nseg = static_cast<unsigned>(r.s.seg_grid);
  const unsigned nb = static_cast<unsigned>((batch + 31) / 32);
  // dynamic LDS: the largest bound block (+ the action tiles of a launch of several steps behind it)
  const size_t lds = single ? ((e->bind->lds_bytes0 + 15u) & ~size_t(15))
                            : ((e->bind->lds_bytes + 15u) & ~size_t(15)) + static_cast<size_t>(PW_SEG_ACT_TILE) * PW_SEG_ENVS;
  const bool all_bound = e->bind->seg_grid != e->bind->seg_cap && e->bind->info[1] == batch;  // (known after pw_batch_bind's readback)
  // ONE launch for both roles: single steps (a launch is short: both roles must start together).  Launches of several steps keep the
  // kernels apart -- the segment role's registers (one lane carries a whole environment) would cost the lane groups a wavefront per
  // SIMD -- and run them side by side on two streams.
  if ((narrow || wide) && e->bind_fused != 2 && !all_bound && single) {
    const dim3 block(256);
    if (narrow) hipLaunchKernelGGL((pw_step_group_mixed_kernel<true, true, true>), dim3(nseg + nb), block, lds, st, r);
    else hipLaunchKernelGGL((pw_step_group_mixed_kernel<true, false, true>), dim3(nseg + nb), block, lds, st, r);
    return;
  }
  r.s.seg_grid = 0;  // (the lane-group launch below has no segment role; its environments are those with bound[e] == 0)
  const bool exact = e->bind->seg_grid != e->bind->seg_cap;
  // every environment the segments do not hold plays a puzzle whose block fits a lane's LDS slot (a C4 shard's Level-0 half): they
  // are stepped one lane each as well, 64 puzzles per wavefront (pw_step_mseg_kernel) -- launches of several steps only
  const bool lanes_rest = !single && exact && e->bind->multi_envs > 0 && e->bind->info[1] + e->bind->multi_envs == batch;
  const bool have_segs = !exact || e->bind->info[0] > 0;
  // Two kernels side by side: the one expected to run longer stays on the caller's stream and starts at once; the other one's
  // dependencies across streams (fork and join by events, ~10 us each) are hidden behind it -- the segments next to the lanes of
  // pw_step_mseg_kernel (a C4 shard: 199 against 155 us; with the segments on the side stream the launch took 224 us), the lane
  // groups next to the segments otherwise.  (Both in ONE launch, tried: every workgroup then carries the LDS of the largest block and a
  // quarter of them waits for a slot -- 239 us.)
  hipStream_t seg_st = st, rest_st = st;
  bool forked = false;
  if (!all_bound && have_segs && e->bind_fused != 2) {
    if (!e->side_stream) {
      if (hipStreamCreateWithFlags(&e->side_stream, hipStreamNonBlocking) != hipSuccess) e->side_stream = nullptr;
      if (e->side_stream && hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming) != hipSuccess) e->ev_fork = nullptr;
      if (e->side_stream && hipEventCreateWithFlags(&e->ev_join, hipEventDisableTiming) != hipSuccess) e->ev_join = nullptr;
    }
    if (e->side_stream && e->ev_fork && e->ev_join && hipEventRecord(e->ev_fork, st) == hipSuccess &&
        hipStreamWaitEvent(e->side_stream, e->ev_fork, 0) == hipSuccess) {
      if (lanes_rest) rest_st = e->side_stream;
      else seg_st = e->side_stream;
      forked = true;
    }
  }
#define PW_LAUNCH_SEG(NPV)                                                                                              \
  do {                                                                                                                  \
    if (single) hipLaunchKernelGGL((pw_step_seg_kernel<NPV, true>), dim3(nseg), dim3(PW_SEG_ENVS), lds, seg_st, r);     \
    else hipLaunchKernelGGL((pw_step_seg_kernel<NPV, false>), dim3(nseg), dim3(PW_SEG_ENVS), lds, seg_st, r);           \
  } while (0)
  if (have_segs) {
    switch (e->np) {
      case 4: PW_LAUNCH_SEG(4); break;
      case 8: PW_LAUNCH_SEG(8); break;
      case 16: PW_LAUNCH_SEG(16); break;
      default: PW_LAUNCH_SEG(32); break;
    }
  }
#undef PW_LAUNCH_SEG
  if (lanes_rest) {
    const int msp = e->bind->mepw_log2, per = 64 >> msp;  // (spread: 64 >> msp environments per wavefront)
    const dim3 grid(static_cast<unsigned>((e->bind->multi_envs + per - 1) / per)), block(64);
    r.s.mseg_spread = msp;
    const size_t mlds = ((static_cast<size_t>(e->bind->multi_slot) + 15u) & ~size_t(15)) + static_cast<size_t>(PW_SEG_ACT_TILE) * 64;
    switch (e->np) {
      case 4: hipLaunchKernelGGL(pw_step_mseg_kernel<4>, grid, block, mlds, rest_st, r); break;
      case 8: hipLaunchKernelGGL(pw_step_mseg_kernel<8>, grid, block, mlds, rest_st, r); break;
      case 16: hipLaunchKernelGGL(pw_step_mseg_kernel<16>, grid, block, mlds, rest_st, r); break;
      default: hipLaunchKernelGGL(pw_step_mseg_kernel<32>, grid, block, mlds, rest_st, r); break;
    }
  } else if (!all_bound) {
    launch_group(e, r, batch, st);
  }
  if (forked) {
    (void)hipEventRecord(e->ev_join, e->side_stream);
    (void)hipStreamWaitEvent(st, e->ev_join, 0);
  }
}

// One step of every environment with the kernel PW_OPT_STEP_KERNEL selects.  Returns true when the kernel left the page
// records of the new state in a.rec (only the lane-group kernel does).
static bool launch_one_step(PwEngine* e, const StepArgs& a_in, int32_t batch, hipStream_t st) {
  StepArgs a = a_in;
  if (a.segs && (a.dirty || (board_kernel(e, a.rec != nullptr || a.dirty != nullptr) && !bound_all(e, a)) ||
                 (e->bind->seg_grid != e->bind->seg_cap && e->bind->info[0] == 0))) {  // (no segment role in these launches)
    a.segs = nullptr;
    a.bound = nullptr;
    a.seg_grid = 0;
  }
  if (a.segs) {
    RolloutArgs r;
    r.s = a;
    r.num_steps = 1;
    r.reward_hist = nullptr;
    r.term_hist = nullptr;
    r.trunc_hist = nullptr;
    launch_bound(e, r, batch, st);
    return a.rec != nullptr;
  }
  if (e->step_kernel == 1) {  // PW_OPT_STEP_KERNEL = 1: one wavefront per environment
    hipLaunchKernelGGL(pw_step_kernel, dim3(static_cast<unsigned>((batch + 3) / 4)), dim3(256), 0, st, a);
    return false;
  }
  if (board_kernel(e, a.rec != nullptr || a.dirty != nullptr)) {
    RolloutArgs r;
    r.s = a;
    r.num_steps = 1;
    r.reward_hist = nullptr;
    r.term_hist = nullptr;
    r.trunc_hist = nullptr;
    launch_board(e, r, batch, st);
    return false;
  }
  if (lane_per_env(e, batch, a.rec != nullptr || a.dirty != nullptr, false)) {  // one lane per environment (PW_OPT_STEP_KERNEL = 2, or a big batch)
    const dim3 grid(static_cast<unsigned>((batch + 255) / 256)), block(256);
    if (e->ovl_puzzles == e->set->count && e->ovl_puzzles > 0) {  // tables for every puzzle: the loop-free instances
      switch (e->np) {
        case 4: hipLaunchKernelGGL((pw_step_lane_kernel<4, 2>), grid, block, 0, st, a); break;
        case 8: hipLaunchKernelGGL((pw_step_lane_kernel<8, 2>), grid, block, 0, st, a); break;
        case 16: hipLaunchKernelGGL((pw_step_lane_kernel<16, 2>), grid, block, 0, st, a); break;
        default: hipLaunchKernelGGL((pw_step_lane_kernel<32, 2>), grid, block, 0, st, a); break;
      }
      return false;
    }
    switch (e->np) {
      case 4: hipLaunchKernelGGL(pw_step_lane_kernel<4>, grid, block, 0, st, a); break;
      case 8: hipLaunchKernelGGL(pw_step_lane_kernel<8>, grid, block, 0, st, a); break;
      case 16: hipLaunchKernelGGL(pw_step_lane_kernel<16>, grid, block, 0, st, a); break;
      default: hipLaunchKernelGGL(pw_step_lane_kernel<32>, grid, block, 0, st, a); break;
    }
    return false;
  }
  RolloutArgs r;
  r.s = a;
  r.num_steps = 1;
  r.reward_hist = nullptr;
  r.term_hist = nullptr;
  r.trunc_hist = nullptr;
  launch_group(e, r, batch, st);
  return a.rec != nullptr;
}

int pw_step(PwEngine* e, const int32_t* puzzle_id, const uint8_t* actions, int8_t* pos, int32_t* steps,
            double* reward, int8_t* dgoals, uint8_t* terminated, uint8_t* truncated, int32_t batch,
            uint32_t flags, void* stream) try {
  StepArgs a;
  int rc = fill_step_args(e, puzzle_id, actions, pos, steps, reward, dgoals, terminated, truncated, batch, flags, &a);
  if (rc != PW_OK) return rc;
  if (batch <= 0) return PW_OK;
  attach_binding(e, &a);
  PwDeviceGuard guard(e->set->device);
  {
    RenderProfScope prof(e, static_cast<hipStream_t>(stream));  // PW_OPT_PROFILE_RENDER: a state-only call times its step launch
    launch_one_step(e, a, batch, static_cast<hipStream_t>(stream));
  }
  return check_launch("pw_step");
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_rollout(PwEngine* e, const int32_t* puzzle_id, const uint8_t* actions, int32_t num_steps, int8_t* pos,
               int32_t* steps, double* reward, int8_t* dgoals, uint8_t* terminated, uint8_t* truncated,
               double* reward_hist, uint8_t* terminated_hist, uint8_t* truncated_hist, int32_t batch, uint32_t flags,
               void* stream) try {
  RolloutArgs r;
  if (!e) return pw_fail(PW_EINVAL, "null engine");
  if (num_steps < 0) return pw_fail(PW_EINVAL, "num_steps must be >= 0");
  if (batch <= 0 || num_steps == 0) return PW_OK;  // nothing to do: no pointer is looked at
  int rc = fill_step_args(e, puzzle_id, actions, pos, steps, reward, dgoals, terminated, truncated, batch, flags, &r.s);
  if (rc != PW_OK) return rc;
  attach_binding(e, &r.s);
  PwDeviceGuard guard(e->set->device);
  r.num_steps = num_steps;
  r.reward_hist = reward_hist;
  r.term_hist = terminated_hist;
  r.trunc_hist = truncated_hist;
  hipStream_t st = static_cast<hipStream_t>(stream);
  RenderProfScope prof(e, st);  // PW_OPT_PROFILE_RENDER: the rollout launch
  // Launches of several steps take the segments of a bound batch when EVERY environment is bound: the segment role is a chain of
  // dependent steps per wavefront -- the heaviest puzzle of the batch sets its duration, up to ~4 us per step -- and next to lane
  // groups that fill every SIMD it does not finish sooner than they would have stepped its environments themselves (measured per 64
  // steps: C4 shard 299 -> 336 us; C3 270 -> 170; a batch of Level 1-4 puzzles 330 -> 255).  PW_OPT_BIND_ROLLOUTS: 1 always, 2 never.
  // ... and "bound" includes the environments that go one lane each, many puzzles per wavefront (pw_step_mseg_kernel: puzzles with
  // few environments in the batch and a small block -- a C4 shard's Level-0 half): then every environment of the launch is a lane.
  const bool seg_role = r.s.segs && (!board_kernel(e, false) || bound_all(e, r.s)) &&
                        (num_steps == 1 || e->bind_rollouts == 1 ||
                         (e->bind_rollouts == 0 && e->bind->seg_grid != e->bind->seg_cap &&
                          e->bind->info[1] + std::max(e->bind->multi_envs, 0) == batch));
  if (!seg_role) {
    r.s.segs = nullptr;
    r.s.bound = nullptr;
    r.s.seg_grid = 0;
  }
  if (seg_role) {
    launch_bound(e, r, batch, st);
  } else if (board_kernel(e, false)) {
    launch_board(e, r, batch, st);
  } else if (lane_per_env(e, batch, false, num_steps > 1)) {
    const dim3 grid(static_cast<unsigned>((batch + 255) / 256)), block(256);
    if (e->ovl_puzzles == e->set->count && e->ovl_puzzles > 0) {
      switch (e->np) {
        case 4: hipLaunchKernelGGL((pw_rollout_lane_kernel<4, 2>), grid, block, 0, st, r); break;
        case 8: hipLaunchKernelGGL((pw_rollout_lane_kernel<8, 2>), grid, block, 0, st, r); break;
        case 16: hipLaunchKernelGGL((pw_rollout_lane_kernel<16, 2>), grid, block, 0, st, r); break;
        default: hipLaunchKernelGGL((pw_rollout_lane_kernel<32, 2>), grid, block, 0, st, r); break;
      }
    } else
    switch (e->np) {
      case 4: hipLaunchKernelGGL(pw_rollout_lane_kernel<4>, grid, block, 0, st, r); break;
      case 8: hipLaunchKernelGGL(pw_rollout_lane_kernel<8>, grid, block, 0, st, r); break;
      case 16: hipLaunchKernelGGL(pw_rollout_lane_kernel<16>, grid, block, 0, st, r); break;
      default: hipLaunchKernelGGL(pw_rollout_lane_kernel<32>, grid, block, 0, st, r); break;
    }
  } else {
    launch_group(e, r, batch, st);
  }
  prof.close();
  return check_launch("pw_rollout");
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_batch_bind(PwEngine* e, const int32_t* puzzle_id, int32_t batch, int64_t* info, void* stream) try {
  if (!e) return pw_fail(PW_EINVAL, "null engine");
  if (e->mailbox) return pw_fail(PW_EINVAL, "pw_batch_bind: this engine has an open mailbox (pw_mailbox_close first)");
  if (batch <= 0 || !puzzle_id) return pw_fail(PW_EINVAL, "pw_batch_bind: puzzle_id must be a device buffer of batch > 0 ids");
  PwDeviceGuard guard(e->set->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  e->ret.valid = e->ret.shown_valid = false;  // (established again by the next full render of the new binding into a buffer of pw_obs_alloc)
  if (!e->d_seg_dir || e->seg_puzzles == 0) {  // nothing to bind to (PW_OPT_STEP_TABLES never): every call stays unbound
    if (hipStreamSynchronize(st) != hipSuccess) return pw_fail(PW_EDEVICE, "pw_batch_bind: stream synchronisation failed");
    release_bind(e);
    if (info) info[0] = info[1] = info[2] = info[3] = info[4] = info[5] = 0;
    return PW_OK;
  }
  const int P = e->set->count;
  const int min_envs = e->bind_min_envs > 0 ? e->bind_min_envs : 48;
  const int epw_log2 = (e->bind_spread & 15) > 0 ? (e->bind_spread & 15) - 1 : 0;  // (PW_OPT_BIND_SPREAD: 0 = automatic = none so far)
  const int mepw_log2 = (e->bind_spread >> 4) > 0 ? std::min((e->bind_spread >> 4) - 1, 4) : std::min(epw_log2, 4);  // (... of the listed environments)
  if (!e->bind || e->bind->batch != batch || e->bind->min_envs != min_envs || e->bind->epw_log2 != epw_log2 || e->bind->mepw_log2 != mepw_log2) {
    if (hipDeviceSynchronize() != hipSuccess) return pw_fail(PW_EDEVICE, "pw_batch_bind: device synchronisation failed");  // nothing in flight reads the old list
    release_bind(e);
    std::unique_ptr<PwBind> b(new PwBind());
    b->puzzle_id = puzzle_id;
    b->batch = batch;
    b->min_envs = min_envs;
    b->epw_log2 = epw_log2;
    b->mepw_log2 = mepw_log2;
    b->seg_cap = batch / (PW_SEG_ENVS >> std::max(3, epw_log2)) + std::min(P, batch / min_envs) + 1;  // (segments of 32 .. 256 environments: 8 .. 1 lanes each; fewer when spread)
    b->d_ints = nullptr;
    b->d_bound = nullptr;
    b->d_segs = nullptr;
    const size_t n_ints = static_cast<size_t>(5) * P + static_cast<size_t>(4) * batch + 16;
    hipError_t err = hipMalloc(reinterpret_cast<void**>(&b->d_ints), n_ints * 4);
    if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&b->d_bound), static_cast<size_t>(batch));
    if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&b->d_segs), static_cast<size_t>(b->seg_cap) * sizeof(PwSegDesc));
    if (err != hipSuccess) {
      if (b->d_ints) (void)hipFree(b->d_ints);
      if (b->d_bound) (void)hipFree(b->d_bound);
      if (b->d_segs) (void)hipFree(b->d_segs);
      return pw_fail(PW_ENOMEM, std::string("pw_batch_bind: ") + hipGetErrorString(err));
    }
    b->cnt = b->d_ints;
    b->mn = b->cnt + P;
    b->mx = b->mn + P;
    b->seg_base = b->mx + P;
    b->perm_base = b->seg_base + P;
    b->rank = b->perm_base + P;
    b->perm = b->rank + batch;
    b->mlist = b->perm + batch;   // [batch][2]
    b->meta = b->mlist + 2 * static_cast<size_t>(batch);
    e->bind = b.release();
  }
  PwBind* b = e->bind;
  b->puzzle_id = puzzle_id;
  bind_launch(e, st);
  // the live pages of this assignment in a library-owned observation buffer; their number comes back with the segment count
  const bool have_live = live_build(e, puzzle_id, batch, st, true);
  uint32_t n_live = 0;
  int32_t meta[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  hipError_t err = hipMemcpyAsync(meta, b->meta, sizeof(meta), hipMemcpyDeviceToHost, st);
  if (err == hipSuccess && have_live) err = hipMemcpyAsync(&n_live, e->ret.d_count, 4, hipMemcpyDeviceToHost, st);
  if (err == hipSuccess) err = hipStreamSynchronize(st);
  if (err != hipSuccess) {
    e->ret.list_pid = nullptr;
    release_bind(e);
    return pw_fail(PW_EDEVICE, std::string("pw_batch_bind: ") + hipGetErrorString(err));
  }
  if (have_live) e->ret.n_live = n_live;
  for (int i = 0; i < 4; i++) b->info[i] = meta[i];
  b->seg_grid = std::max(meta[0], 1);  // (a grid of at least one workgroup: a batch without any segment launches one that leaves)
  b->lds_bytes = static_cast<uint32_t>(meta[4]);
  b->lds_bytes0 = static_cast<uint32_t>(meta[7]);
  b->multi_envs = meta[5];
  b->multi_slot = static_cast<uint32_t>(meta[6]);
  if (info) {
    for (int i = 0; i < 4; i++) info[i] = b->info[i];
    info[4] = meta[5];
    info[5] = meta[6];
  }
  return check_launch("pw_batch_bind");
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_batch_unbind(PwEngine* e) try {
  if (!e) return pw_fail(PW_EINVAL, "null engine");
  e->ret.valid = e->ret.shown_valid = false;
  if (!e->bind) return PW_OK;
  // (its resident kernel may be running the binding's segments -- and the synchronisation below would wait for its idle limit)
  if (e->mailbox) return pw_fail(PW_EINVAL, "pw_batch_unbind: this engine has an open mailbox (pw_mailbox_close first)");
  PwDeviceGuard guard(e->set->device);
  if (hipDeviceSynchronize() != hipSuccess) return pw_fail(PW_EDEVICE, "pw_batch_unbind: device synchronisation failed");
  release_bind(e);
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

}  // extern "C"

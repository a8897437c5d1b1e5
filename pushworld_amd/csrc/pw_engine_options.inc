// pw_engine_options.inc -- the engine options (PW_OPT_*, include/pushworld_amd.h): ONE table row per option, from which
// pw_engine_set_option and pw_engine_get_option both answer, the few options that are code as named cases next to it, and
// pw_engine_profile_read.  Part of the single translation unit pw_kernels.hip, the last of the engine files: included after
// pw_mailbox.inc (mailbox_form_of); uses upload_overlap_tables (pw_engine.inc), step_lane_batch_default (pw_engine_step.inc)
// and pw_value_ok (pw_hostlib_pure.h).
//
// A new option: its #define in the header, its field in PwEngine, its name in _capi.OPTIONS -- and one row here.

namespace pw_opt {

// where an option's value lives: one of the four is set (none: the getter computes it, kOptionRows below)
struct PwOptField {
  int PwEngine::*i;
  int64_t PwEngine::*l;
  bool PwEngine::*b;
  int PwRetained::*r;  // of PwEngine::ret
};
static constexpr PwOptField at(int PwEngine::*p) { return {p, nullptr, nullptr, nullptr}; }
static constexpr PwOptField at(int64_t PwEngine::*p) { return {nullptr, p, nullptr, nullptr}; }
static constexpr PwOptField at(bool PwEngine::*p) { return {nullptr, nullptr, p, nullptr}; }
static constexpr PwOptField at(int PwRetained::*p) { return {nullptr, nullptr, nullptr, p}; }
static constexpr PwOptField computed() { return {nullptr, nullptr, nullptr, nullptr}; }

static constexpr PwValueRule range(int64_t lo, int64_t hi) { return {PW_VALUE_RANGE, lo, hi, 0}; }
static constexpr PwValueRule one_of(int64_t a, int64_t b) { return {PW_VALUE_SET, a, b, b}; }
static constexpr PwValueRule one_of(int64_t a, int64_t b, int64_t c) { return {PW_VALUE_SET, a, b, c}; }
static constexpr PwValueRule non_negative() { return {PW_VALUE_NONNEG, 0, 0, 0}; }
static constexpr PwValueRule any_value() { return {PW_VALUE_ANY, 0, 0, 0}; }
static constexpr PwValueRule custom() { return {PW_VALUE_CUSTOM, 0, 0, 0}; }  // option_custom_ok below
static constexpr PwValueRule read_only() { return {PW_VALUE_READ_ONLY, 0, 0, 0}; }

// what else a successful set does
enum PwOptEffect : uint8_t {
  PW_FX_NONE,
  PW_FX_RETAINED,  // the retained observation is no longer established (the next full render establishes it again)
  PW_FX_HAND_SET,  // a launch configuration set by hand holds for the live launch too
};

struct PwOptRow {
  int32_t id;
  PwValueRule accept;
  const char* reject;  // pw_last_error() of a value outside `accept`
  PwOptField field;
  PwOptEffect effect;
};

static const PwOptRow kOptionRows[] = {
    {PW_OPT_STEP_KERNEL, range(0, 2), "PW_OPT_STEP_KERNEL: 0 lane group, 1 wavefront, 2 lane", at(&PwEngine::step_kernel), PW_FX_NONE},
    {PW_OPT_FUSED_STEP_RENDER, any_value(), "", at(&PwEngine::force_fused), PW_FX_RETAINED},
    {PW_OPT_RENDER_KERNEL, range(0, 1), "PW_OPT_RENDER_KERNEL: 0 automatic, 1 per-environment LDS kernel", at(&PwEngine::force_lds_render), PW_FX_RETAINED},
    {PW_OPT_PAGE_SLICE_ENVS, non_negative(), "PW_OPT_PAGE_SLICE_ENVS must be >= 0", at(&PwEngine::page_slice_envs), PW_FX_RETAINED},
    {PW_OPT_SEARCH_CHUNK, non_negative(), "PW_OPT_SEARCH_CHUNK must be >= 0", at(&PwEngine::search_chunk), PW_FX_NONE},
    {PW_OPT_PROFILE_RENDER, range(0, 65536), "PW_OPT_PROFILE_RENDER: 0 .. 65536 launches", computed(), PW_FX_NONE},  // (code: the event pool)
    {PW_OPT_PAGE_ORDER, range(0, 2), "PW_OPT_PAGE_ORDER: 0 address order, 1 eighth per XCD, 2 runs per XCD", at(&PwEngine::page_order), PW_FX_HAND_SET},
    {PW_OPT_PAGE_RUN_LOG2, range(0, 20), "PW_OPT_PAGE_RUN_LOG2: 0 .. 20 (0 .. 2 with page order 1)", at(&PwEngine::page_run_log2), PW_FX_HAND_SET},
    {PW_OPT_PAGE_LDS_PAD_KB, range(0, 48), "PW_OPT_PAGE_LDS_PAD_KB: 0 .. 48", at(&PwEngine::page_lds_pad_kb), PW_FX_HAND_SET},
    {PW_OPT_STEP_LDS_TABLES, range(0, 2), "PW_OPT_STEP_LDS_TABLES: 0 automatic, 1 always, 2 never", at(&PwEngine::step_lds_tables), PW_FX_NONE},  // (code: 1 must fit)
    {PW_OPT_TUNED_NS, read_only(), "", at(&PwEngine::tuned_ns), PW_FX_NONE},
    {PW_OPT_STEP_WIDE_GROUPS, range(0, 1), "PW_OPT_STEP_WIDE_GROUPS: 0 two movables per lane, 1 32-lane groups", at(&PwEngine::step_wide_groups), PW_FX_NONE},
    {PW_OPT_PAGE_LOAD_ALL, range(0, 1), "PW_OPT_PAGE_LOAD_ALL: 0 or 1", at(&PwEngine::page_load_all), PW_FX_HAND_SET},
    {PW_OPT_OBS_CHUNK_MB, range(0, 4096), "PW_OPT_OBS_CHUNK_MB: 0 (the default, 32 MiB) .. 4096", at(&PwEngine::obs_chunk_mb), PW_FX_NONE},
    {PW_OPT_OBS_ACCEPT_GBS, range(0, 100000), "PW_OPT_OBS_ACCEPT_GBS: 0 .. 100000 GB/s", at(&PwEngine::obs_accept_gbs), PW_FX_NONE},
    {PW_OPT_STEP_TABLES, range(0, 3), "PW_OPT_STEP_TABLES: 0 automatic, 1 every puzzle, 2 none, 3 puzzles with big movables", at(&PwEngine::step_tables), PW_FX_NONE},  // (code: the tables are rebuilt)
    {PW_OPT_STEP_TABLE_BYTES, read_only(), "", at(&PwEngine::ovl_bytes), PW_FX_NONE},
    {PW_OPT_STEP_TABLE_PUZZLES, read_only(), "", at(&PwEngine::ovl_puzzles), PW_FX_NONE},
    {PW_OPT_STEP_NARROW_GROUPS, range(0, 2), "PW_OPT_STEP_NARROW_GROUPS: 0 automatic, 1 always, 2 never", at(&PwEngine::step_narrow_groups), PW_FX_NONE},
    {PW_OPT_STEP_BLOCK_ORDER, range(0, 3), "PW_OPT_STEP_BLOCK_ORDER: 0 first environments first, 1 last first, + 2 a contiguous eighth per XCD", at(&PwEngine::step_reverse), PW_FX_NONE},
    {PW_OPT_STEP_LANE_BATCH, non_negative(), "PW_OPT_STEP_LANE_BATCH: 0 default, otherwise the smallest batch that runs one lane per environment", at(&PwEngine::step_lane_batch), PW_FX_NONE},  // (get: 0 reads as the default)
    {PW_OPT_STEP_BOARDS, one_of(0, 2), "PW_OPT_STEP_BOARDS: 0 automatic, 2 never", at(&PwEngine::step_boards), PW_FX_NONE},
    {PW_OPT_STEP_BOARD_SET, read_only(), "", computed(), PW_FX_NONE},
    {PW_OPT_EXPAND_LDS_TABLES, one_of(0, 2, 3), "PW_OPT_EXPAND_LDS_TABLES: 0 automatic, 2 never, 3 never + whole runs", at(&PwEngine::expand_lds_tables), PW_FX_NONE},
    {PW_OPT_EXPAND_TILE_ORDER, range(0, 3), "PW_OPT_EXPAND_TILE_ORDER: 0 interleaved, 1 a contiguous eighth per XCD (+ 2: plain instead of non-temporal stores)", at(&PwEngine::expand_tile_order), PW_FX_NONE},
    {PW_OPT_EXPAND_PREFETCH, one_of(-1, 0, 2), "PW_OPT_EXPAND_PREFETCH: -1 automatic (= 2), 0 none, 2 two tiles ahead", at(&PwEngine::expand_prefetch), PW_FX_NONE},
    {PW_OPT_EXPAND_GROUPS_PER_CU, range(0, 64), "PW_OPT_EXPAND_GROUPS_PER_CU: 0 automatic, 1 .. 64", at(&PwEngine::expand_groups_per_cu), PW_FX_NONE},
    {PW_OPT_SEARCH_BATCH_GROUPS_PER_CU, range(0, 8), "PW_OPT_SEARCH_BATCH_GROUPS_PER_CU: 0 automatic, 1 .. 8", at(&PwEngine::search_batch_groups_per_cu), PW_FX_NONE},
    {PW_OPT_EXPAND_WG_WAVES, one_of(0, 4, 8), "PW_OPT_EXPAND_WG_WAVES: 0 automatic, 4, 8", at(&PwEngine::expand_wg_waves), PW_FX_NONE},
    {PW_OPT_STEP_MIXED_GROUPS, one_of(0, 2), "PW_OPT_STEP_MIXED_GROUPS: 0 automatic, 2 never", at(&PwEngine::step_mixed), PW_FX_NONE},
    {PW_OPT_STEP_QUAD16, one_of(0, 2), "PW_OPT_STEP_QUAD16: 0 automatic, 2 never", at(&PwEngine::step_quad16), PW_FX_NONE},
    {PW_OPT_STEP_QUAD16_PUZZLES, read_only(), "", at(&PwEngine::quad_puzzles), PW_FX_NONE},
    {PW_OPT_SEARCH_KEYS, range(0, 1), "PW_OPT_SEARCH_KEYS: 0 fingerprinted entries, 1 exact keys where they fit", at(&PwEngine::search_keys), PW_FX_NONE},
    {PW_OPT_EXPAND_PAIR_DIMS, one_of(0, 2), "PW_OPT_EXPAND_PAIR_DIMS: 0 automatic, 2 never", at(&PwEngine::expand_pair_dims), PW_FX_NONE},
    {PW_OPT_MAILBOX_MODE, custom(), "PW_OPT_MAILBOX_MODE: 0 .. 3 (+ 4), or 11; + 16 profile", at(&PwEngine::mailbox_mode), PW_FX_NONE},
    {PW_OPT_BIND_MIN_ENVS, range(0, 65536), "PW_OPT_BIND_MIN_ENVS: 0 default (48), else 1 .. 65536", at(&PwEngine::bind_min_envs), PW_FX_NONE},  // (get: 0 reads as 48)
    {PW_OPT_BIND_FUSED, one_of(0, 2), "PW_OPT_BIND_FUSED: 0 automatic, 2 never", at(&PwEngine::bind_fused), PW_FX_NONE},
    {PW_OPT_BIND_PUZZLES, read_only(), "", at(&PwEngine::seg_puzzles), PW_FX_NONE},
    {PW_OPT_BIND_MISMATCHES, read_only(), "", computed(), PW_FX_NONE},
    {PW_OPT_OBS_TUNE_MS, non_negative(), "PW_OPT_OBS_TUNE_MS: milliseconds (0 = default 10 000)", at(&PwEngine::obs_tune_ms), PW_FX_NONE},  // (get: 0 reads as 10 000)
    {PW_OPT_OBS_SCREEN_MS, read_only(), "", at(&PwEngine::obs_screen_ms), PW_FX_NONE},
    {PW_OPT_BIND_LANES, range(0, 4), "PW_OPT_BIND_LANES: 0 automatic, 1 / 2 / 3 / 4 = at most 1 / 2 / 4 / 8 lanes per environment", at(&PwEngine::bind_lanes), PW_FX_NONE},
    {PW_OPT_BIND_ROLLOUTS, range(0, 2), "PW_OPT_BIND_ROLLOUTS: 0 automatic, 1 always, 2 never", at(&PwEngine::bind_rollouts), PW_FX_NONE},
    {PW_OPT_BIND_MAX_KB, range(0, 48), "PW_OPT_BIND_MAX_KB: 0 default (48), else 1 .. 48", at(&PwEngine::bind_max_kb), PW_FX_NONE},  // (get: 0 reads as 48)
    {PW_OPT_BIND_SPREAD, custom(), "PW_OPT_BIND_SPREAD: 0 automatic, 1 .. 5 = at most 64 / 32 / 16 / 8 / 4 environments per wavefront (+ 16 x the same for the listed environments)", at(&PwEngine::bind_spread), PW_FX_NONE},
    {PW_OPT_STEP_ONE_FUSED, range(0, 2), "PW_OPT_STEP_ONE_FUSED: 0, 1 or 2", at(&PwEngine::step_one_fused), PW_FX_NONE},
    {PW_OPT_MAILBOX_SEG, one_of(0, 2), "PW_OPT_MAILBOX_SEG: 0 automatic, 2 never", at(&PwEngine::mailbox_seg), PW_FX_NONE},
    {PW_OPT_MAILBOX_FORM, read_only(), "", computed(), PW_FX_NONE},
    {PW_OPT_STEP_ONE_APPLIES, read_only(), "", computed(), PW_FX_NONE},
    {PW_OPT_EXPAND_FORM, read_only(), "", at(&PwEngine::expand_form), PW_FX_NONE},
    {PW_OPT_CELLS_BASE_BYTES, read_only(), "", at(&PwEngine::cells_base_bytes), PW_FX_NONE},
    {PW_OPT_PUSH_SEARCH_FP_BITS, range(0, 32), "PW_OPT_PUSH_SEARCH_FP_BITS: 0 default, 1 .. 32 fingerprint bits", at(&PwEngine::push_search_fp_bits), PW_FX_NONE},
    {PW_OPT_OBS_PADDING_ONCE, range(0, 3), "PW_OPT_OBS_PADDING_ONCE: 0 off, 1 on (2 / 3: on, with the early-exit / the list form of the live launch)", at(&PwRetained::option), PW_FX_RETAINED},
    {PW_OPT_OBS_LIVE_PAGES, read_only(), "", computed(), PW_FX_NONE},
    {PW_OPT_RESAMPLE_FENCE, range(0, 1), "PW_OPT_RESAMPLE_FENCE: 0 the search reads the cdf alone, 1 a fence in LDS", at(&PwEngine::resample_fence), PW_FX_NONE},
    {PW_OPT_STATS_LDS_PUZZLES, custom(), "PW_OPT_STATS_LDS_PUZZLES: 0 default, 1 .. 1024 puzzles, 2048 never", at(&PwEngine::stats_lds_puzzles), PW_FX_NONE},
    {PW_OPT_STATS_GROUPS, range(0, 1 << 20), "PW_OPT_STATS_GROUPS: 0 one workgroup per 256 environments, or the most workgroups of a launch", at(&PwEngine::stats_groups), PW_FX_NONE},
    {PW_OPT_OBS_CHANGED_PAGES, range(0, 1), "PW_OPT_OBS_CHANGED_PAGES: 0 the live launch, 1 the changed pages of it only", at(&PwRetained::chg_option), PW_FX_NONE},  // (code: `shown` alone ends)
};

static const PwOptRow* option_row(int32_t option) {
  for (const PwOptRow& r : kOptionRows)
    if (r.id == option) return &r;
  return nullptr;
}

// the three rules that are neither a range nor a small set
static bool option_custom_ok(int32_t option, int64_t value) {
  switch (option) {
    case PW_OPT_MAILBOX_MODE: return !(value < 0 || value > 31 || ((value & 8) && (value & 7) != 3));
    case PW_OPT_BIND_SPREAD: return !(value < 0 || (value & 15) > 5 || (value >> 4) > 5);
    case PW_OPT_STATS_LDS_PUZZLES: return !(value < 0 || (value > 1024 && value != 2048));
    default: return false;
  }
}

}  // namespace pw_opt

extern "C" {

int pw_engine_set_option(PwEngine* e, int32_t option, int64_t value) try {
  if (!e) return pw_fail(PW_EINVAL, "null engine");
  const pw_opt::PwOptRow* r = pw_opt::option_row(option);
  if (!r) return pw_fail(PW_EINVAL, "unknown engine option");
  if (r->accept.kind == PW_VALUE_READ_ONLY) return pw_fail(PW_EINVAL, "read-only option");
  if (!(r->accept.kind == PW_VALUE_CUSTOM ? pw_opt::option_custom_ok(option, value) : pw_value_ok(r->accept, value)))
    return pw_fail(PW_EINVAL, r->reject);
  switch (option) {  // the options whose set is code
    case PW_OPT_STEP_LDS_TABLES:
      if (value == 1 && !e->lds_tables_fit)
        return pw_fail(PW_ELIMIT, "PW_OPT_STEP_LDS_TABLES: a puzzle of the set has more than 128 shape rows");
      break;
    case PW_OPT_STEP_TABLES: {
      if (static_cast<int>(value) == e->step_tables) return PW_OK;
      PwDeviceGuard guard(e->set->device);
      e->step_tables = static_cast<int>(value);
      return upload_overlap_tables(e);  // rebuilt on the spot (synchronises the device)
    }
    case PW_OPT_PROFILE_RENDER: {
      PwDeviceGuard guard(e->set->device);
      for (hipEvent_t ev : e->prof_events) (void)hipEventDestroy(ev);
      e->prof_events.clear();
      e->prof_used = 0;
      for (int64_t i = 0; i < 2 * value; i++) {
        hipEvent_t ev;
        if (hipEventCreate(&ev) != hipSuccess) return pw_fail(PW_EDEVICE, "PW_OPT_PROFILE_RENDER: hipEventCreate failed");
        e->prof_events.push_back(ev);
      }
      return PW_OK;
    }
    case PW_OPT_OBS_CHANGED_PAGES:
      e->ret.shown_valid = false;  // (the next pw_step_render into the retained buffer takes the live launch and fills `shown`)
      break;
    default: break;
  }
  const pw_opt::PwOptField& f = r->field;
  if (f.i) e->*f.i = static_cast<int>(value);
  else if (f.l) e->*f.l = value;
  else if (f.b) e->*f.b = value != 0;
  else e->ret.*f.r = static_cast<int>(value);
  if (r->effect == pw_opt::PW_FX_RETAINED) e->ret.valid = e->ret.shown_valid = false;
  if (r->effect == pw_opt::PW_FX_HAND_SET) e->ret.tuned = false;
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int64_t pw_engine_get_option(const PwEngine* e, int32_t option) try {
  if (!e) return pw_fail(PW_EINVAL, "null engine");
  switch (option) {  // the options whose get is code: a default in place of 0, a computed value, a word of the device
    case PW_OPT_BIND_MIN_ENVS: return e->bind_min_envs > 0 ? e->bind_min_envs : 48;
    case PW_OPT_BIND_MAX_KB: return e->bind_max_kb > 0 ? e->bind_max_kb : 48;
    case PW_OPT_OBS_TUNE_MS: return e->obs_tune_ms > 0 ? e->obs_tune_ms : 10000;
    case PW_OPT_STEP_LANE_BATCH: return e->step_lane_batch == 0 ? step_lane_batch_default(e, false) : e->step_lane_batch;
    case PW_OPT_STEP_ONE_APPLIES:
      return (!e->fast_u8_ppc3 && e->step_kernel == 0 && !e->force_fused && e->step_one_fused && e->obs_bytes >= (64 << 10)) ? 1 : 0;
    case PW_OPT_MAILBOX_FORM: return mailbox_form_of(e);
    case PW_OPT_STEP_BOARD_SET: return e->d_boards ? 1 : 0;
    case PW_OPT_PROFILE_RENDER: return static_cast<int64_t>(e->prof_events.size() / 2);
    case PW_OPT_BIND_MISMATCHES: {
      uint32_t n = 0;
      PwDeviceGuard guard(e->set->device);
      if (hipMemcpy(&n, e->d_scratch + 8, 4, hipMemcpyDeviceToHost) != hipSuccess) return pw_fail(PW_EDEVICE, "PW_OPT_BIND_MISMATCHES: copy failed");
      return n;
    }
    case PW_OPT_OBS_LIVE_PAGES: {
      if (!e->ret.valid) return 0;
      if (e->ret.n_live >= 0) return e->ret.n_live;
      uint32_t n = 0;  // (list rebuilt in-stream: its length is on the device)
      PwDeviceGuard guard(e->set->device);
      if (hipMemcpy(&n, e->ret.d_count, 4, hipMemcpyDeviceToHost) != hipSuccess) return pw_fail(PW_EDEVICE, "PW_OPT_OBS_LIVE_PAGES: copy failed");
      return n;
    }
    default: break;
  }
  const pw_opt::PwOptRow* r = pw_opt::option_row(option);
  if (!r) return pw_fail(PW_EINVAL, "unknown engine option");
  const pw_opt::PwOptField& f = r->field;
  return f.i ? e->*f.i : f.l ? e->*f.l : f.b ? (e->*f.b ? 1 : 0) : e->ret.*f.r;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_engine_profile_read(PwEngine* e, float* ms, int32_t cap) try {
  if (!e || (!ms && cap > 0)) return pw_fail(PW_EINVAL, "null argument");
  PwDeviceGuard guard(e->set->device);
  const int n = e->prof_used;
  for (int i = 0; i < n; i++) {
    hipError_t err = hipEventSynchronize(e->prof_events[2 * i + 1]);
    float t = 0.0f;
    if (err == hipSuccess) err = hipEventElapsedTime(&t, e->prof_events[2 * i], e->prof_events[2 * i + 1]);
    if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string("pw_engine_profile_read: ") + hipGetErrorString(err));
    if (i < cap) ms[i] = t;
  }
  e->prof_used = 0;
  return n;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

}  // extern "C"

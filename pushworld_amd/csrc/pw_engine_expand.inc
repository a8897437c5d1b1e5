// pw_engine_expand.inc -- pw_expand4: which instance of the expansion kernels (pw_expand_kernels.inc) a frontier takes, on
// which grid, and the word PW_OPT_EXPAND_FORM reports about it.  Part of the single translation unit pw_kernels.hip, included
// after pw_engine_render.inc: uses RenderProfScope from there, the push-table limits of pw_engine.inc and check_launch.

extern "C" {

static constexpr int64_t kExpandLaneStates = 131072;  // pw_expand4: frontiers from this size on run one lane per state

// PW_OPT_EXPAND_FORM: which kernel instance and grid a pw_expand4 launch used, packed as include/pushworld_amd.h lays it out
static int64_t expand_form_word(int family, int n, bool pipe, bool nt, bool pair_dims, int waves, int tile_order, bool persistent,
                                int64_t groups) {
  return static_cast<int64_t>(family) | (static_cast<int64_t>(n) << 8) | (pipe ? 1ll << 16 : 0) | (nt ? 1ll << 17 : 0) |
         (pair_dims ? 1ll << 18 : 0) | (static_cast<int64_t>(waves) << 20) | (static_cast<int64_t>(tile_order) << 24) |
         (persistent ? 1ll << 25 : 0) | (groups << 32);
}

int pw_expand4(PwEngine* e, int32_t puzzle, const int32_t* states, int32_t* succ, uint32_t* moved, uint8_t* goal,
               int32_t num_states, void* stream) try {
  if (!e) return pw_fail(PW_EINVAL, "null engine");
  if (puzzle < 0 || puzzle >= e->set->count) return pw_fail(PW_EINVAL, "puzzle index out of range");
  if (num_states <= 0) return PW_OK;
  if (!states || !succ || !moved || !goal) return pw_fail(PW_EINVAL, "null argument");
  PwDeviceGuard guard(e->set->device);
  ExpandArgs a{e->set->d_headers, e->set->d_blob, puzzle, states, succ, moved, goal, num_states, e->d_ovl, e->d_ovl_dir,
               e->d_push_dir};
  const bool push_tab = !e->push_has.empty() && e->push_has[static_cast<size_t>(puzzle)];  // ... and push tables
  const bool tab = !e->ovl_has.empty() && e->ovl_has[static_cast<size_t>(puzzle)];  // this puzzle has overlap tables
  hipStream_t st = static_cast<hipStream_t>(stream);
  RenderProfScope prof(e, st);  // PW_OPT_PROFILE_RENDER: the expansion launch
  const int n = e->set->headers[puzzle].N;
  const dim3 g8(static_cast<unsigned>((num_states + 31) / 32)), g16(static_cast<unsigned>((num_states + 15) / 16)),
      g32(static_cast<unsigned>((num_states + 7) / 8)), block(256);
  // One lane per parent state (pw_expand4_lane_kernel) once the frontier alone fills the chip: puzzles with push tables
  // (engines of at most 64 puzzles) (LDS: 4 N + 44 bytes per state and action staged at a time), PW_OPT_STEP_KERNEL lane or at
  // least PW_OPT_STEP_LANE_BATCH states
  const int64_t lane_from = e->step_lane_batch == 0 ? kExpandLaneStates : e->step_lane_batch;
  const bool lanes = push_tab && n <= 32 && (e->step_kernel == 2 || (e->step_kernel == 0 && num_states >= lane_from));
  // ... with the tables in LDS where they fit and the buffers are aligned for whole-row vector accesses (pw_expand4_v2_kernel)
  // pair tables sized per pair where the engine built them (uniform tables beyond 16 KB; PW_OPT_EXPAND_PAIR_DIMS 2 = never)
  bool pair_dims = false, byte_tables = false;
  if (push_tab) {
    const PwPushDir& pd0 = e->push_host[static_cast<size_t>(puzzle)];
    pair_dims = pd0.pairp_off != 0u && n >= 7 && e->expand_pair_dims != 2 && (pd0.pairb_off == 0u || pd0.pairb_bytes > kPairDimsFrom);
    // (PW_OPT_EXPAND_PAIR_DIMS never: set-wide tables, or -- where those do not fit LDS -- the lane kernel)
    byte_tables = pair_dims || pd0.pairb_off != 0u;
  }
  if (lanes && e->expand_lds_tables == 0 && n >= 2 && (n <= 16 || (pair_dims && n <= kPairDimsMaxN)) && byte_tables &&
      static_cast<int64_t>(num_states) <= static_cast<int64_t>(INT32_MAX) - 64 &&  // (the kernel's state indices are 32-bit)
      reinterpret_cast<uintptr_t>(states) % (4u * static_cast<unsigned>(pw_expand2_load_width(n))) == 0 &&
      reinterpret_cast<uintptr_t>(succ) % 16 == 0 && reinterpret_cast<uintptr_t>(moved) % 16 == 0 &&
      reinterpret_cast<uintptr_t>(goal) % 4 == 0) {
    const PwPushDir& pd = e->push_host[static_cast<size_t>(puzzle)];
    Expand2Args x;
    x.a = a;
    auto up16 = [](uint32_t v) { return (v + 15u) & ~15u; };
    x.lds_wall = up16(pair_dims ? pd.pairp_bytes : pd.pairb_bytes);
    x.lds_obj = up16(x.lds_wall + static_cast<uint32_t>(n) * pd.Hs * pd.WW * 4u);
    x.lds_reach = up16(x.lds_obj + (n > 16 ? 128u : 64u));  // (4 bytes of PwObjDesc per movable)
    x.lds_wave = n > 16 ? up16(x.lds_reach + 48u * static_cast<uint32_t>(n)) : x.lds_reach;  // (17 .. 20 movables: 12 dwords of reach bytes per pusher)
    // ---- how many workgroups (4 wavefronts each, striding over the 64-state tiles), and which kernel
    // A workgroup pays for its own copy of the tables (L2 -> LDS, table_bytes); what it buys with MANY small workgroups is
    // the dispatcher's load balance: with few tiles per wavefront the tiles are handed out as wavefronts finish, instead of
    // every wavefront owning the same number of tiles whatever its CU's luck with the memory channels.  On 4 M-state
    // frontiers (sessions E, G, I, K, M of profiles/r04_expand4_variants.txt) the best grids are those whose table copies
    // stay near a tenth of the HBM bytes of the workgroup's tiles:
    //   tiles per wavefront k = the smallest with table bytes <= 0.11 x (4 k tiles' bytes); k <= 4: that grid, kPipe 0
    //     (N = 3: k = 1, 0.72 -> 0.83 of peak; N = 8 / 7 KB: k = 2, 0.80 -> 0.85; N = 8 / 16 KB: k = 4, 0.69 -> 0.81);
    //   otherwise persistent workgroups: 8 per CU (those that do not fit at once queue up and even out the tail) for tables
    //     up to 32 KB; beyond, exactly as many as are resident at this LDS footprint, at most 2 per CU (a 50-100 KB copy per
    //     workgroup: N = 8 / 50 KB: 0.78 at 2 per CU, 0.61 at one workgroup per 8 tiles; N = 16 / 58 KB: 0.47 at 1, 0.43 at 8).
    // kPipe 1 (stores one tile late) stages a whole tile: only for persistent workgroups, and only where it leaves room for
    // two workgroups per CU (78 KB each).  PW_OPT_EXPAND_PREFETCH 0 / 2 and PW_OPT_EXPAND_GROUPS_PER_CU > 0 (persistent, that
    // many per CU) override.
    const int64_t tiles = (static_cast<int64_t>(num_states) + 63) / 64;
    int64_t blocks = (tiles + 3) / 4;
    const size_t table_bytes = x.lds_wave;
    const double group_tile_bytes = 4.0 * 64.0 * (20.0 * n + 20.0);  // HBM bytes of one tile per wavefront of a workgroup
    int tiles_per_wave = static_cast<int>(std::ceil(static_cast<double>(table_bytes) / (0.11 * group_tile_bytes)));
    if (tiles_per_wave < 1) tiles_per_wave = 1;
    if (tiles_per_wave > 4 || e->expand_groups_per_cu > 0) tiles_per_wave = 0;  // 0: persistent
    bool pipe = e->expand_prefetch == -1 ? tiles_per_wave == 0 : e->expand_prefetch != 0;
    if (n > 16) pipe = false;  // (17 .. 20 movables: one instance each -- 4 wavefronts, stores at the tile's end)
    size_t lds = 0;
    for (int attempt = 0; attempt < 2; attempt++) {
      x.stage_bytes = 16u * static_cast<uint32_t>(pw_expand2_stage_pieces(n, pipe));
      x.wave_bytes = up16(x.stage_bytes + 64u * static_cast<uint32_t>(((n + 1) / 2) | 1) * 4u);
      lds = x.lds_wave + 4u * static_cast<size_t>(x.wave_bytes);
      if (!pipe || lds <= 78u * 1024u) break;  // (two of them in the 156 KB a CU gives out)
      pipe = false;
    }
    x.tile_order = e->expand_tile_order & 1;
    const bool nt = !(e->expand_tile_order & 2);  // (PW_OPT_EXPAND_TILE_ORDER + 2: plain stores, A/B runs only)
    if (lds <= 156u * 1024u) {
      const int64_t resident = std::max<int64_t>(1, static_cast<int64_t>((156u * 1024u) / lds));
      // one workgroup per CU: 8 wavefronts instead of 4 share the copy of the tables where their staging fits too -- N = 16 /
      // 58 KB: 0.47 -> 0.63 of peak, N = 8 / 69 KB: 0.39 -> 0.58 (session L)
      int waves = 4;
      if (resident == 1 && !pipe && n <= 16) {  // (lds beyond 78 KB: the loop above has switched the pipeline off)
        for (int w = 8; w > 4; w -= 4)
          if (x.lds_wave + static_cast<size_t>(w) * x.wave_bytes <= 156u * 1024u) {
            waves = w;
            break;
          }
        const int cap = e->expand_groups_per_cu > 0 ? 0 : static_cast<int>(e->expand_wg_waves);  // (A/B: PW_OPT_EXPAND_WG_WAVES)
        if (cap >= 4 && cap < waves) waves = cap;
        lds = x.lds_wave + static_cast<size_t>(waves) * x.wave_bytes;
        blocks = (tiles + waves - 1) / waves;
      }
      int64_t groups;
      if (e->expand_groups_per_cu > 0) groups = std::min<int64_t>(blocks, static_cast<int64_t>(e->num_cus) * e->expand_groups_per_cu);
      else if (tiles_per_wave > 0)  // (a small frontier still fills the chip: at least 8 workgroups per CU while there are tiles)
        groups = std::max<int64_t>((blocks + tiles_per_wave - 1) / tiles_per_wave, std::min<int64_t>(blocks, static_cast<int64_t>(e->num_cus) * 8));
      else groups = std::min<int64_t>(blocks, static_cast<int64_t>(e->num_cus) * (table_bytes <= 32u * 1024u ? 8 : std::min<int64_t>(2, resident)));
      // tile order 1: workgroup b sweeps the eighth b mod 8 of the tiles -- with fewer than 8 workgroups (frontiers of fewer
      // than 8 blocks) the other eighths would have none; the extra workgroups of a small frontier find no tiles of their own
      if (x.tile_order == 1 && groups < 8) groups = 8;
      const dim3 grid(static_cast<unsigned>(groups)), block(static_cast<unsigned>(64 * waves));
      // (kPipe 0 instances store non-temporally, and so do all per-pair ones: 17 .. 20 movables among them)
      e->expand_form = expand_form_word(n > 16 ? 5 : (waves == 8 ? 4 : 3), n, pipe, nt || !pipe || pair_dims, pair_dims, waves,
                                        x.tile_order, tiles_per_wave == 0, groups);
#define PW_X2P(K) /* per-pair table dimensions (7 .. 16 movables): the same grids; no plain-store A/B instance */          \
  case K: {                                                                                                               \
    const void* fn = waves == 8 ? reinterpret_cast<const void*>(pw_expand4_v2w_kernel<K, true>)                           \
                     : (!pipe ? reinterpret_cast<const void*>(pw_expand4_v2_kernel<K, 0, true, true>)                     \
                              : reinterpret_cast<const void*>(pw_expand4_v2_kernel<K, 1, true, true>));                   \
    if (lds > 64u * 1024u) (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)); \
    if (waves == 8) hipLaunchKernelGGL((pw_expand4_v2w_kernel<K, true>), grid, block, lds, st, x);                        \
    else if (!pipe) hipLaunchKernelGGL((pw_expand4_v2_kernel<K, 0, true, true>), grid, block, lds, st, x);                \
    else hipLaunchKernelGGL((pw_expand4_v2_kernel<K, 1, true, true>), grid, block, lds, st, x);                           \
    break;                                                                                                                \
  }
#define PW_X2Q(K) /* 17 .. 20 movables (128-bit work word, per-pair tables), registers capped for 3 wavefronts per SIMD */   \
  case K: {                                                                                                               \
    const void* fn = reinterpret_cast<const void*>(pw_expand4_v2q_kernel<K>);                                             \
    if (lds > 64u * 1024u) (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)); \
    hipLaunchKernelGGL((pw_expand4_v2q_kernel<K>), grid, block, lds, st, x);                                              \
    break;                                                                                                                \
  }
#define PW_X2(K)                                                                                                          \
  case K: {                                                                                                               \
    const void* fn = waves == 8 ? reinterpret_cast<const void*>(pw_expand4_v2w_kernel<K>)                                 \
                     : (!pipe ? reinterpret_cast<const void*>(pw_expand4_v2_kernel<K, 0, true>)                           \
                              : (nt ? reinterpret_cast<const void*>(pw_expand4_v2_kernel<K, 1, true>)                     \
                                    : reinterpret_cast<const void*>(pw_expand4_v2_kernel<K, 1, false>)));                 \
    if (lds > 64u * 1024u) (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(lds)); \
    if (waves == 8) hipLaunchKernelGGL((pw_expand4_v2w_kernel<K>), grid, block, lds, st, x);                              \
    else if (!pipe) hipLaunchKernelGGL((pw_expand4_v2_kernel<K, 0, true>), grid, block, lds, st, x);                      \
    else if (nt) hipLaunchKernelGGL((pw_expand4_v2_kernel<K, 1, true>), grid, block, lds, st, x);                         \
    else hipLaunchKernelGGL((pw_expand4_v2_kernel<K, 1, false>), grid, block, lds, st, x);                                \
    break;                                                                                                                \
  }
      if (n > 16) {
        switch (n) {
          PW_X2Q(17) PW_X2Q(18) PW_X2Q(19) PW_X2Q(20)
          default: break;
        }
      } else if (pair_dims) {
        switch (n) {
          PW_X2P(7) PW_X2P(8) PW_X2P(9) PW_X2P(10) PW_X2P(11) PW_X2P(12) PW_X2P(13) PW_X2P(14) PW_X2P(15) PW_X2P(16)
          default: break;
        }
      } else {
        switch (n) {
          PW_X2(2) PW_X2(3) PW_X2(4) PW_X2(5) PW_X2(6) PW_X2(7) PW_X2(8) PW_X2(9) PW_X2(10) PW_X2(11) PW_X2(12) PW_X2(13) PW_X2(14)
          PW_X2(15) PW_X2(16)
          default: break;
        }
      }
#undef PW_X2
#undef PW_X2P
#undef PW_X2Q
      prof.close();
      return check_launch("pw_expand4");
    }
  }
  if (lanes) {
    const dim3 grid(static_cast<unsigned>((num_states + 63) / 64)), wave(64);
    // Successors leave through LDS, `per_pass` actions at a time, in stores of `width` ints.  Runs start at multiples of
    // per_pass * N ints: 16-byte stores need that to be a multiple of 4.  Few actions per pass = little LDS = many resident
    // wavefronts (N = 12: 5.6 KB, 7 per SIMD; all four at once: 15 KB, 2 per SIMD and 1.0 instead of 1.4e10 parents/s);
    // odd N beyond 3 go two actions at a time in 8-byte pieces (profiles/r03_expand4_lanes.txt, staging variants).
    const uintptr_t sa = reinterpret_cast<uintptr_t>(succ);
    // Up to 14 movables all four actions are staged at once: a state's successors leave as ONE run, in non-temporal stores
    // (kNT) -- with those, whole runs beat the occupancy that staging fewer actions buys (N = 8: 0.34 -> 0.62 of the HBM
    // peak, N = 12: 0.35 -> 0.45, N = 14: 0.34 -> 0.37; N = 16: 0.38 -> 0.32, i.e. not beyond 14: session J of
    // profiles/r04_expand4_variants.txt).  PW_OPT_EXPAND_LDS_TABLES 3 forces them, 2 keeps round 3's staging.
    int per_pass = 1, width = 1;
    if ((n <= 14 && e->expand_lds_tables != 2) || e->expand_lds_tables == 3) per_pass = 4, width = 4;
    else if (n % 4 == 0) width = 4;
    else if (n % 2 == 0 && n <= 10) per_pass = 2, width = 4;
    else if (n % 2 == 0) width = 2;
    else if (n <= 3) per_pass = 4, width = 4;
    else per_pass = 2, width = 2;  // odd N: pairs of actions in 8-byte pieces (single ints: up to 2x slower, `Armor`, N = 7)
    if (sa % (4 * static_cast<unsigned>(width)) != 0) width = 1;
    const int np_lane = n <= 4 ? 4 : (n <= 8 ? 8 : (n <= 16 ? 16 : 32));  // the kernel instance: positions in LDS take NP / 2 + 1 words
    const size_t lds = static_cast<size_t>(64) * (per_pass * n + 2 + np_lane / 2 + 1) * sizeof(int);
    const bool flags_vec = reinterpret_cast<uintptr_t>(moved) % 16 == 0 && reinterpret_cast<uintptr_t>(goal) % 4 == 0;
    const int vec_out = flags_vec ? width : -width;
    e->expand_form = expand_form_word(2, n, false, false, false, 1, 0, false, grid.x);
#define PW_X1(NP)                                                                                         \
  do {                                                                                                    \
    if (per_pass == 4) hipLaunchKernelGGL((pw_expand4_lane_kernel<NP, true>), grid, wave, lds, st, a, vec_out, per_pass);  \
    else hipLaunchKernelGGL((pw_expand4_lane_kernel<NP, false>), grid, wave, lds, st, a, vec_out, per_pass);                \
  } while (0)
    if (n <= 4) PW_X1(4);
    else if (n <= 8) PW_X1(8);
    else if (n <= 16) PW_X1(16);
    else PW_X1(32);
#undef PW_X1
    prof.close();
    return check_launch("pw_expand4");
  }
  e->expand_form = expand_form_word(1, n, false, false, false, 4, 0, false, (n <= 8 || (n <= 16 && !e->step_wide_groups)) ? g8.x : (n <= 16 ? g16.x : g32.x));
  if (n <= 8) {
    if (tab) hipLaunchKernelGGL((pw_expand4_kernel<8, true>), g8, block, 0, st, a);
    else hipLaunchKernelGGL((pw_expand4_kernel<8, false>), g8, block, 0, st, a);
  } else if (n <= 16 && !e->step_wide_groups) {  // two movables per lane: 8 states per wavefront
    if (tab) hipLaunchKernelGGL((pw_expand4_kernel<8, true, true>), g8, block, 0, st, a);
    else hipLaunchKernelGGL((pw_expand4_kernel<8, false, true>), g8, block, 0, st, a);
  } else if (n <= 16) {
    if (tab) hipLaunchKernelGGL((pw_expand4_kernel<16, true>), g16, block, 0, st, a);
    else hipLaunchKernelGGL((pw_expand4_kernel<16, false>), g16, block, 0, st, a);
  } else {
    if (tab) hipLaunchKernelGGL((pw_expand4_kernel<32, true>), g32, block, 0, st, a);
    else hipLaunchKernelGGL((pw_expand4_kernel<32, false>), g32, block, 0, st, a);
  }
  prof.close();
  return check_launch("pw_expand4");
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

}  // extern "C"

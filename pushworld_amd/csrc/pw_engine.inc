// pw_engine.inc -- engine half of the C ABI (include/pushworld_amd.h), first file: fill_render_args, the release helpers, the
// table builders (overlap, push and segment tables) and their uploads, pw_engine_create / _destroy and the small queries.
// Part of the single translation unit pw_kernels.hip, after the kernel files and pw_hostlib.inc.  The launches and the other
// entry points follow by family: pw_engine_render.inc, _step.inc, _step_render.inc, _expand.inc, _obs.inc, _plan.inc and
// _options.inc.

// ------------------------------------------------------------------------------------
// engine half of the C ABI
// ------------------------------------------------------------------------------------
namespace {

// zero fill of a library-owned observation buffer (whole 16-byte words)
__global__ __launch_bounds__(256) void pw_zero_kernel(uint4* p, size_t n) {
  for (size_t i = blockIdx.x * static_cast<size_t>(256) + threadIdx.x; i < n; i += static_cast<size_t>(gridDim.x) * 256)
    p[i] = make_uint4(0u, 0u, 0u, 0u);
}

const uint8_t kPaletteRGB[PW_NUM_COLORS][3] = {
    {0, 0, 0},           // PW_C_PAD
    {255, 255, 255},     // PW_C_BACKGROUND      puzzle.py:451
    {0xFA, 0xC7, 0x1E},  // AGENT_WALL           puzzle.py:70
    {0x7D, 0x64, 0x0F},  // AGENT_WALL_BORDER    :71
    {0x0A, 0x0A, 0x0A},  // WALL                 :78
    {0x05, 0x05, 0x05},  // WALL_BORDER          :79
    {0x00, 0xDC, 0x00},  // AGENT                :68
    {0x00, 0x6E, 0x00},  // AGENT_BORDER         :69
    {0xDC, 0x00, 0x00},  // GOAL_OBJECT          :74
    {0x6E, 0x00, 0x00},  // GOAL_OBJECT_BORDER   :75
    {0x46, 0x9B, 0xFF},  // MOVABLE              :76
    {0x23, 0x48, 0x7F},  // MOVABLE_BORDER       :77
    {0xB9, 0x00, 0x00},  // GOAL_BORDER          :73
};

int fill_render_args(const PwEngine* e, const int32_t* puzzle_id, const int8_t* pos, void* obs, int64_t stride,
                     int32_t batch, RenderArgs* ra) {
  if (!puzzle_id || !pos || !obs) return pw_fail(PW_EINVAL, "null device pointer");
  if (stride < e->obs_bytes || (stride & 15)) return pw_fail(PW_EINVAL, "env_stride_bytes must be >= obs bytes rounded up to 16 and a multiple of 16");
  if (stride < ((e->obs_bytes + 15) & ~int64_t(15))) return pw_fail(PW_EINVAL, "env_stride_bytes too small");
  if (reinterpret_cast<uintptr_t>(obs) & 15) return pw_fail(PW_EINVAL, "obs must be 16-byte aligned");
  ra->hdrs = e->set->d_headers;
  ra->blob = e->set->d_blob;
  ra->puzzle_id = puzzle_id;
  ra->pos = pos;
  ra->obs = static_cast<uint8_t*>(obs);
  ra->env_stride = stride;
  ra->batch = batch;
  ra->np = e->np;
  ra->ppc = e->cfg.pixels_per_cell;
  ra->bw = e->cfg.border_width;
  ra->pad_h = e->pad_h;
  ra->pad_w = e->pad_w;
  ra->estat = e->d_estat;
  ra->estat_off = e->d_estat_off;
  ra->obs_bytes = static_cast<int32_t>(e->obs_bytes);
  ra->num_puzzles = e->set->count;
  ra->do_step = 0;
  ra->skip_movables = 0;
  ra->dirty_rows = nullptr;
  ra->bands = 1;
  ra->signal = nullptr;
  ra->signal_seq = 0ull;
  ra->signal_count = nullptr;
  for (int i = 0; i < 16; i++) {
    ra->pal_rgb[i] = e->pal_rgb[i];
    for (int c = 0; c < 4; c++) ra->pal_f32[i][c] = e->pal_f32[i][c];
  }
  return PW_OK;
}

void release_obs_buf(PwObsBuf& b) {
  // Unmap chunk by chunk (the way they were mapped), release the physical chunks, free the address range: on this
  // runtime the memory only returns to the DEVICE once the range is freed too (profiles/r03_vmm_cycle.txt: without
  // hipMemAddressFree hipMemGetInfo keeps counting released chunks as used).
  for (size_t i = 0; b.ptr && i * b.chunk < b.bytes; i++) (void)hipMemUnmap(static_cast<char*>(b.ptr) + i * b.chunk, b.chunk);
  for (hipMemGenericAllocationHandle_t h : b.handles) (void)hipMemRelease(h);
  if (b.ptr && b.reserved) (void)hipMemAddressFree(b.ptr, b.reserved);
  b.reserved = 0;
  b.handles.clear();
  b.ptr = nullptr;
  b.bytes = 0;
}


// drops the engine's binding (pw_batch_bind); the device is idle or the caller has synchronised
void release_bind(PwEngine* e) {
  if (!e->bind) return;
  if (e->bind->d_ints) (void)hipFree(e->bind->d_ints);
  if (e->bind->d_bound) (void)hipFree(e->bind->d_bound);
  if (e->bind->d_segs) (void)hipFree(e->bind->d_segs);
  delete e->bind;
  e->bind = nullptr;
}

// Overlap tables (PwOvlDir) of the puzzles `mode` selects (PW_OPT_STEP_TABLES), from the host copy of the packed set.
// words[0] is unused (offset 0 = "no tables").  Budget: 256 MB; puzzles beyond it (and grids wider than 62 cells,
// movables wider than 32) keep the row loops.
void build_overlap_tables(const PwPuzzleSet* s, int mode, std::vector<uint64_t>& words, std::vector<PwOvlDir>& dir,
                          int* n_puzzles) {
  words.assign(1, 0ull);
  dir.assign(static_cast<size_t>(s->count), PwOvlDir{0u, 0u, 0, 0, 0u});
  *n_puzzles = 0;
  if (mode == 2) return;
  auto has_big = [&](const PwPuzzleHeader& h) {
    const uint64_t* small = reinterpret_cast<const uint64_t*>(s->blob.data() + h.base + h.off_small);
    for (int j = 0; j < h.N; j++)
      if (small[j] == 0ull) return true;
    return false;
  };
  if (mode == 0) mode = 1;  // automatic = every puzzle: the table-only kernels are the faster ones also for sets of small
                            // movables (one or two loads instead of the wall-row loops, fewer registers;
                            // profiles/r03_step_tables.txt), and the tables of all 14 223 benchmark puzzles are 7 MB
  const size_t budget_words = (size_t(256) << 20) / 8;
  for (int p = 0; p < s->count; p++) {
    const PwPuzzleHeader& h = s->headers[p];
    const uint8_t* b = s->blob.data() + h.base;
    const uint64_t* wall = reinterpret_cast<const uint64_t*>(b + h.off_wall);
    const uint64_t* awall = reinterpret_cast<const uint64_t*>(b + h.off_awall);
    const uint64_t* shapes = reinterpret_cast<const uint64_t*>(b + h.off_shapes);
    const int N = h.N, W = h.W, H = h.H;
    if (N < 1 || W > 62) continue;  // wall-table bit x + 1 of x = W - w + 1 must stay below 64
    int w1 = 0, h1 = 0;  // the largest width / height
    for (int j = 0; j < N; j++) {
      w1 = std::max<int>(w1, h.objtab[j].w);
      h1 = std::max<int>(h1, h.objtab[j].h);
    }
    if (mode == 3 && !has_big(h)) continue;
    if (2 * w1 - 1 > 64) continue;  // a pair-table row is one uint64
    const int R = 2 * h1 - 1, Hs = H + 2;
    const size_t need = static_cast<size_t>(N) * N * R + static_cast<size_t>(N) * Hs;
    if (words.size() + need > budget_words) continue;
    PwOvlDir d;
    d.pair_off = static_cast<uint32_t>(words.size());
    d.wall_off = static_cast<uint32_t>(words.size() + static_cast<size_t>(N) * N * R);
    d.R = static_cast<uint16_t>(R);
    d.Hs = static_cast<uint16_t>(Hs);
    d.reserved = 0u;
    words.resize(words.size() + need, 0ull);
    uint64_t* pair = words.data() + d.pair_off;
    uint64_t* wt = words.data() + d.wall_off;
    for (int i = 0; i < N; i++) {
      const PwObjEntry oi = h.objtab[i];
      for (int j = 0; j < N; j++) {
        const PwObjEntry oj = h.objtab[j];
        uint64_t* t = pair + (static_cast<size_t>(i) * N + j) * R;
        // i at (rx, ry) in the frame of j: rows yj of j meet rows yi = yj - ry of i
        for (int ry = -(oi.h - 1); ry <= oj.h - 1; ry++) {
          uint64_t bits = 0;
          for (int rx = -(oi.w - 1); rx <= oj.w - 1; rx++) {
            bool ov = false;
            for (int yj = std::max(0, ry); yj < std::min<int>(oj.h, ry + oi.h) && !ov; yj++) {
              const uint64_t si = shapes[oi.row_off + (yj - ry)], sj = shapes[oj.row_off + yj];
              ov = ((rx >= 0 ? si << rx : si >> -rx) & sj) != 0ull;
            }
            if (ov) bits |= 1ull << (rx + oi.w - 1);
          }
          t[ry + oi.h - 1] = bits;
        }
      }
    }
    for (int j = 0; j < N; j++) {
      const PwObjEntry oj = h.objtab[j];
      const uint64_t* rows = j == 0 ? awall : wall;  // the agent also stops at agent walls (puzzle.py:272-281)
      uint64_t* t = wt + static_cast<size_t>(j) * Hs;
      for (int y = -1; y <= H - oj.h + 1; y++) {
        uint64_t bits = 0;
        for (int x = -1; x <= W - oj.w + 1; x++) {
          // a position that is not entirely inside the grid counts as "overlapping a wall now": a movable there is never
          // stopped by a wall (the bounds clause, puzzle.py:557-561 -- the reference's tables hold in-bounds positions only),
          // whatever gaps its shape has where the border wall is.  (An object entering such a position comes from the edge
          // of the grid, where its tight bounding box overlaps the border wall already: no new verdict for positions inside.)
          bool ov = x < 0 || y < 0 || x + oj.w > W || y + oj.h > H;
          for (int r = 0; r < oj.h && !ov; r++) {
            const int yy = y + r;
            if (yy < 0 || yy >= H) continue;
            const uint64_t so = shapes[oj.row_off + r];
            ov = ((x >= 0 ? so << x : so >> -x) & rows[yy]) != 0ull;
          }
          if (ov) bits |= 1ull << (x + 1);
        }
        t[y + 1] = bits;
      }
    }
    dir[static_cast<size_t>(p)] = d;
    *n_puzzles += 1;
  }
}

// Push tables (PwPushDir) of the puzzles that have overlap tables, appended to `words`: nibble a of an offset = the overlap
// table says "overlap at offset + displacement(a) and none at the offset" (puzzle.py:522-593).
constexpr size_t kPushLdsBytes = 112 * 1024;  // tables of a puzzle that pw_expand4_v2_kernel may keep in LDS (160 KB per CU)
constexpr int kPairDimsMaxN = 20;  // ... with a 128-bit work word from 17 movables on (instances up to 20: `Clean Sweep` has 19)
constexpr size_t kPairDimsFrom = 16 * 1024;  // uniform byte pair tables beyond this: the per-pair form too (pw_expand4_v2_kernel<., ., ., true>)
constexpr int kPushTablePuzzles = 64;  // the planner's engines hold one puzzle; pools of thousands do not need these
void build_push_tables(const PwPuzzleSet* s, std::vector<uint64_t>& words, const std::vector<PwOvlDir>& dir,
                       std::vector<PwPushDir>& push) {
  push.assign(dir.size(), PwPushDir{0u, 0u, 0, 0, 0, 0, 0u, 0, 0, 0u, 0u, 0u, 0u});
  if (s->count > kPushTablePuzzles) return;
  static const int DX[4] = {-1, 1, 0, 0}, DY[4] = {0, 0, -1, 1};
  for (int p = 0; p < s->count; p++) {
    const PwOvlDir d = dir[static_cast<size_t>(p)];
    if (d.pair_off == 0u) continue;
    const PwPuzzleHeader& h = s->headers[p];
    const int N = h.N, W = h.W, R = d.R, Hs = d.Hs;
    int w1 = 0, h1 = 0;
    for (int j = 0; j < N; j++) {
      w1 = std::max<int>(w1, h.objtab[j].w);
      h1 = std::max<int>(h1, h.objtab[j].h);
    }
    const int R2 = 2 * h1 + 1, RW = (2 * w1 + 1 + 7) / 8, WW = (W + 2 + 7) / 8;
    const size_t pair_words32 = static_cast<size_t>(N) * N * R2 * RW, wall_words32 = static_cast<size_t>(N) * Hs * WW;
    const size_t start = words.size();
    words.resize(start + (pair_words32 + 1) / 2 + (wall_words32 + 1) / 2, 0ull);
    PwPushDir q;
    q.pair_off = static_cast<uint32_t>(start);
    q.wall_off = static_cast<uint32_t>(start + (pair_words32 + 1) / 2);
    q.R2 = static_cast<uint16_t>(R2);
    q.RW = static_cast<uint16_t>(RW);
    q.Hs = static_cast<uint16_t>(Hs);
    q.WW = static_cast<uint16_t>(WW);
    std::vector<uint32_t> pw(pair_words32, 0u), ww(wall_words32, 0u);
    const uint64_t* ovl_pair = words.data() + d.pair_off;
    const uint64_t* ovl_wall = words.data() + d.wall_off;
    auto bit_at = [](const uint64_t* t, int row, int bit, int rows) {
      return row >= 0 && row < rows && bit >= 0 && bit < 64 && ((t[row] >> bit) & 1ull) != 0ull;
    };
    for (int i = 0; i < N; i++) {
      const PwObjEntry oi = h.objtab[i];
      for (int j = 0; j < N; j++) {
        const PwObjEntry oj = h.objtab[j];
        const uint64_t* o = ovl_pair + (static_cast<size_t>(i) * N + j) * R;
        uint32_t* t = pw.data() + (static_cast<size_t>(i) * N + j) * R2 * RW;
        for (int ry = -oi.h; ry <= oj.h; ry++)
          for (int rx = -oi.w; rx <= oj.w; rx++) {
            if (bit_at(o, ry + oi.h - 1, rx + oi.w - 1, R)) continue;  // they overlap already: nobody pushes
            uint32_t nib = 0;
            for (int a = 0; a < 4; a++)
              if (bit_at(o, ry + DY[a] + oi.h - 1, rx + DX[a] + oi.w - 1, R)) nib |= 1u << a;
            const int row = ry + oi.h, col = rx + oi.w;
            t[row * RW + (col >> 3)] |= nib << (4 * (col & 7));
          }
      }
    }
    for (int j = 0; j < N; j++) {
      const uint64_t* o = ovl_wall + static_cast<size_t>(j) * Hs;
      uint32_t* t = ww.data() + static_cast<size_t>(j) * Hs * WW;
      for (int row = 0; row < Hs; row++)
        for (int col = 0; col < W + 2 && col < 64; col++) {
          if (bit_at(o, row, col, Hs)) continue;
          uint32_t nib = 0;
          for (int a = 0; a < 4; a++)
            if (bit_at(o, row + DY[a], col + DX[a], Hs)) nib |= 1u << a;
          t[row * WW + (col >> 3)] |= nib << (4 * (col & 7));
        }
    }
    // byte form of the pair tables for the LDS-resident kernel (pw_expand4_v2_kernel): guard row R2 and guard column
    // 2 w1 + 1 are zero; only for tables that fit LDS next to the wall tables (kPushLdsBytes in all)
    q.pairb_off = 0u;
    q.CWB = static_cast<uint16_t>(2 * w1 + 2);
    q.reserved = 0;
    q.reserved2 = 0u;
    const size_t pairb = (static_cast<size_t>(N) * N * (R2 + 1) * q.CWB + 15) & ~size_t(15);
    q.pairb_bytes = static_cast<uint32_t>(pairb);
    if (N <= 16 && pairb + wall_words32 * 4 + 256 <= kPushLdsBytes) {
      std::vector<uint8_t> pb(pairb, 0);
      for (int t = 0; t < N * N; t++)
        for (int row = 0; row < R2; row++)
          for (int col = 0; col <= 2 * w1; col++)
            pb[(static_cast<size_t>(t) * (R2 + 1) + row) * q.CWB + col] =
                static_cast<uint8_t>((pw[(static_cast<size_t>(t) * R2 + row) * RW + (col >> 3)] >> (4 * (col & 7))) & 15u);
      const size_t at = words.size();
      words.resize(at + pairb / 8, 0ull);
      memcpy(words.data() + at, pb.data(), pairb);
      q.pairb_off = static_cast<uint32_t>(at);
    }
    // the per-pair form (PwPushDir::pairp_off) where the uniform tables are beyond 16 KB (or beyond LDS altogether)
    q.pairp_off = 0u;
    q.pairp_bytes = 0u;
    if (N <= kPairDimsMaxN && (q.pairb_off == 0u || pairb > kPairDimsFrom)) {
      size_t total = static_cast<size_t>(N) * N * 4;
      for (int i = 0; i < N; i++)
        for (int j = 0; j < N; j++) total += static_cast<size_t>(h.objtab[i].h + h.objtab[j].h + 2) * (h.objtab[i].w + h.objtab[j].w + 2);
      total = (total + 15) & ~size_t(15);
      if (total <= 65536 && total + wall_words32 * 4 + 256 <= kPushLdsBytes) {
        std::vector<uint8_t> pp(total, 0);
        uint32_t* desc = reinterpret_cast<uint32_t*>(pp.data());
        size_t at_b = static_cast<size_t>(N) * N * 4;
        for (int i = 0; i < N; i++)
          for (int j = 0; j < N; j++) {
            const int rows = h.objtab[i].h + h.objtab[j].h + 1, cols = h.objtab[i].w + h.objtab[j].w + 2;  // + the guard row
            const size_t t = static_cast<size_t>(i) * N + j;
            desc[t] = static_cast<uint32_t>(at_b) | (static_cast<uint32_t>(cols) << 16) | (static_cast<uint32_t>(rows) << 24);
            for (int row = 0; row < rows; row++)
              for (int col = 0; col < cols - 1; col++)
                pp[at_b + static_cast<size_t>(row) * cols + col] =
                    static_cast<uint8_t>((pw[(t * R2 + row) * RW + (col >> 3)] >> (4 * (col & 7))) & 15u);
            at_b += static_cast<size_t>(rows + 1) * cols;
          }
        const size_t at = words.size();
        words.resize(at + total / 8, 0ull);
        memcpy(words.data() + at, pp.data(), total);
        q.pairp_off = static_cast<uint32_t>(at);
        q.pairp_bytes = static_cast<uint32_t>(total);
      }
    }
    memcpy(words.data() + q.pair_off, pw.data(), pw.size() * 4);
    memcpy(words.data() + q.wall_off, ww.data(), ww.size() * 4);
    push[static_cast<size_t>(p)] = q;
  }
}

// LDS blocks of the segment kernels (PwSegDir, pw_seg_kernels.inc) of the puzzles that have overlap tables, appended to
// `words`: per-pair push tables as bytes (the nibble of build_push_tables: bit a = "the overlap table says overlap at
// offset + displacement(a) and none at the offset", puzzle.py:522-593), sized per pair with a zero guard row and column, the
// wall bitmaps of the overlap tables, the object table.  Built for EVERY puzzle whose block fits PW_SEG_LDS_BYTES (all 14 000
// Level-0 puzzles at ~0.4 KB, 222 of the 223 Level 1-4 puzzles: median 3 KB, largest 15.2 KB; `Mind The Gap` needs 37 KB).
// Two blocks per puzzle, two halves of `seg` (2 x set size entries): [p] with the wall tables as stop nibbles (launches of several
// steps), [set size + p] with wall bitmaps -- a fifth of the bytes: what a launch of one step copies, and what fits a lane's slot of
// pw_step_mseg_kernel (PW_SEG_MULTI_BYTES: the Level-0 puzzles).
void build_seg_tables(const PwPuzzleSet* s, std::vector<uint64_t>& words, const std::vector<PwOvlDir>& dir,
                      std::vector<PwSegDir>& seg, int* n_puzzles) {
  seg.assign(2 * dir.size(), PwSegDir{});
  *n_puzzles = 0;
  static const int DX[4] = {-1, 1, 0, 0}, DY[4] = {0, 0, -1, 1};
  std::vector<uint8_t> blk;
  for (int fmt = 1; fmt >= 0; fmt--)
  for (int p = 0; p < s->count; p++) {
    const PwOvlDir d = dir[static_cast<size_t>(p)];
    if (d.pair_off == 0u) continue;
    const PwPuzzleHeader& h = s->headers[p];
    const int N = h.N, G = h.G, R = d.R, Hs = d.Hs;
    if (N < 1 || N > PW_MAX_OBJECTS) continue;
    const int NS = (N + 3) & ~3;                        // descriptor rows are padded to whole blocks of four pairs
    size_t total = static_cast<size_t>(N) * NS * 4;     // descriptors
    const size_t obj_off = total;
    total += static_cast<size_t>(NS) * 4;               // object table
    const size_t goal_off = total;
    total += static_cast<size_t>(NS) * 2;               // goals
    total = (total + 3) & ~size_t(3);
    const size_t init_off = total;
    total += static_cast<size_t>(NS / 2) * 4;           // initial positions
    total = (total + 7) & ~size_t(7);
    const size_t wall_off = total;
    // bytes per wall row: bitmaps (bit x + 1 of row y + 1, x <= W - w + 1) or stop nibbles (W + 4 of them)
    const int wcols = h.W + 4, wstride = fmt == 1 ? (wcols + 1) / 2 : (h.W + 2 <= 16 ? 2 : 8);
    const size_t wper = static_cast<size_t>(fmt == 1 ? Hs + 2 : Hs) * wstride;
    total += static_cast<size_t>(N) * wper;             // wall tables
    const size_t zero_off = total;                      // the one-byte zero table of the pairs nobody looks up
    total += 1;
    const size_t pair_start = total;
    for (int i = 0; i < N; i++)
      for (int j = 1; j < N; j++)
        if (i != j) total += static_cast<size_t>(h.objtab[i].h + h.objtab[j].h + 2) * (h.objtab[i].w + h.objtab[j].w + 2);
    total = (total + 15) & ~size_t(15);
    if (total > PW_SEG_LDS_BYTES || wper > 65535u || wcols > 255) continue;
    if (fmt == 0 && seg[static_cast<size_t>(p)].off == 0u) continue;  // (both forms or none)
    bool fits = true;  // (the descriptor's fields: 8 bits of columns, 8 bits of guard row index)
    for (int i = 0; i < N && fits; i++)
      for (int j = 1; j < N; j++)
        if (i != j && (h.objtab[i].w + h.objtab[j].w + 2 > 255 || h.objtab[i].h + h.objtab[j].h + 1 > 255)) fits = false;
    if (!fits) continue;
    blk.assign(total, 0);
    uint32_t* desc = reinterpret_cast<uint32_t*>(blk.data());
    memcpy(blk.data() + obj_off, h.objtab, static_cast<size_t>(N) * 4);
    uint16_t* goal = reinterpret_cast<uint16_t*>(blk.data() + goal_off);
    int init_goals = 0;
    for (int j = 0; j < NS; j++) {
      goal[j] = 0x8080;  // (x = y = -128: no position has it)
      if (j >= 1 && j <= G) {
        memcpy(&goal[j], h.goal[j - 1], 2);
        init_goals += memcmp(h.goal[j - 1], h.init[j], 2) == 0;
      }
    }
    memcpy(blk.data() + init_off, h.init, static_cast<size_t>(N) * 2);
    auto bit_at = [](const uint64_t* t, int row, int bit, int rows) {
      return row >= 0 && row < rows && bit >= 0 && bit < 64 && ((t[row] >> bit) & 1ull) != 0ull;
    };
    for (int j = 0; j < N; j++) {
      const uint64_t* wj = words.data() + d.wall_off + static_cast<size_t>(j) * Hs;
      if (fmt == 0) {
        for (int row = 0; row < Hs; row++)  // (little endian: the low bytes of the overlap table's row)
          memcpy(blk.data() + wall_off + (static_cast<size_t>(j) * Hs + row) * wstride, wj + row, static_cast<size_t>(wstride));
        continue;
      }
      for (int r2 = 0; r2 < Hs + 2; r2++)
        for (int c2 = 0; c2 < wcols; c2++) {
          const int row = r2 - 1, bit = c2 - 1;  // (bitmap coordinates of the position)
          if (bit_at(wj, row, bit, Hs)) continue;  // it overlaps a wall now: no move is stopped by that (puzzle.py:522-564)
          uint8_t nib = 0;
          for (int a = 0; a < 4; a++)
            if (bit_at(wj, row + DY[a], bit + DX[a], Hs)) nib |= static_cast<uint8_t>(1u << a);
          blk[wall_off + static_cast<size_t>(j) * wper + static_cast<size_t>(r2) * wstride + (c2 >> 1)] |= static_cast<uint8_t>(nib << (4 * (c2 & 1)));
        }
    }
    size_t at = pair_start;
    for (int i = 0; i < N; i++) {
      const PwObjEntry oi = h.objtab[i];
      for (int j = 0; j < NS; j++) {
        const size_t t = static_cast<size_t>(i) * NS + j;
        if (j == 0 || i == j || j >= N) {  // the agent is never pushed (puzzle.py:364), nobody pushes itself; padding
          desc[t] = static_cast<uint32_t>(zero_off) | (0u << 16) | (0u << 24);
          continue;
        }
        const PwObjEntry oj = h.objtab[j];
        const int rows = oi.h + oj.h + 1, cols = oi.w + oj.w + 2;  // rows of data (the guard row has index `rows`), columns incl. the guard
        desc[t] = static_cast<uint32_t>(at) | (static_cast<uint32_t>(cols - 1) << 16) | (static_cast<uint32_t>(rows) << 24);  // (columns - 1 = index of the guard column)
        const uint64_t* o = words.data() + d.pair_off + (static_cast<size_t>(i) * N + j) * static_cast<size_t>(R);
        for (int ry = -oi.h; ry <= oj.h; ry++)
          for (int rx = -oi.w; rx <= oj.w; rx++) {
            if (bit_at(o, ry + oi.h - 1, rx + oi.w - 1, R)) continue;  // they overlap already: nobody pushes (puzzle.py:592)
            uint8_t nib = 0;
            for (int a = 0; a < 4; a++)
              if (bit_at(o, ry + DY[a] + oi.h - 1, rx + DX[a] + oi.w - 1, R)) nib |= static_cast<uint8_t>(1u << a);
            blk[at + static_cast<size_t>(ry + oi.h) * cols + (rx + oi.w)] = nib;
          }
        at += static_cast<size_t>(rows + 1) * cols;
      }
    }
    const size_t w0 = words.size();
    words.resize(w0 + total / 8, 0ull);
    memcpy(words.data() + w0, blk.data(), total);
    PwSegDir q{};
    q.off = static_cast<uint32_t>(w0);
    q.bytes = static_cast<uint32_t>(total);
    q.wall_off = static_cast<uint16_t>(wall_off);
    q.obj_off = static_cast<uint16_t>(obj_off);
    q.goal_off = static_cast<uint16_t>(goal_off);
    q.init_off = static_cast<uint16_t>(init_off);
    q.Hs = static_cast<uint16_t>(Hs);
    q.N = static_cast<uint8_t>(N);
    q.G = static_cast<uint8_t>(G);
    q.NS = static_cast<uint8_t>(NS);
    q.init_goals = static_cast<uint8_t>(init_goals);
    q.w0h0 = static_cast<uint16_t>(h.objtab[0].w | (h.objtab[0].h << 8));
    q.wall_stride = static_cast<uint8_t>(wstride);
    q.wall_fmt = static_cast<uint8_t>(fmt);
    q.wall_cols = static_cast<uint8_t>(wcols);
    q.wall_per = static_cast<uint16_t>(wper);
    seg[(fmt == 1 ? 0 : dir.size()) + static_cast<size_t>(p)] = q;
    if (fmt == 1) *n_puzzles += 1;
  }
}

// (re)builds the engine's overlap tables on its device (device guard held by the caller)
int upload_overlap_tables(PwEngine* e) {
  std::vector<uint64_t> words;
  std::vector<PwOvlDir> dir;
  int n = 0;
  std::vector<PwPushDir> push;
  build_overlap_tables(e->set, e->step_tables, words, dir, &n);
  build_push_tables(e->set, words, dir, push);
  std::vector<PwSegDir> seg;
  int n_seg = 0;
  build_seg_tables(e->set, words, dir, seg, &n_seg);
  (void)hipDeviceSynchronize();  // nothing in flight reads the old tables
  release_bind(e);               // (a binding holds offsets into them)
  if (e->d_ovl) (void)hipFree(e->d_ovl);
  if (e->d_ovl_dir) (void)hipFree(e->d_ovl_dir);
  if (e->d_push_dir) (void)hipFree(e->d_push_dir);
  if (e->d_seg_dir) (void)hipFree(e->d_seg_dir);
  e->d_ovl = nullptr;
  e->d_ovl_dir = nullptr;
  e->d_push_dir = nullptr;
  e->d_seg_dir = nullptr;
  e->seg_puzzles = 0;
  e->ovl_bytes = 0;
  e->ovl_puzzles = 0;
  e->ovl_has.assign(dir.size(), 0);
  e->push_has.assign(dir.size(), 0);
  e->push_host.clear();
  if (n == 0) return PW_OK;
  hipError_t err = hipMalloc(reinterpret_cast<void**>(&e->d_ovl), words.size() * 8);
  if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&e->d_ovl_dir), dir.size() * sizeof(PwOvlDir));
  if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&e->d_push_dir), push.size() * sizeof(PwPushDir));
  if (err == hipSuccess) err = hipMemcpy(e->d_ovl, words.data(), words.size() * 8, hipMemcpyHostToDevice);
  if (err == hipSuccess) err = hipMemcpy(e->d_ovl_dir, dir.data(), dir.size() * sizeof(PwOvlDir), hipMemcpyHostToDevice);
  if (err == hipSuccess) err = hipMemcpy(e->d_push_dir, push.data(), push.size() * sizeof(PwPushDir), hipMemcpyHostToDevice);
  if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&e->d_seg_dir), seg.size() * sizeof(PwSegDir));
  if (err == hipSuccess) err = hipMemcpy(e->d_seg_dir, seg.data(), seg.size() * sizeof(PwSegDir), hipMemcpyHostToDevice);
  if (err != hipSuccess) {
    if (e->d_ovl) (void)hipFree(e->d_ovl);
    if (e->d_ovl_dir) (void)hipFree(e->d_ovl_dir);
    if (e->d_push_dir) (void)hipFree(e->d_push_dir);
    if (e->d_seg_dir) (void)hipFree(e->d_seg_dir);
    e->d_ovl = nullptr;
    e->d_ovl_dir = nullptr;
    e->d_push_dir = nullptr;
    e->d_seg_dir = nullptr;
    e->ovl_has.assign(dir.size(), 0);
    return pw_fail(PW_EDEVICE, std::string("overlap tables: ") + hipGetErrorString(err));
  }
  e->ovl_bytes = static_cast<int64_t>(words.size() * 8);
  e->ovl_puzzles = n;
  e->seg_puzzles = n_seg;
  e->seg_max_bytes = 0;
  for (size_t p = 0; p < seg.size() / 2; p++) e->seg_max_bytes = std::max(e->seg_max_bytes, seg[p].bytes);  // (the segment kernels' half)
  for (size_t p = 0; p < dir.size(); p++) {
    e->ovl_has[p] = dir[p].pair_off != 0u;
    e->push_has[p] = push[p].pair_off != 0u;
  }
  e->push_host = push;
  return PW_OK;
}

// Sets whose puzzles ALL fit into 8 x 8 cells (with their border walls) and have at most 8 movables: the grid's walls as one
// uint64 per puzzle (bit 8 y + x), once without and once with the agent walls -- all pw_step_board_kernel needs besides the
// movables' own 8 x 8 shape boards (PwPuzzleHeader::off_small).
int upload_boards(PwEngine* e) {
  const PwPuzzleSet* s = e->set;
  std::vector<uint64_t> b(static_cast<size_t>(s->count) * 2, 0ull);
  for (int p = 0; p < s->count; p++) {
    const PwPuzzleHeader& h = s->headers[p];
    if (h.W > 8 || h.H > 8 || h.N > 8 || h.N < 1) return PW_OK;  // one puzzle that does not fit: no boards for the set
    const uint64_t* wall = reinterpret_cast<const uint64_t*>(s->blob.data() + h.base + h.off_wall);
    const uint64_t* awall = reinterpret_cast<const uint64_t*>(s->blob.data() + h.base + h.off_awall);
    for (int y = 0; y < h.H; y++) {
      b[2 * static_cast<size_t>(p)] |= (wall[y] & 0xffull) << (8 * y);
      b[2 * static_cast<size_t>(p) + 1] |= (awall[y] & 0xffull) << (8 * y);
    }
  }
  if (e->np > 8) return PW_OK;
  hipError_t err = hipMalloc(reinterpret_cast<void**>(&e->d_boards), b.size() * 8);
  if (err == hipSuccess) err = hipMemcpy(e->d_boards, b.data(), b.size() * 8, hipMemcpyHostToDevice);
  if (err != hipSuccess) {
    if (e->d_boards) (void)hipFree(e->d_boards);
    e->d_boards = nullptr;
    return pw_fail(PW_EDEVICE, std::string("grid boards: ") + hipGetErrorString(err));
  }
  return PW_OK;
}


// PwQuadDesc records of step_quad16_body (layout: PW_QD_* in pw_step_kernels.inc): one 576-byte record per puzzle whose grid
// fits 16 x 16 cells with at most 8 movables of at most 16 x 8 cells; the others get a record that only says so (N = 0; the
// real movable count in byte 4 serves the workgroups' choice of lanes per environment).
int upload_quad_desc(PwEngine* e) {
  const PwPuzzleSet* s = e->set;
  e->quad_puzzles = 0;
  if (e->ovl_puzzles == 0 || e->ovl_puzzles != s->count) return PW_OK;  // (its fallback for states outside the grid is the table form)
  std::vector<uint8_t> rec(static_cast<size_t>(s->count) * PW_QD_BYTES, 0);
  for (int p = 0; p < s->count; p++) {
    const PwPuzzleHeader& h = s->headers[p];
    uint8_t* d = rec.data() + static_cast<size_t>(p) * PW_QD_BYTES;
    d[0] = h.W;
    d[1] = h.H;
    d[3] = h.G;
    d[4] = h.N;
    bool fits = h.W <= 16 && h.H <= 16 && h.N >= 1 && h.N <= 8;
    for (int j = 0; fits && j < h.N; j++) fits = h.objtab[j].w <= 16 && h.objtab[j].h <= 8 && h.objtab[j].w <= h.W && h.objtab[j].h <= h.H;
    if (!fits) continue;
    d[2] = h.N;
    const uint8_t* blob = s->blob.data() + h.base;
    const uint64_t* wall = reinterpret_cast<const uint64_t*>(blob + h.off_wall);
    const uint64_t* awall = reinterpret_cast<const uint64_t*>(blob + h.off_awall);
    const uint64_t* shapes = reinterpret_cast<const uint64_t*>(blob + h.off_shapes);
    for (int j = 0; j < 8; j++) {
      d[PW_QD_LIM + 2 * j] = j < h.N ? static_cast<uint8_t>(h.W - h.objtab[j].w) : 0x7f;
      d[PW_QD_LIM + 2 * j + 1] = j < h.N ? static_cast<uint8_t>(h.H - h.objtab[j].h) : 0x7f;
      d[PW_QD_GOAL + 2 * j] = (j >= 1 && j <= h.G) ? static_cast<uint8_t>(h.goal[j - 1][0]) : 0x80;
      d[PW_QD_GOAL + 2 * j + 1] = (j >= 1 && j <= h.G) ? static_cast<uint8_t>(h.goal[j - 1][1]) : 0x80;
      d[PW_QD_INIT + 2 * j] = j < h.N ? static_cast<uint8_t>(h.init[j][0]) : 0;
      d[PW_QD_INIT + 2 * j + 1] = j < h.N ? static_cast<uint8_t>(h.init[j][1]) : 0;
      if (j < h.N) {
        uint16_t* rows = reinterpret_cast<uint16_t*>(d + PW_QD_SHAPE + PW_QD_SHAPE_STRIDE * j);
        for (int r = 0; r < h.objtab[j].h; r++) rows[r] = static_cast<uint16_t>(shapes[h.objtab[j].row_off + r] & 0xffffull);
      }
    }
    uint32_t* qw = reinterpret_cast<uint32_t*>(d + PW_QD_WALL);
    uint32_t* qa = reinterpret_cast<uint32_t*>(d + PW_QD_AWALL);
    for (int y = 0; y < h.H; y++) {
      qw[y >> 1] |= static_cast<uint32_t>(wall[y] & 0xffffull) << (16 * (y & 1));
      qa[y >> 1] |= static_cast<uint32_t>(awall[y] & 0xffffull) << (16 * (y & 1));
    }
    e->quad_puzzles++;
  }
  if (e->quad_puzzles == 0) return PW_OK;
  hipError_t err = hipMalloc(reinterpret_cast<void**>(&e->d_qdesc), rec.size());
  if (err == hipSuccess) err = hipMemcpy(e->d_qdesc, rec.data(), rec.size(), hipMemcpyHostToDevice);
  if (err != hipSuccess) {
    if (e->d_qdesc) (void)hipFree(e->d_qdesc);
    e->d_qdesc = nullptr;
    return pw_fail(PW_EDEVICE, std::string("16 x 16 board records: ") + hipGetErrorString(err));
  }
  return PW_OK;
}

}  // namespace

extern "C" {

int64_t pw_puzzleset_overlap_tables(const PwPuzzleSet* s, int mode, uint64_t* words, int64_t cap_words, uint32_t* dir) try {
  if (!s) return pw_fail(PW_EINVAL, "null puzzle set");
  if (mode < 0 || mode > 3) return pw_fail(PW_EINVAL, "mode: 0 automatic, 1 every puzzle, 2 none, 3 puzzles with big movables");
  std::vector<uint64_t> w;
  std::vector<PwOvlDir> d;
  int n = 0;
  build_overlap_tables(s, mode, w, d, &n);
  if (words && cap_words >= static_cast<int64_t>(w.size())) memcpy(words, w.data(), w.size() * 8);
  if (dir) memcpy(dir, d.data(), d.size() * sizeof(PwOvlDir));
  return static_cast<int64_t>(w.size());
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_engine_create(const PwPuzzleSet* s, const PwEngineConfig* cfg, PwEngine** out) try {
  if (!s || !cfg || !out) return pw_fail(PW_EINVAL, "null argument");
  if (s->device < 0 || !s->d_blob) return pw_fail(PW_EDEVICE, "puzzle set has no device tables (created with device < 0)");
  if (cfg->border_width < 1) return pw_fail(PW_EINVAL, "border_width must be >= 1");
  if (cfg->pixels_per_cell < 3) return pw_fail(PW_EINVAL, "pixels_per_cell must be >= 3");
  if (cfg->pixels_per_cell < 1 + 2 * cfg->border_width)
    return pw_fail(PW_EINVAL, "pixels_per_cell must be >= 1 + 2*border_width");
  if (cfg->obs_dtype != PW_OBS_U8 && cfg->obs_dtype != PW_OBS_F32) return pw_fail(PW_EINVAL, "bad obs_dtype");
  if (cfg->max_batch < 0) return pw_fail(PW_EINVAL, "max_batch must be >= 0 (0 = scratch grows on demand)");
  // owner: whatever throws below (the host vectors of the static tables), the engine and its device memory are released
  struct EngineOwner {
    PwEngine* e;
    ~EngineOwner() { if (e) pw_engine_destroy(e); }
  } owner{new (std::nothrow) PwEngine()};  // (value-initialised: every pointer starts out null)
  PwEngine* e = owner.e;
  if (!e) return pw_fail(PW_ENOMEM, "out of memory");
  e->set = s;
  e->cfg = *cfg;
  e->np = s->max_n <= 4 ? 4 : (s->max_n <= 8 ? 8 : (s->max_n <= 16 ? 16 : 32));
  e->pad_h = cfg->pad_cell_height > 0 ? cfg->pad_cell_height : s->max_h;
  e->pad_w = cfg->pad_cell_width > 0 ? cfg->pad_cell_width : s->max_w;
  if (e->pad_h < s->max_h || e->pad_w < s->max_w)
    return pw_fail(PW_EINVAL, "observation frame is smaller than the largest puzzle in the set");
  e->obs_h = e->pad_h * cfg->pixels_per_cell;
  e->obs_w = e->pad_w * cfg->pixels_per_cell;
  e->obs_bytes = static_cast<int64_t>(e->obs_h) * e->obs_w * 3 * (cfg->obs_dtype == PW_OBS_F32 ? 4 : 1);
  if (e->obs_bytes > (int64_t(1) << 30)) return pw_fail(PW_ELIMIT, "observation larger than 1 GiB");
  e->fast_u8_ppc3 = cfg->obs_dtype == PW_OBS_U8 && cfg->pixels_per_cell == 3 && cfg->border_width == 1;
  e->page_f32 = cfg->obs_dtype == PW_OBS_F32 && cfg->pixels_per_cell == 3 && cfg->border_width == 1;
  e->d_estat_page = nullptr;
  e->d_estat_page_off = nullptr;
  e->rowpage = false;
  e->rowpage_aligned = false;
  e->d_srow = nullptr;
  e->srow_stride = 0;
  e->srow_pitch = 0;
  e->row_bytes = e->obs_w * 3 * (cfg->obs_dtype == PW_OBS_F32 ? 4 : 1);
  e->d_estat = nullptr;
  e->d_estat_off = nullptr;
  e->d_scratch = nullptr;
  e->d_counters = nullptr;
  e->bad_total = 0;
  e->lat_stream = nullptr;
  e->lat_host = nullptr;
  e->lat_dev = nullptr;
  e->lat_bytes = 0;
  e->lat_seq = 0;
  e->mailbox = nullptr;
  e->step_signal = nullptr;
  e->step_signal_seq = 0ull;
  e->mailbox_seg = 0;
  e->mailbox_mode = 11;  // (pipelined; ONE wavefront reads the host's words: every further poller adds ~0.15 us to a round trip -- 64: 11.6 instead of 2.5 us)
  e->d_boards = nullptr;
  e->step_boards = 0;
  e->d_qdesc = nullptr;
  e->quad_puzzles = 0;
  e->step_quad16 = 0;
  e->step_kernel = 0;
  e->force_fused = false;
  e->step_one_fused = 1;
  e->step_one_seq = 0ull;
  e->step_host_copy = nullptr;
  e->force_lds_render = false;
  e->page_slice_envs = 0;
  e->search_chunk = 0;
  e->search_keys = 0;
  e->push_search_fp_bits = 0;
  e->resample_fence = 0;
  e->stats_lds_puzzles = 0;
  e->stats_groups = 0;
  e->expand_pair_dims = 0;
  e->step_lds_tables = 0;
  e->step_wide_groups = 0;
  e->step_narrow_groups = 0;
  e->step_reverse = 0;
  e->step_lane_batch = 0;
  e->expand_lds_tables = 0;
  e->expand_tile_order = 0;
  e->expand_prefetch = -1;
  e->expand_groups_per_cu = 0;
  e->search_batch_groups_per_cu = 0;
  e->expand_wg_waves = 0;
  e->expand_form = 0;
  e->step_mixed = 0;
  e->num_cus = 256;
  e->d_search_slab = nullptr;
  e->search_slab_bytes = 0;
  e->lds_tables_fit = true;  // the LDS copy of the group step kernel holds 128 shape rows per puzzle
  for (const PwPuzzleHeader& h : s->headers)
    if (((h.off_static - h.off_shapes) >> 3) > PW_LDS_SHAPE_ROWS) e->lds_tables_fit = false;
  // robust optimum over the allocations and boxes measured (profiles/r02_page_xp.txt): every XCD writes runs of
  // 64 consecutive pages, 13-14 workgroups per CU
  e->page_order = 2;
  e->page_run_log2 = 6;
  e->page_lds_pad_kb = cfg->obs_dtype == PW_OBS_F32 ? 8 : 7;
  e->page_load_all = 0;
  e->step_tables = 0;
  e->d_ovl = nullptr;
  e->d_ovl_dir = nullptr;
  e->d_push_dir = nullptr;
  e->d_seg_dir = nullptr;
  e->seg_puzzles = 0;
  e->seg_max_bytes = 0;
  e->side_stream = nullptr;
  e->ev_fork = nullptr;
  e->ev_join = nullptr;
  e->bind = nullptr;
  e->obs_tune_ms = 0;
  e->obs_screen_ms = 0;
  e->bind_min_envs = 0;
  e->bind_lanes = 0;
  e->bind_rollouts = 0;
  e->bind_max_kb = 0;
  e->bind_spread = 0;
  e->bind_fused = 0;
  e->d_bind_mismatch = nullptr;
  e->ovl_bytes = 0;
  e->ovl_puzzles = 0;
  e->obs_chunk_mb = 0;
  e->obs_accept_gbs = 7050;  // 0.88 of the 8 TB/s peak: what the tuned render reaches on allocations of the fast class
  e->tuning = false;
  e->tuned_ns = 0;
  e->d_rec = nullptr;
  e->rec_cap = 0;
  e->ret = PwRetained{};  // (option 0, nothing retained, no list)
  e->ret.form = 1;
  e->prof_used = 0;
  // Static zone-colour tables (walls, agent walls, background, goal outlines) of every puzzle in
  // the layout the render kernel of this engine streams from: row stride pad_w with the puzzle
  // shifted by c0 virtual columns for the 3-pixel fast path, row stride W otherwise.
  std::vector<uint16_t> estat, estat_page;
  std::vector<uint32_t> estat_off(s->count), estat_page_off(s->count);
  size_t max_e_bytes = 0;
  auto build_tables = [&](bool frame_layout, std::vector<uint16_t>& tab, std::vector<uint32_t>& off, size_t* max_bytes) {
    for (int p = 0; p < s->count; p++) {
      const PwPuzzleHeader& h = s->headers[p];
      const int W = h.W, H = h.H;
      const int estride = frame_layout ? e->pad_w : W;
      const int c0 = frame_layout ? ((e->pad_w - W) * 3 / 2 + 2) / 3 : 0;
      const uint32_t* codes = reinterpret_cast<const uint32_t*>(s->blob.data() + h.base + h.off_static);
      const size_t n_entries = static_cast<size_t>(3) * H * estride;
      const size_t e_bytes = ((2 * (n_entries + 3) + 15) >> 4) << 4;
      if (max_bytes) *max_bytes = std::max(*max_bytes, e_bytes);
      off[p] = static_cast<uint32_t>(tab.size() * 2);
      const size_t first = tab.size();
      tab.resize(first + e_bytes / 2, 0);
      for (int cy = 0; cy < H; cy++)
        for (int cx = 0; cx < W; cx++) {
          const uint32_t code = codes[cy * W + cx];
          const uint32_t kind = (code >> PW_CODE_KIND_SHIFT) & 0xfu;
          const uint32_t om = code & 0xffu, gm = code >> PW_CODE_GOAL_SHIFT;
          for (int zy = 0; zy < 3; zy++)
            tab[first + static_cast<size_t>(3 * cy + zy) * estride + cx + c0] =
                static_cast<uint16_t>(pw_zone_entry(kind, pw_zone_border_bits(om, zy), pw_zone_border_bits(gm, zy)));
        }
    }
  };
  build_tables(e->fast_u8_ppc3, estat, estat_off, &max_e_bytes);
  if (e->page_f32) build_tables(true, estat_page, estat_page_off, nullptr);
  e->render_lds = 16 + max_e_bytes + 64 + 64 + 16 + 256;  // guard, E, spos, pal, flag, float palette
  for (int i = 0; i < 16; i++) {
    e->pal_rgb[i] = 0;
    for (int c = 0; c < 4; c++) e->pal_f32[i][c] = 0.0f;
  }
  for (int i = 0; i < PW_NUM_COLORS; i++) {
    e->pal_rgb[i] = kPaletteRGB[i][0] | (kPaletteRGB[i][1] << 8) | (kPaletteRGB[i][2] << 16);
    for (int c = 0; c < 3; c++) {
      // env_utils.py:65-72: uint8.astype(float32) / 255 -- one correctly rounded binary32 division
      volatile float num = static_cast<float>(kPaletteRGB[i][c]);
      volatile float den = 255.0f;
      e->pal_f32[i][c] = num / den;
    }
  }
  PwDeviceGuard guard(s->device);  // the caller's current device is restored on return
  hipError_t err = guard.status();
  {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, s->device) == hipSuccess && cus > 0) e->num_cus = cus;
  }
  if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&e->d_estat), estat.size() * 2);
  if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&e->d_estat_off), estat_off.size() * 4);
  // 64 bytes of counters + one 4 KiB page of zeros (source of the padding pages of the every-page-loads render instance)
  if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&e->d_scratch), 4096 + 4096);
  if (err == hipSuccess) err = hipMemset(e->d_scratch, 0, 4096 + 4096);
  if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&e->d_counters), PW_COUNTER_SLOTS * 64);
  if (err == hipSuccess) err = hipMemset(e->d_counters, 0, PW_COUNTER_SLOTS * 64);
  if (err == hipSuccess) err = hipMemcpy(e->d_estat, estat.data(), estat.size() * 2, hipMemcpyHostToDevice);
  if (err == hipSuccess)
    err = hipMemcpy(e->d_estat_off, estat_off.data(), estat_off.size() * 4, hipMemcpyHostToDevice);
  if (e->page_f32) {
    if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&e->d_estat_page), estat_page.size() * 2);
    if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&e->d_estat_page_off), estat_page_off.size() * 4);
    if (err == hipSuccess)
      err = hipMemcpy(e->d_estat_page, estat_page.data(), estat_page.size() * 2, hipMemcpyHostToDevice);
    if (err == hipSuccess)
      err = hipMemcpy(e->d_estat_page_off, estat_page_off.data(), estat_page_off.size() * 4, hipMemcpyHostToDevice);
  }
  if (err == hipSuccess)
    err = hipFuncSetAttribute(reinterpret_cast<const void*>(pw_render_u8_ppc3_kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(e->render_lds));
  if (err == hipSuccess)
    err = hipFuncSetAttribute(reinterpret_cast<const void*>(pw_render_generic_kernel<uint8_t>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(e->render_lds));
  if (err == hipSuccess)
    err = hipFuncSetAttribute(reinterpret_cast<const void*>(pw_render_generic_kernel<float>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, static_cast<int>(e->render_lds));
  // Static row tables for the row-page kernel: every frame with pixel rows of at least 512 bytes that has no ppc-3
  // page kernel of its own, up to 2 GB of tables.
  if (err == hipSuccess && !e->fast_u8_ppc3 && !e->page_f32 && e->row_bytes >= 512 && e->obs_bytes >= 4096) {
    e->srow_pitch = ((e->row_bytes + 15) & ~15) + 16;
    e->srow_stride = 16 + static_cast<int64_t>(3 * s->max_h + 1) * e->srow_pitch;
    // whole-chunk rows take the cheaper index arithmetic (chunk -> pixel row is one 32-bit mulhi with a rounded-up
    // reciprocal: exact while chunks * chunks-per-row < 2^32)
    e->rowpage_aligned = e->row_bytes % 16 == 0 && (e->obs_bytes / 16) * (e->row_bytes / 16) < (int64_t(1) << 32);
    if (e->srow_stride * s->count <= (int64_t(2) << 30)) {
      const size_t bytes = static_cast<size_t>(e->srow_stride) * s->count;
      err = hipMalloc(reinterpret_cast<void**>(&e->d_srow), bytes);
      if (err == hipSuccess) err = hipMemset(e->d_srow, 0, bytes);
      if (err == hipSuccess) {
        StaticRowsArgs sa;
        sa.hdrs = s->d_headers;
        sa.estat = e->d_estat;
        sa.estat_off = e->d_estat_off;
        sa.out = e->d_srow;
        sa.stride = e->srow_stride;
        sa.pad_w = e->pad_w;
        sa.ppc = cfg->pixels_per_cell;
        sa.bw = cfg->border_width;
        sa.pitch = e->srow_pitch;
        for (int i = 0; i < 16; i++) {
          sa.pal_rgb[i] = e->pal_rgb[i];
          for (int c = 0; c < 4; c++) sa.pal_f32[i][c] = e->pal_f32[i][c];
        }
        const dim3 grid(static_cast<unsigned>(3 * s->max_h), static_cast<unsigned>(s->count));
        if (cfg->obs_dtype == PW_OBS_F32) hipLaunchKernelGGL(pw_static_rows_kernel<float>, grid, dim3(256), 0, nullptr, sa);
        else hipLaunchKernelGGL(pw_static_rows_kernel<uint8_t>, grid, dim3(256), 0, nullptr, sa);
        err = hipGetLastError();
        if (err == hipSuccess) err = hipDeviceSynchronize();
        e->rowpage = err == hipSuccess;
      }
    }
  }
  // static images of all puzzles for the page-ordered kernels, drawn once by the LDS kernel itself
  e->d_simg = nullptr;
  e->simg_stride = (e->obs_bytes + 255) & ~int64_t(255);
  e->d_dirty = nullptr;
  e->dirty_cap = 0;
  // Default for uint8 / ppc 3: the page-ordered kernel (static-image copy + LDS entry window), as long
  // as the static images of the whole puzzle set stay cache resident (64 MB; they are read once per
  // observation).  PW_OPT_RENDER_KERNEL = 1 forces the per-environment LDS kernel.
  // The delta kernel reads only the rows a step changed, so for it the images may live in HBM (<= 4 GB).
  const int64_t simg_total = static_cast<int64_t>(s->count) * e->simg_stride;
  // The page-ordered full render reads, per observation, the puzzle's own pixel rows of its static image (the frame
  // padding above and below is never loaded).  Those bytes should mostly come from L2 / the 256 MB MALL: up to
  // 512 MB of them in total (environments grouped by puzzle re-use an image while it is hot).
  int64_t simg_live = 0;
  for (int p = 0; p < s->count; p++)
    simg_live += static_cast<int64_t>(3) * s->headers[p].H * 9 * e->pad_w * (cfg->obs_dtype == PW_OBS_F32 ? 4 : 1);
  e->simg_cached = simg_live <= (int64_t(512) << 20);
  const bool want_page = (e->fast_u8_ppc3 || e->page_f32) && simg_total <= (int64_t(4) << 30);
  if (err == hipSuccess && want_page) {
    int32_t* d_ids = nullptr;
    int8_t* d_pos = nullptr;
    std::vector<int32_t> ids(s->count);
    for (int p = 0; p < s->count; p++) ids[p] = p;
    err = hipMalloc(reinterpret_cast<void**>(&e->d_simg), static_cast<size_t>(s->count) * e->simg_stride);
    if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&d_ids), ids.size() * 4);
    if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&d_pos), static_cast<size_t>(s->count) * e->np * 2);
    if (err == hipSuccess) err = hipMemcpy(d_ids, ids.data(), ids.size() * 4, hipMemcpyHostToDevice);
    if (err == hipSuccess) err = hipMemset(d_pos, 0, static_cast<size_t>(s->count) * e->np * 2);
    if (err == hipSuccess) {
      RenderArgs ra;
      uint8_t* simg = e->d_simg;
      e->d_simg = nullptr;  // fill_render_args / launch_render must take the LDS path here
      if (fill_render_args(e, d_ids, d_pos, simg, e->simg_stride, s->count, &ra) == PW_OK) {
        ra.skip_movables = 1;
        launch_render(e, ra, s->count, nullptr);
        err = hipGetLastError();
        if (err == hipSuccess) err = hipDeviceSynchronize();
      } else {
        err = hipErrorInvalidValue;
      }
      e->d_simg = simg;
    }
    if (d_ids) (void)hipFree(d_ids);
    if (d_pos) (void)hipFree(d_pos);
  }
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string("engine setup failed: ") + hipGetErrorString(err));
  if (cfg->max_batch > 0) {
    // per-environment scratch of the render entry points, sized once: no entry point allocates for batches up to max_batch
    const size_t nb = static_cast<size_t>(cfg->max_batch);
    if (hipMalloc(&e->d_rec, nb * sizeof(PageRec)) != hipSuccess) return pw_fail(PW_ENOMEM, "pw_engine_create: cannot allocate the page records of max_batch environments");
    e->rec_cap = cfg->max_batch;
    if (hipMalloc(reinterpret_cast<void**>(&e->d_dirty), nb * sizeof(uint32_t)) != hipSuccess) return pw_fail(PW_ENOMEM, "pw_engine_create: cannot allocate the dirty-row records of max_batch environments");
    e->dirty_cap = cfg->max_batch;
  }
  if (int rc = upload_overlap_tables(e)) return rc;  // overlap tables (PW_OPT_STEP_TABLES: every puzzle by default)
  if (int rc = upload_boards(e)) return rc;          // whole-grid boards of sets of 8 x 8 puzzles (pw_step_board_kernel)
  if (int rc = upload_quad_desc(e)) return rc;       // 16 x 16 board records (step_quad16_body)
  owner.e = nullptr;
  *out = e;
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

void pw_engine_destroy(PwEngine* e) {
  if (!e) return;
  if (e->mailbox) (void)pw_mailbox_close(e->mailbox);  // (stops the resident kernel; it reads this engine's tables)
  for (hipEvent_t ev : e->prof_events) (void)hipEventDestroy(ev);
  if (e->d_estat) (void)hipFree(e->d_estat);
  if (e->d_estat_off) (void)hipFree(e->d_estat_off);
  if (e->d_estat_page) (void)hipFree(e->d_estat_page);
  if (e->d_estat_page_off) (void)hipFree(e->d_estat_page_off);
  if (e->d_simg) (void)hipFree(e->d_simg);
  if (e->d_cells_base) (void)hipFree(e->d_cells_base);
  if (e->d_replay) (void)hipFree(e->d_replay);
  if (e->d_srow) (void)hipFree(e->d_srow);
  if (e->d_dirty) (void)hipFree(e->d_dirty);
  if (e->d_scratch) (void)hipFree(e->d_scratch);
  if (e->d_counters) (void)hipFree(e->d_counters);
  if (e->d_search_slab) (void)hipFree(e->d_search_slab);
  if (e->lat_stream) {
    (void)hipStreamSynchronize(e->lat_stream);
    (void)hipStreamDestroy(e->lat_stream);
  }
  if (e->lat_host) (void)hipHostFree(e->lat_host);
  if (e->d_boards) (void)hipFree(e->d_boards);
  if (e->d_qdesc) (void)hipFree(e->d_qdesc);
  if (e->d_rec) (void)hipFree(e->d_rec);
  if (e->ret.d_live) (void)hipFree(e->ret.d_live);
  if (e->ret.d_changed) (void)hipFree(e->ret.d_changed);  // (one allocation with d_shown)
  if (e->d_ovl) (void)hipFree(e->d_ovl);
  if (e->d_ovl_dir) (void)hipFree(e->d_ovl_dir);
  if (e->d_push_dir) (void)hipFree(e->d_push_dir);
  if (e->d_seg_dir) (void)hipFree(e->d_seg_dir);
  release_bind(e);
  if (e->side_stream) {
    (void)hipStreamSynchronize(e->side_stream);
    (void)hipStreamDestroy(e->side_stream);
  }
  if (e->ev_fork) (void)hipEventDestroy(e->ev_fork);
  if (e->ev_join) (void)hipEventDestroy(e->ev_join);
  if (!e->obs_bufs.empty()) {
    PwDeviceGuard guard(e->set->device);
    (void)hipDeviceSynchronize();
    for (PwObsBuf& b : e->obs_bufs) release_obs_buf(b);
  }
  delete e;
}

int pw_engine_npad(const PwEngine* e) try { return e ? e->np : pw_fail(PW_EINVAL, "null engine"); } catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_engine_obs_shape(const PwEngine* e, int* h, int* w, int* c) try {
  if (!e) return pw_fail(PW_EINVAL, "null engine");
  if (h) *h = e->obs_h;
  if (w) *w = e->obs_w;
  if (c) *c = 3;
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_engine_render_kernel(const PwEngine* e, char* buf, int cap) try {
  if (!e) return pw_fail(PW_EINVAL, "null engine");
  const char* name = "pw_render_generic_kernel";
  const bool page = e->d_simg && e->simg_cached && !e->force_lds_render;
  if (e->fast_u8_ppc3) name = page ? "pw_render_page_kernel" : "pw_render_u8_ppc3_kernel";
  else if (e->page_f32 && page) name = "pw_render_page_kernel";
  else if (e->rowpage && !e->force_lds_render) name = "pw_render_rowpage_kernel";
  const int n = static_cast<int>(strlen(name));
  if (buf && cap > 0) {
    const int m = n < cap - 1 ? n : cap - 1;
    memcpy(buf, name, m);
    buf[m] = 0;
  }
  return n;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int64_t pw_engine_obs_bytes(const PwEngine* e) try { return e ? e->obs_bytes : pw_fail(PW_EINVAL, "null engine"); } catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int64_t pw_engine_obs_stride(const PwEngine* e) try {
  if (!e) return pw_fail(PW_EINVAL, "null engine");
  // multiple of 512 B: 32 chunks of 16 B, so a 4 KiB page of the buffer starts on a word boundary of
  // an environment's dirty-chunk bitmap (overlay render path); 1 KiB / 4 KiB measured no faster
  return (e->obs_bytes + 511) & ~int64_t(511);
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

}  // extern "C"

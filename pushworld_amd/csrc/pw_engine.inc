// pw_engine.inc -- engine half of the C ABI (include/pushworld_amd.h): engine creation, launch logic,
// entry points.  Part of the single translation unit pw_kernels.hip.

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

static void rebind_async(PwEngine* e, const int32_t* puzzle_id, int32_t batch, hipStream_t st);
static bool live_build(PwEngine* e, const int32_t* puzzle_id, int32_t batch, hipStream_t st, bool may_alloc);

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
// list and of it the pages whose rows changed (PwRetained::d_changed, filled by the record writer of this call)
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
      ca.changed = live_form == 3 ? rt.d_changed : nullptr;
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
  launch_render(e, ra, batch, static_cast<hipStream_t>(stream), false, (live_form && track && e->ret.shown_valid) ? 3 : live_form,
                track);
  if (!live_form) retained_after_full_render(e, ra, batch);
  if (track) e->ret.shown_valid = true;  // (whichever form: the pre-pass left the new positions in `shown`)
  return check_launch("pw_render_retained");
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

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
    launch_render(e, ra, batch, st, rec_ready, (live_form && track && e->ret.shown_valid) ? 3 : live_form, track);
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

static int mailbox_form_of(const PwEngine* e);  // (pw_mailbox.inc: 0 no mailbox open, 1 one lane per environment / whole-grid boards, 2 segments)
int pw_engine_set_option(PwEngine* e, int32_t option, int64_t value) try {
  if (!e) return pw_fail(PW_EINVAL, "null engine");
  switch (option) {
    case PW_OPT_STEP_KERNEL:
      if (value < 0 || value > 2) return pw_fail(PW_EINVAL, "PW_OPT_STEP_KERNEL: 0 lane group, 1 wavefront, 2 lane");
      e->step_kernel = static_cast<int>(value);
      return PW_OK;
    case PW_OPT_FUSED_STEP_RENDER:
      e->force_fused = value != 0;
      e->ret.valid = e->ret.shown_valid = false;
      return PW_OK;
    case PW_OPT_RENDER_KERNEL:
      if (value < 0 || value > 1) return pw_fail(PW_EINVAL, "PW_OPT_RENDER_KERNEL: 0 automatic, 1 per-environment LDS kernel");
      e->force_lds_render = value != 0;
      e->ret.valid = e->ret.shown_valid = false;
      return PW_OK;
    case PW_OPT_PAGE_SLICE_ENVS:
      if (value < 0) return pw_fail(PW_EINVAL, "PW_OPT_PAGE_SLICE_ENVS must be >= 0");
      e->page_slice_envs = value;
      e->ret.valid = e->ret.shown_valid = false;
      return PW_OK;
    case PW_OPT_SEARCH_CHUNK:
      if (value < 0) return pw_fail(PW_EINVAL, "PW_OPT_SEARCH_CHUNK must be >= 0");
      e->search_chunk = value;
      return PW_OK;
    case PW_OPT_STEP_LDS_TABLES:
      if (value < 0 || value > 2) return pw_fail(PW_EINVAL, "PW_OPT_STEP_LDS_TABLES: 0 automatic, 1 always, 2 never");
      if (value == 1 && !e->lds_tables_fit)
        return pw_fail(PW_ELIMIT, "PW_OPT_STEP_LDS_TABLES: a puzzle of the set has more than 128 shape rows");
      e->step_lds_tables = static_cast<int>(value);
      return PW_OK;
    case PW_OPT_STEP_MIXED_GROUPS:
      if (value != 0 && value != 2) return pw_fail(PW_EINVAL, "PW_OPT_STEP_MIXED_GROUPS: 0 automatic, 2 never");
      e->step_mixed = static_cast<int>(value);
      return PW_OK;
    case PW_OPT_STEP_WIDE_GROUPS:
      if (value < 0 || value > 1) return pw_fail(PW_EINVAL, "PW_OPT_STEP_WIDE_GROUPS: 0 two movables per lane, 1 32-lane groups");
      e->step_wide_groups = static_cast<int>(value);
      return PW_OK;
    case PW_OPT_STEP_BLOCK_ORDER:
      if (value < 0 || value > 3) return pw_fail(PW_EINVAL, "PW_OPT_STEP_BLOCK_ORDER: 0 first environments first, 1 last first, + 2 a contiguous eighth per XCD");
      e->step_reverse = static_cast<int>(value);
      return PW_OK;
    case PW_OPT_STEP_BOARDS:
      if (value != 0 && value != 2) return pw_fail(PW_EINVAL, "PW_OPT_STEP_BOARDS: 0 automatic, 2 never");
      e->step_boards = static_cast<int>(value);
      return PW_OK;
    case PW_OPT_EXPAND_PAIR_DIMS:
      if (value != 0 && value != 2) return pw_fail(PW_EINVAL, "PW_OPT_EXPAND_PAIR_DIMS: 0 automatic, 2 never");
      e->expand_pair_dims = static_cast<int>(value);
      return PW_OK;
    case PW_OPT_MAILBOX_MODE:
      if (value < 0 || value > 31 || ((value & 8) && (value & 7) != 3)) return pw_fail(PW_EINVAL, "PW_OPT_MAILBOX_MODE: 0 .. 3 (+ 4), or 11; + 16 profile");
      e->mailbox_mode = static_cast<int>(value);
      return PW_OK;
    case PW_OPT_SEARCH_KEYS:
      if (value != 0 && value != 1) return pw_fail(PW_EINVAL, "PW_OPT_SEARCH_KEYS: 0 fingerprinted entries, 1 exact keys where they fit");
      e->search_keys = static_cast<int>(value);
      return PW_OK;
    case PW_OPT_PUSH_SEARCH_FP_BITS:
      if (value < 0 || value > 32) return pw_fail(PW_EINVAL, "PW_OPT_PUSH_SEARCH_FP_BITS: 0 default, 1 .. 32 fingerprint bits");
      e->push_search_fp_bits = static_cast<int>(value);
      return PW_OK;
    case PW_OPT_STEP_QUAD16:
      if (value != 0 && value != 2) return pw_fail(PW_EINVAL, "PW_OPT_STEP_QUAD16: 0 automatic, 2 never");
      e->step_quad16 = static_cast<int>(value);
      return PW_OK;
    case PW_OPT_OBS_TUNE_MS:
      if (value < 0) return pw_fail(PW_EINVAL, "PW_OPT_OBS_TUNE_MS: milliseconds (0 = default 10 000)");
      e->obs_tune_ms = value;
      return PW_OK;
    case PW_OPT_BIND_MIN_ENVS:
      if (value < 0 || value > 65536) return pw_fail(PW_EINVAL, "PW_OPT_BIND_MIN_ENVS: 0 default (48), else 1 .. 65536");
      e->bind_min_envs = static_cast<int>(value);
      return PW_OK;
    case PW_OPT_BIND_MAX_KB:
      if (value < 0 || value > 48) return pw_fail(PW_EINVAL, "PW_OPT_BIND_MAX_KB: 0 default (48), else 1 .. 48");
      e->bind_max_kb = static_cast<int>(value);
      return PW_OK;
    case PW_OPT_MAILBOX_SEG:
      if (value != 0 && value != 2) return pw_fail(PW_EINVAL, "PW_OPT_MAILBOX_SEG: 0 automatic, 2 never");
      e->mailbox_seg = static_cast<int>(value);
      return PW_OK;
    case PW_OPT_STEP_ONE_FUSED:
      if (value < 0 || value > 2) return pw_fail(PW_EINVAL, "PW_OPT_STEP_ONE_FUSED: 0, 1 or 2");
      e->step_one_fused = static_cast<int>(value);
      return PW_OK;
    case PW_OPT_BIND_SPREAD:
      if (value < 0 || (value & 15) > 5 || (value >> 4) > 5)
        return pw_fail(PW_EINVAL, "PW_OPT_BIND_SPREAD: 0 automatic, 1 .. 5 = at most 64 / 32 / 16 / 8 / 4 environments per wavefront (+ 16 x the same for the listed environments)");
      e->bind_spread = static_cast<int>(value);
      return PW_OK;
    case PW_OPT_BIND_ROLLOUTS:
      if (value < 0 || value > 2) return pw_fail(PW_EINVAL, "PW_OPT_BIND_ROLLOUTS: 0 automatic, 1 always, 2 never");
      e->bind_rollouts = static_cast<int>(value);
      return PW_OK;
    case PW_OPT_BIND_LANES:
      if (value < 0 || value > 4) return pw_fail(PW_EINVAL, "PW_OPT_BIND_LANES: 0 automatic, 1 / 2 / 3 / 4 = at most 1 / 2 / 4 / 8 lanes per environment");
      e->bind_lanes = static_cast<int>(value);
      return PW_OK;
    case PW_OPT_BIND_FUSED:
      if (value != 0 && value != 2) return pw_fail(PW_EINVAL, "PW_OPT_BIND_FUSED: 0 automatic, 2 never");
      e->bind_fused = static_cast<int>(value);
      return PW_OK;
    case PW_OPT_STEP_LANE_BATCH:
      if (value < 0) return pw_fail(PW_EINVAL, "PW_OPT_STEP_LANE_BATCH: 0 default, otherwise the smallest batch that runs one lane per environment");
      e->step_lane_batch = value;
      return PW_OK;
    case PW_OPT_STEP_NARROW_GROUPS:
      if (value < 0 || value > 2) return pw_fail(PW_EINVAL, "PW_OPT_STEP_NARROW_GROUPS: 0 automatic, 1 always, 2 never");
      e->step_narrow_groups = static_cast<int>(value);
      return PW_OK;
    case PW_OPT_EXPAND_LDS_TABLES:
      if (value != 0 && value != 2 && value != 3) return pw_fail(PW_EINVAL, "PW_OPT_EXPAND_LDS_TABLES: 0 automatic, 2 never, 3 never + whole runs");
      e->expand_lds_tables = static_cast<int>(value);
      return PW_OK;
    case PW_OPT_EXPAND_TILE_ORDER:
      if (value < 0 || value > 3) return pw_fail(PW_EINVAL, "PW_OPT_EXPAND_TILE_ORDER: 0 interleaved, 1 a contiguous eighth per XCD (+ 2: plain instead of non-temporal stores)");
      e->expand_tile_order = static_cast<int>(value);
      return PW_OK;
    case PW_OPT_EXPAND_PREFETCH:
      if (value != -1 && value != 0 && value != 2) return pw_fail(PW_EINVAL, "PW_OPT_EXPAND_PREFETCH: -1 automatic (= 2), 0 none, 2 two tiles ahead");
      e->expand_prefetch = static_cast<int>(value);
      return PW_OK;
    case PW_OPT_EXPAND_GROUPS_PER_CU:
      if (value < 0 || value > 64) return pw_fail(PW_EINVAL, "PW_OPT_EXPAND_GROUPS_PER_CU: 0 automatic, 1 .. 64");
      e->expand_groups_per_cu = static_cast<int>(value);
      return PW_OK;
    case PW_OPT_EXPAND_WG_WAVES:
      if (value != 0 && value != 4 && value != 8) return pw_fail(PW_EINVAL, "PW_OPT_EXPAND_WG_WAVES: 0 automatic, 4, 8");
      e->expand_wg_waves = static_cast<int>(value);
      return PW_OK;
    case PW_OPT_SEARCH_BATCH_GROUPS_PER_CU:
      if (value < 0 || value > 8) return pw_fail(PW_EINVAL, "PW_OPT_SEARCH_BATCH_GROUPS_PER_CU: 0 automatic, 1 .. 8");
      e->search_batch_groups_per_cu = static_cast<int>(value);
      return PW_OK;
    case PW_OPT_PAGE_ORDER:
      if (value < 0 || value > 2) return pw_fail(PW_EINVAL, "PW_OPT_PAGE_ORDER: 0 address order, 1 eighth per XCD, 2 runs per XCD");
      e->page_order = static_cast<int>(value);
      e->ret.tuned = false;  // (a launch configuration set by hand holds for the live launch too)
      return PW_OK;
    case PW_OPT_PAGE_RUN_LOG2:
      if (value < 0 || value > 20) return pw_fail(PW_EINVAL, "PW_OPT_PAGE_RUN_LOG2: 0 .. 20 (0 .. 2 with page order 1)");
      e->page_run_log2 = static_cast<int>(value);
      e->ret.tuned = false;
      return PW_OK;
    case PW_OPT_PAGE_LDS_PAD_KB:
      if (value < 0 || value > 48) return pw_fail(PW_EINVAL, "PW_OPT_PAGE_LDS_PAD_KB: 0 .. 48");
      e->page_lds_pad_kb = static_cast<int>(value);
      e->ret.tuned = false;
      return PW_OK;
    case PW_OPT_TUNED_NS:
    case PW_OPT_STEP_TABLE_BYTES:
    case PW_OPT_STEP_TABLE_PUZZLES:
    case PW_OPT_EXPAND_FORM:
    case PW_OPT_CELLS_BASE_BYTES:
    case PW_OPT_OBS_LIVE_PAGES:
      return pw_fail(PW_EINVAL, "read-only option");
    case PW_OPT_STEP_TABLES: {
      if (value < 0 || value > 3)
        return pw_fail(PW_EINVAL, "PW_OPT_STEP_TABLES: 0 automatic, 1 every puzzle, 2 none, 3 puzzles with big movables");
      if (static_cast<int>(value) == e->step_tables) return PW_OK;
      PwDeviceGuard guard(e->set->device);
      e->step_tables = static_cast<int>(value);
      return upload_overlap_tables(e);  // rebuilt on the spot (synchronises the device)
    }
    case PW_OPT_PAGE_LOAD_ALL:
      if (value < 0 || value > 1) return pw_fail(PW_EINVAL, "PW_OPT_PAGE_LOAD_ALL: 0 or 1");
      e->page_load_all = static_cast<int>(value);
      e->ret.tuned = false;
      return PW_OK;
    case PW_OPT_OBS_PADDING_ONCE:
      if (value < 0 || value > 3)
        return pw_fail(PW_EINVAL, "PW_OPT_OBS_PADDING_ONCE: 0 off, 1 on (2 / 3: on, with the early-exit / the list form of the live launch)");
      e->ret.option = static_cast<int>(value);
      e->ret.valid = e->ret.shown_valid = false;  // (established by the next full render)
      return PW_OK;
    case PW_OPT_OBS_CHANGED_PAGES:
      if (value != 0 && value != 1) return pw_fail(PW_EINVAL, "PW_OPT_OBS_CHANGED_PAGES: 0 the live launch, 1 the changed pages of it only");
      e->ret.chg_option = static_cast<int>(value);
      e->ret.shown_valid = false;  // (the next pw_step_render into the retained buffer takes the live launch and fills `shown`)
      return PW_OK;
    case PW_OPT_RESAMPLE_FENCE:
      if (value != 0 && value != 1) return pw_fail(PW_EINVAL, "PW_OPT_RESAMPLE_FENCE: 0 the search reads the cdf alone, 1 a fence in LDS");
      e->resample_fence = static_cast<int>(value);
      return PW_OK;
    case PW_OPT_STATS_LDS_PUZZLES:
      if (value < 0 || (value > 1024 && value != 2048)) return pw_fail(PW_EINVAL, "PW_OPT_STATS_LDS_PUZZLES: 0 default, 1 .. 1024 puzzles, 2048 never");
      e->stats_lds_puzzles = static_cast<int>(value);
      return PW_OK;
    case PW_OPT_STATS_GROUPS:
      if (value < 0 || value > (1 << 20)) return pw_fail(PW_EINVAL, "PW_OPT_STATS_GROUPS: 0 one workgroup per 256 environments, or the most workgroups of a launch");
      e->stats_groups = static_cast<int>(value);
      return PW_OK;
    case PW_OPT_OBS_CHUNK_MB:
      if (value < 0 || value > 4096) return pw_fail(PW_EINVAL, "PW_OPT_OBS_CHUNK_MB: 0 (the default, 32 MiB) .. 4096");
      e->obs_chunk_mb = static_cast<int>(value);
      return PW_OK;
    case PW_OPT_OBS_ACCEPT_GBS:
      if (value < 0 || value > 100000) return pw_fail(PW_EINVAL, "PW_OPT_OBS_ACCEPT_GBS: 0 .. 100000 GB/s");
      e->obs_accept_gbs = static_cast<int>(value);
      return PW_OK;
    case PW_OPT_PROFILE_RENDER: {
      if (value < 0 || value > 65536) return pw_fail(PW_EINVAL, "PW_OPT_PROFILE_RENDER: 0 .. 65536 launches");
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
    default:
      return pw_fail(PW_EINVAL, "unknown engine option");
  }
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int64_t pw_engine_get_option(const PwEngine* e, int32_t option) try {
  if (!e) return pw_fail(PW_EINVAL, "null engine");
  switch (option) {
    case PW_OPT_STEP_KERNEL: return e->step_kernel;
    case PW_OPT_FUSED_STEP_RENDER: return e->force_fused ? 1 : 0;
    case PW_OPT_RENDER_KERNEL: return e->force_lds_render ? 1 : 0;
    case PW_OPT_PAGE_SLICE_ENVS: return e->page_slice_envs;
    case PW_OPT_SEARCH_CHUNK: return e->search_chunk;
    case PW_OPT_STEP_LDS_TABLES: return e->step_lds_tables;
    case PW_OPT_STEP_WIDE_GROUPS: return e->step_wide_groups;
    case PW_OPT_STEP_MIXED_GROUPS: return e->step_mixed;
    case PW_OPT_STEP_NARROW_GROUPS: return e->step_narrow_groups;
    case PW_OPT_EXPAND_LDS_TABLES: return e->expand_lds_tables;
    case PW_OPT_EXPAND_TILE_ORDER: return e->expand_tile_order;
    case PW_OPT_EXPAND_PREFETCH: return e->expand_prefetch;
    case PW_OPT_EXPAND_GROUPS_PER_CU: return e->expand_groups_per_cu;
    case PW_OPT_SEARCH_BATCH_GROUPS_PER_CU: return e->search_batch_groups_per_cu;
    case PW_OPT_EXPAND_WG_WAVES: return e->expand_wg_waves;
    case PW_OPT_EXPAND_FORM: return e->expand_form;
    case PW_OPT_CELLS_BASE_BYTES: return e->cells_base_bytes;
    case PW_OPT_STEP_BLOCK_ORDER: return e->step_reverse;
    case PW_OPT_STEP_BOARDS: return e->step_boards;
    case PW_OPT_STEP_BOARD_SET: return e->d_boards ? 1 : 0;
    case PW_OPT_STEP_QUAD16: return e->step_quad16;
    case PW_OPT_BIND_MIN_ENVS: return e->bind_min_envs > 0 ? e->bind_min_envs : 48;
    case PW_OPT_BIND_FUSED: return e->bind_fused;
    case PW_OPT_BIND_LANES: return e->bind_lanes;
    case PW_OPT_BIND_ROLLOUTS: return e->bind_rollouts;
    case PW_OPT_MAILBOX_SEG: return e->mailbox_seg;
    case PW_OPT_STEP_ONE_APPLIES:
      return (!e->fast_u8_ppc3 && e->step_kernel == 0 && !e->force_fused && e->step_one_fused && e->obs_bytes >= (64 << 10)) ? 1 : 0;
    case PW_OPT_MAILBOX_FORM: return mailbox_form_of(e);
    case PW_OPT_STEP_ONE_FUSED: return e->step_one_fused;
    case PW_OPT_BIND_SPREAD: return e->bind_spread;
    case PW_OPT_BIND_MAX_KB: return e->bind_max_kb > 0 ? e->bind_max_kb : 48;
    case PW_OPT_OBS_TUNE_MS: return e->obs_tune_ms > 0 ? e->obs_tune_ms : 10000;
    case PW_OPT_OBS_SCREEN_MS: return e->obs_screen_ms;
    case PW_OPT_BIND_PUZZLES: return e->seg_puzzles;
    case PW_OPT_BIND_MISMATCHES: {
      uint32_t n = 0;
      PwDeviceGuard guard(e->set->device);
      if (hipMemcpy(&n, e->d_scratch + 8, 4, hipMemcpyDeviceToHost) != hipSuccess) return pw_fail(PW_EDEVICE, "PW_OPT_BIND_MISMATCHES: copy failed");
      return n;
    }
    case PW_OPT_SEARCH_KEYS: return e->search_keys;
    case PW_OPT_PUSH_SEARCH_FP_BITS: return e->push_search_fp_bits;
    case PW_OPT_MAILBOX_MODE: return e->mailbox_mode;
    case PW_OPT_EXPAND_PAIR_DIMS: return e->expand_pair_dims;
    case PW_OPT_STEP_QUAD16_PUZZLES: return e->quad_puzzles;
    case PW_OPT_STEP_LANE_BATCH: return e->step_lane_batch == 0 ? step_lane_batch_default(e, false) : e->step_lane_batch;
    case PW_OPT_PAGE_ORDER: return e->page_order;
    case PW_OPT_PAGE_RUN_LOG2: return e->page_run_log2;
    case PW_OPT_PAGE_LDS_PAD_KB: return e->page_lds_pad_kb;
    case PW_OPT_TUNED_NS: return e->tuned_ns;
    case PW_OPT_PAGE_LOAD_ALL: return e->page_load_all;
    case PW_OPT_OBS_PADDING_ONCE: return e->ret.option;
    case PW_OPT_OBS_CHANGED_PAGES: return e->ret.chg_option;
    case PW_OPT_RESAMPLE_FENCE: return e->resample_fence;
    case PW_OPT_STATS_LDS_PUZZLES: return e->stats_lds_puzzles;
    case PW_OPT_STATS_GROUPS: return e->stats_groups;
    case PW_OPT_OBS_LIVE_PAGES: {
      if (!e->ret.valid) return 0;
      if (e->ret.n_live >= 0) return e->ret.n_live;
      uint32_t n = 0;  // (list rebuilt in-stream: its length is on the device)
      PwDeviceGuard guard(e->set->device);
      if (hipMemcpy(&n, e->ret.d_count, 4, hipMemcpyDeviceToHost) != hipSuccess) return pw_fail(PW_EDEVICE, "PW_OPT_OBS_LIVE_PAGES: copy failed");
      return n;
    }
    case PW_OPT_STEP_TABLES: return e->step_tables;
    case PW_OPT_STEP_TABLE_BYTES: return e->ovl_bytes;
    case PW_OPT_STEP_TABLE_PUZZLES: return e->ovl_puzzles;
    case PW_OPT_OBS_CHUNK_MB: return e->obs_chunk_mb;
    case PW_OPT_OBS_ACCEPT_GBS: return e->obs_accept_gbs;
    case PW_OPT_PROFILE_RENDER: return static_cast<int64_t>(e->prof_events.size() / 2);
    default: return pw_fail(PW_EINVAL, "unknown engine option");
  }
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

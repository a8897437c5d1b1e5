// pw_render_kernels.inc -- observation kernels: per-environment LDS kernels, page-ordered kernel,
// incremental redraw.  Part of the single translation unit pw_kernels.hip.

// ------------------------------------------------------------------------------------
// K2 render  (puzzle.py:426-469, :596-638; env_utils.py:44-91)
// ------------------------------------------------------------------------------------
struct RenderArgs {
  const PwPuzzleHeader* hdrs;
  const uint8_t* blob;
  const int32_t* puzzle_id;
  const int8_t* pos;
  uint8_t* obs;
  const uint16_t* estat;      // static zone tables (engine frame layout)
  const uint32_t* estat_off;
  int64_t env_stride;
  int32_t batch;
  int32_t np;
  int32_t ppc, bw;
  int32_t pad_h, pad_w;    // frame in cells
  int32_t obs_bytes;       // bytes of one observation
  uint32_t pal_rgb[16];    // byte0 = R, byte1 = G, byte2 = B
  float pal_f32[16][4];    // uint8 -> float32 / 255 (env_utils.py:65-72), exact IEEE division
  int32_t do_step;         // fused pw_step_render: wave 0 advances the environment first
  int32_t skip_movables;   // draw the static layers only (engine setup: static images)
  int32_t num_puzzles;     // puzzle ids are clamped to 0 .. num_puzzles - 1 (pw_clamp_pid)
  const uint32_t* dirty_rows;  // generic kernel, pw_step_render_delta: per env cell rows to redraw (NULL = all)
  int32_t bands;               // generic kernel, full render: workgroups per environment (>= 1), each streams a
                               // contiguous band of the image -- parallelism for small batches of big frames
  unsigned long long* signal;     // generic kernel, pw_step_render_delta on a batch of one: pinned host
  unsigned long long signal_seq;  // word that receives signal_seq once everything is written (pw_engine_set_step_signal), or NULL
  uint32_t* signal_count;         // device memory: workgroups of the launch that have finished (launches of several workgroups)
  StepArgs step;
};

static void launch_render(PwEngine* e, const RenderArgs& ra, int32_t batch, hipStream_t st, bool rec_ready = false, int live_form = 0, bool track = false);

// LDS layout of the render kernels (dynamic):
//   [0, 16)        8 zero guard entries in front of E
//   E              zone table of this environment, uint16 entries, 16 B aligned; followed by >= 3
//                  zero entries (part of the static table image)
//   spos, pal, flag
struct RenderLds {
  uint16_t* E;
  int16_t* spos;
  uint32_t* pal;
  uint32_t* flag;
};

__device__ __forceinline__ RenderLds carve_lds(unsigned char* smem, int e_bytes) {
  RenderLds l;
  l.E = reinterpret_cast<uint16_t*>(smem + 16);
  l.spos = reinterpret_cast<int16_t*>(smem + 16 + e_bytes);
  l.pal = reinterpret_cast<uint32_t*>(smem + 16 + e_bytes + 64);
  l.flag = l.pal + 16;
  return l;
}

// Writes the three sub-row entries of one movable cell over the static table.
__device__ __forceinline__ void patch_cell(const PuzzleView& pv, uint16_t* E, const int16_t* spos, uint32_t c,
                                           int estride, int c0, int row_lo = 0, int row_hi = PW_MAX_DIM) {
  const int obj = c >> 24;
  const int p = static_cast<uint16_t>(spos[obj]);
  const int x = static_cast<int8_t>(p & 0xff) + static_cast<int>(c & 0xff);
  const int y = static_cast<int8_t>((p >> 8) & 0xff) + static_cast<int>((c >> 8) & 0xff);
  if (static_cast<unsigned>(x) >= static_cast<unsigned>(pv.W) || static_cast<unsigned>(y) >= static_cast<unsigned>(pv.H) ||
      y < row_lo || y >= row_hi)
    return;
  const uint32_t kind = obj == 0 ? 3u : (obj <= pv.G ? 4u : 5u);
  const uint32_t om = (c >> 16) & 0xffu;
#pragma unroll
  for (int zy = 0; zy < 3; zy++) {
    const int idx = (3 * y + zy) * estride + x + c0;
    const uint32_t gb = pw_entry_goal_bits(E[idx]);  // goal outlines stay on top (puzzle.py:458)
    E[idx] = static_cast<uint16_t>(pw_zone_entry(kind, pw_zone_border_bits(om, zy), gb));
  }
}

// Per-environment zone table: the puzzle's static table (walls, agent walls, background, goal
// outlines; precomputed per engine) is copied into LDS with 16-byte loads and the cells under
// the movables are patched in painter order (puzzle.py:453-458).  In an overlap-free state
// (always, under legal play) no two movables share a cell and the patches are independent;
// otherwise objects are applied one after the other so that a higher index wins.
// Only the cell rows [row_lo, row_hi) are needed by the caller (incremental redraw): the rest of the table
// is neither copied nor patched.
__device__ __forceinline__ void build_zone_table(const RenderArgs& a, const PuzzleView& pv, int pid, int env,
                                                 const RenderLds& l, int estride, int c0, int row_lo = 0,
                                                 int row_hi = PW_MAX_DIM, const int16_t* lds_xy = nullptr) {
  const int tid = threadIdx.x;
  const int lane = tid & (PW_WAVE - 1);
  const int n_entries = 3 * pv.H * estride;
  const int n16 = (2 * (n_entries + 3) + 15) >> 4;
  const uint4* src = reinterpret_cast<const uint4*>(reinterpret_cast<const uint8_t*>(a.estat) + a.estat_off[pid]);
  uint4* dst = reinterpret_cast<uint4*>(l.E);
  const int i_lo = (2 * 3 * max(row_lo, 0) * estride) >> 4;
  const int i_hi = min(n16, (2 * (3 * min(row_hi, pv.H) * estride + 3) + 15) >> 4);
  for (int i = i_lo + tid; i < i_hi; i += blockDim.x) dst[i] = src[i];
  if (tid < 16) l.pal[tid] = a.pal_rgb[tid];
  if (tid >= 64 && tid < 72) l.E[tid - 72] = 0;  // guard entries E[-8..-1]
  if (tid < PW_WAVE) {
    // wave 0: (fused step,) positions to LDS + overlap check of the state to draw
    int xy = 0;
    bool legal;
    if (lds_xy) {  // (pw_step_render_one_kernel: the positions were handed over in LDS)
      if (lane < 32) xy = static_cast<uint16_t>(lds_xy[lane]);
      legal = load_boards(pv, xy, lane).legal;
    } else if (a.do_step) {
      step_one_env(a.step, env, lane, pv, xy, legal);
    } else {
      if (lane < a.np) xy = static_cast<uint16_t>(reinterpret_cast<const int16_t*>(a.pos)[static_cast<int64_t>(env) * a.np + lane]);
      legal = load_boards(pv, xy, lane).legal;
    }
    if (lane < 32) l.spos[lane] = static_cast<int16_t>(xy);
    if (lane == 0) l.flag[0] = legal ? 1u : 0u;
  }
  __syncthreads();
  if (a.skip_movables) return;
  if (l.flag[0]) {
    for (int m = tid; m < pv.n_mcells; m += blockDim.x)
      patch_cell(pv, l.E, l.spos, pv.mcells[m], estride, c0, row_lo, row_hi);
  } else {
    for (int j = 0; j < pv.N; j++) {
      for (int m = tid; m < pv.n_mcells; m += blockDim.x) {
        const uint32_t c = pv.mcells[m];
        if (static_cast<int>(c >> 24) == j) patch_cell(pv, l.E, l.spos, c, estride, c0, row_lo, row_hi);
      }
      __syncthreads();
    }
  }
  __syncthreads();
}

// Fast path: uint8 observation, pixels_per_cell = 3, border_width = 1 (zones == pixels).
// A zone-table entry is then exactly 3 pixels = 9 bytes of one image row, and because the
// frame is pad_w * 3 pixels wide the table (row stride pad_w) is the image itself in
// 9-byte units: output byte o belongs to entry floor((o - shift) / 9).
__global__ __launch_bounds__(PW_RENDER_THREADS) void pw_render_u8_ppc3_kernel(RenderArgs a) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int env = blockIdx.x;
  const int tid = threadIdx.x;
  const int pid = pw_clamp_pid(a.puzzle_id[env], a.num_puzzles);
  const PuzzleView pv = view_of(a.hdrs, a.blob, pid);

  // pixel padding of env_utils.py:75-91 (left/top get the floor half)
  const int wpx = a.pad_w * 3;
  const int pady = (a.pad_h - pv.H) * 3 / 2;
  const int padx = (a.pad_w - pv.W) * 3 / 2;
  const int c0 = (padx + 2) / 3;  // virtual cell columns left of the puzzle
  const int n_entries = 3 * pv.H * a.pad_w;
  const RenderLds l = carve_lds(smem, ((2 * (n_entries + 3) + 15) >> 4) << 4);
#ifdef PW_STAGGER
  // De-correlate the first generation of workgroups: all workgroups take equally long, so
  // without this the whole chip alternates between "everyone in the preamble" and "everyone
  // streaming" for the entire launch.
  if (blockIdx.x < PW_STAGGER) {
    const unsigned h = (blockIdx.x * 2654435761u) >> 26;
    for (unsigned i = 0; i < h; i++) __builtin_amdgcn_s_sleep(8);
  }
#endif
  build_zone_table(a, pv, pid, env, l, a.pad_w, c0);
  const uint16_t* E = l.E;
  const uint32_t* pal = l.pal;

  const int shift_bytes = 3 * (pady * wpx + padx - 3 * c0);  // may be negative by < 9 bytes per row
  // bias keeps the dividend non-negative; multiple of 9
  const int bias_q = (shift_bytes > 0 ? shift_bytes / 9 : 0) + 2;
  const int n_chunks = (a.obs_bytes + 15) >> 4;
  uint8_t* out = a.obs + static_cast<int64_t>(env) * a.env_stride;

  for (int chunk = tid; chunk < n_chunks; chunk += PW_RENDER_THREADS) {
    const unsigned o3 = static_cast<unsigned>(chunk * 16 - shift_bytes + 9 * bias_q);
    const unsigned qb = o3 / 9u;
    const int b = static_cast<int>(o3 - qb * 9u);
    int q0 = static_cast<int>(qb) - bias_q;
    q0 = min(max(q0, -3), n_entries);
    const uint32_t e0 = E[q0], e1 = E[q0 + 1], e2 = E[q0 + 2];
    // 9-byte pixel triples -> the 24 bytes d0..d5 of the concatenation
    const uint32_t r00 = pal[e0 & 15u], r01 = pal[(e0 >> 4) & 15u], r02 = pal[(e0 >> 8) & 15u];
    const uint32_t r10 = pal[e1 & 15u], r11 = pal[(e1 >> 4) & 15u], r12 = pal[(e1 >> 8) & 15u];
    const uint32_t r20 = pal[e2 & 15u], r21 = pal[(e2 >> 4) & 15u];
    const uint32_t d0 = r00 | (r01 << 24);
    const uint32_t d1 = (r01 >> 8) | (r02 << 16);
    const uint32_t d2 = (r02 >> 16) | (r10 << 8);
    const uint32_t d3 = r11 | (r12 << 24);
    const uint32_t d4 = (r12 >> 8) | (r20 << 16);
    const uint32_t d5 = (r20 >> 16) | (r21 << 8);
    // byte-granular funnel shift by b (0..8): dword select by b >> 2, then v_alignbyte by b & 3
    const int sel = b >> 2;
    const uint32_t s0 = sel == 0 ? d0 : (sel == 1 ? d1 : d2);
    const uint32_t s1 = sel == 0 ? d1 : (sel == 1 ? d2 : d3);
    const uint32_t s2 = sel == 0 ? d2 : (sel == 1 ? d3 : d4);
    const uint32_t s3 = sel == 0 ? d3 : (sel == 1 ? d4 : d5);
    const uint32_t s4 = sel == 0 ? d4 : d5;  // sel == 2 implies b == 8: byte shift 0, s4 unused
    const uint32_t bs = static_cast<uint32_t>(b & 3);
    uint4 v;
    v.x = __builtin_amdgcn_alignbyte(s1, s0, bs);
    v.y = __builtin_amdgcn_alignbyte(s2, s1, bs);
    v.z = __builtin_amdgcn_alignbyte(s3, s2, bs);
    v.w = __builtin_amdgcn_alignbyte(s4, s3, bs);
    // plain store: nt stores measured 4-7 % slower for this access pattern
    *reinterpret_cast<uint4*>(out + static_cast<int64_t>(chunk) * 16) = v;
  }
}

// geometry of the page-ordered kernels below: the observation buffer as a flat run of 16-byte chunks
struct CopyArgs {
  const uint8_t* simg;
  const int32_t* puzzle_id;
  uint8_t* obs;
  int64_t simg_stride;
  int32_t batch;
  uint32_t chunks_per_env;  // env stride / 16
  uint32_t n_chunks;        // 16-byte chunks of one observation
  float inv_cpe;            // 1 / chunks_per_env
  const PageRec* rec;       // [batch] page records (page kernel)
  uint32_t magic_cellrow;   // ceil(2^32 / (27 * pad_w)): channels -> cell row by one mulhi
  uint32_t n_pages;         // pages of this launch (the grid may be rounded up, see `order`)
  // Which page a workgroup takes.  Workgroups are dispatched round-robin over the 8 XCDs (workgroup i runs on XCD
  // i mod 8), so with the identity mapping every XCD writes every 8th page.
  //   0  page = workgroup index
  //   1  the buffer in 8 >> run_log2 contiguous parts, XCD k sweeps part k mod parts (run_log2 0: one eighth per XCD)
  //   2  XCD k writes runs of 2^run_log2 consecutive pages; the chip-wide write front stays 8 runs wide
  // Same bytes either way; which one is fastest depends on the physical backing of the buffer (pw_engine_tune_render).
  uint32_t order;
  uint32_t run_log2;
  const uint8_t* zero_page;  // 4 KiB of zeros: what the every-page-loads instance loads for pages of the frame padding
  // live-page launch of a retained observation buffer (kLive = 1, PW_OPT_OBS_PADDING_ONCE): workgroup i renders page live[i]
  const uint32_t* live;      // pages with a chunk outside the frame padding, ascending
  const uint32_t* live_n;    // device-side length of `live` when the host does not know it (list rebuilt in-stream: the grid is
                             // the upper bound n_pages and the workgroups beyond the count return), else NULL
  uint32_t n_live;           // length of `live` as the host knows it (ignored with live_n)
  // changed-page launch (kLive = 3, PW_OPT_OBS_CHANGED_PAGES): the list form, and a workgroup returns when none of its page's pixel
  // rows differs from what the buffer holds
  const uint64_t* changed;   // [batch] bit y: grid row y of the environment may show other pixels than the buffer (pw_shown_rows)
};

// grid of a page-ordered launch over n indices: orders 1 and 2 permute a rounded-up index range; the surplus workgroups exit
__host__ __device__ inline unsigned page_grid(uint32_t n, uint32_t order, uint32_t run_log2) {
  if (order == 1u) return (n + 7u) & ~7u;
  if (order == 2u) {
    const unsigned span = 8u << run_log2;
    return (n + span - 1u) / span * span;
  }
  return n;
}

struct PageRecArgs {
  const PwPuzzleHeader* hdrs;
  const int32_t* puzzle_id;
  const int8_t* pos;
  PageRec* out;
  int32_t batch;
  int32_t np;
  int32_t num_puzzles;
  int8_t* shown;      // PW_OPT_OBS_CHANGED_PAGES (StepArgs::shown / changed), or both NULL
  uint64_t* changed;
};

__global__ __launch_bounds__(256) void pw_page_records_kernel(PageRecArgs a) {
  const int env = blockIdx.x * 256 + threadIdx.x;
  if (env >= a.batch) return;
  const int pid = pw_clamp_pid(a.puzzle_id[env], a.num_puzzles);
  const PwPuzzleHeader& h = a.hdrs[pid];
  const int8_t* row = a.pos + static_cast<int64_t>(env) * a.np * 2;
  uint64_t rows = 0;
  for (int j = 0; j < h.N; j++) {
    const int y = row[2 * j + 1], hh = h.objtab[j].h;
    const uint64_t m = hh >= 64 ? ~0ull : ((1ull << hh) - 1ull);
    if (static_cast<unsigned>(y) < 64u) rows |= m << y;
  }
  PageRec r;
  r.pid = pid;
  r.H = h.H;
  r.W = h.W;
  r.reserved = 0;
  r.rows = rows;
  a.out[env] = r;
  if (a.changed)
    pw_shown_update(row, a.shown + static_cast<int64_t>(env) * a.np * 2, a.changed + env, h.N, [&](int j) { return static_cast<int>(h.objtab[j].h); });
}

// ------------------------------------------------------------------------------------
// Page render (ppc 3; uint8 and float32): ONE pass, page ordered.  A workgroup is a single wavefront that
// owns one 4 KiB page of the observation buffer; which page is CopyArgs::order (short-lived workgroups sweeping
// the buffer in a dense front are the pattern HBM sustains best, DESIGN.md section 4 K2).  Chunks that no movable
// touches (98.8 % on the Level-1 mix) are copied from the puzzle's L2-resident static image -- or are zero without
// a load in the frame padding; the wave finds the movable-cell entries that intersect its page (one pass over the
// puzzle's movable-cell list, 64 cells at a time), keeps them in an LDS list and recomputes only the chunks they
// touch from zone entries -- every byte of the observation is written exactly once, as part of a full 16-byte
// non-temporal store.
// ------------------------------------------------------------------------------------
#define PW_PAGE_ENTRIES 472  // zone entries a 4 KiB page can touch (4096 / 9 + margins), multiple of 8

// geometry of one environment's image inside the frame (workgroup-uniform)
struct PageEnv {
  const PwPuzzleHeader* h;
  const uint16_t* estat;
  int W, H, N, G, n_mcells, c0, shift_bytes, n_entries;
  int lo;     // byte offset of the page start inside this environment's image (may be negative)
  int q_lo;   // first entry kept in the page's LDS entry window
  uint32_t env;
};

// ES = bytes per channel value (1: uint8, 4: float32).  Offsets inside an image are kept in BYTES (`lo`);
// entries are addressed in channel units: entry q covers channels [9 q + shift, 9 q + shift + 9).
template <int ES>
__device__ __forceinline__ PageEnv page_env(const RenderArgs& a, int pid, uint32_t env, int lo) {
  PageEnv pe;
  pe.h = a.hdrs + pid;
  pe.estat = reinterpret_cast<const uint16_t*>(reinterpret_cast<const uint8_t*>(a.estat) + a.estat_off[pid]);
  pe.W = pe.h->W;
  pe.H = pe.h->H;
  pe.N = pe.h->N;
  pe.G = pe.h->G;
  pe.n_mcells = static_cast<int>(pe.h->n_mcells);
  const int pady = (a.pad_h - pe.H) * 3 / 2;
  const int padx = (a.pad_w - pe.W) * 3 / 2;
  pe.c0 = (padx + 2) / 3;
  pe.shift_bytes = 3 * (pady * a.pad_w * 3 + padx - 3 * pe.c0);
  pe.n_entries = 3 * pe.H * a.pad_w;
  pe.lo = lo;
  // entry holding the first channel of the page is floor((lo / ES - shift) / 9); two entries of margin
  const int t = (lo >= 0 ? lo / ES : -((-lo) / ES)) - pe.shift_bytes;
  pe.q_lo = (t >= 0 ? t / 9 : -((-t + 8) / 9)) - 2;
  pe.env = env;
  return pe;
}

// Movable cells of the environment that reach into the page [lo, lo + 4096): their zone entries go
// into the page's LDS entry window `win` (atomicMax on (object + 1) << 12 | entry: the highest
// object index wins = painter order, puzzle.py:457) and the chunks they touch are marked in
// `dirty`.  page_prefilter() tells beforehand whether any object's rows meet the page at all.
// packed positions of an environment's movables, lane j = movable j (zero padding beyond N); needs
// no puzzle data, so it is issued before the puzzle id is known
__device__ __forceinline__ int page_load_xy(const RenderArgs& a, uint32_t env, int lane) {
  int xy = 0;
  if (lane < a.np) xy = static_cast<uint16_t>(reinterpret_cast<const int16_t*>(a.pos)[static_cast<int64_t>(env) * a.np + lane]);
  return xy;
}

// `any` = some movable's rows meet the page
template <int ES>
__device__ __forceinline__ bool page_prefilter(const RenderArgs& a, const PageEnv& pe, int lane, int xy) {
  const int row_bytes = 9 * a.pad_w;  // one image row, in channels
  const int lo = pe.lo / ES, hi = lo + 4096 / ES;  // (exact: lo is a multiple of 16, also when negative)
  bool hit = false;
  if (lane < pe.N) {
    const int y = static_cast<int8_t>((xy >> 8) & 0xff);
    const int hh = pe.h->objtab[lane].h;
    hit = 3 * y * row_bytes + pe.shift_bytes < hi && 3 * (y + hh) * row_bytes + pe.shift_bytes + 9 > lo;
  }
  return __ballot(hit) != 0ull;
}

template <int ES>
__device__ __forceinline__ void page_mark(const RenderArgs& a, const PageEnv& pe, int lane, int xy, uint32_t* win, uint32_t* dirty) {
  const int row_bytes = 9 * a.pad_w;  // one image row, in channels
  const int lo = pe.lo / ES, hi = lo + 4096 / ES;
  const uint32_t* mcells = reinterpret_cast<const uint32_t*>(a.blob + pe.h->base + pe.h->off_mcells);
  for (int m0 = 0; m0 < pe.n_mcells; m0 += PW_WAVE) {
    const int m = m0 + lane;
    const uint32_t c = m < pe.n_mcells ? mcells[m] : 0u;
    const int obj = c >> 24;
    const int p = __shfl(xy, obj, PW_WAVE);
    const int x = static_cast<int8_t>(p & 0xff) + static_cast<int>(c & 0xff);
    const int y = static_cast<int8_t>((p >> 8) & 0xff) + static_cast<int>((c >> 8) & 0xff);
    const int q0 = 3 * y * a.pad_w + x + pe.c0;
    const int b00 = 9 * q0 + pe.shift_bytes;  // first byte of the cell's top sub-row
    if (m >= pe.n_mcells || static_cast<unsigned>(x) >= static_cast<unsigned>(pe.W) ||
        static_cast<unsigned>(y) >= static_cast<unsigned>(pe.H) || b00 >= hi || b00 + 2 * row_bytes + 9 <= lo)
      continue;
    const uint32_t kind = obj == 0 ? 3u : (obj <= pe.G ? 4u : 5u);
    const uint32_t om = (c >> 16) & 0xffu;
#pragma unroll
    for (int zy = 0; zy < 3; zy++) {
      const int q = q0 + zy * a.pad_w;
      const int b0 = b00 + zy * row_bytes;
      if (b0 + 9 <= lo || b0 >= hi) continue;
      const uint32_t e = pw_zone_entry(kind, pw_zone_border_bits(om, zy), pw_entry_goal_bits(pe.estat[q]));
      atomicMax(&win[q - pe.q_lo], (static_cast<uint32_t>(obj + 1) << 12) | e);
      const int cl = (max(b0 - lo, 0) * ES) >> 4, ch = (min(b0 + 8 - lo, 4096 / ES - 1) * ES) >> 4;
      if (ES == 1) {  // 9 bytes touch at most two 16-byte chunks
        atomicOr(&dirty[cl >> 5], 1u << (cl & 31));
        atomicOr(&dirty[ch >> 5], 1u << (ch & 31));
      } else {        // 36 bytes: up to four
        for (int cc = cl; cc <= ch; cc++) atomicOr(&dirty[cc >> 5], 1u << (cc & 31));
      }
    }
  }
}

// the 16 bytes of chunk c (inside the environment's image) from the page's entry window + static table
typedef unsigned int pw_u32x4 __attribute__((ext_vector_type(4)));
// float32: chunk c = channels 4 c .. 4 c + 3 of the environment's image = parts of at most two entries;
// palf = the 16 x 4 table of exact uint8 / 255 values (env_utils.py:65-72)
__device__ __forceinline__ pw_u32x4 page_chunk_f32(const PageEnv& pe, int c, const uint32_t* win, const float* palf) {
  const int bias_q = (pe.shift_bytes > 0 ? pe.shift_bytes / 9 : 0) + 2;
  const unsigned o3 = static_cast<unsigned>(c * 4 - pe.shift_bytes + 9 * bias_q);
  const unsigned qb = o3 / 9u;
  const int r0 = static_cast<int>(o3 - qb * 9u);
  const int q0 = static_cast<int>(qb) - bias_q;
  const uint32_t w0 = win[q0 - pe.q_lo], w1 = win[q0 + 1 - pe.q_lo];
  const uint32_t e0 = w0 ? (w0 & 0xFFFu) : ((static_cast<unsigned>(q0) < static_cast<unsigned>(pe.n_entries)) ? pe.estat[q0] : 0u);
  const uint32_t e1 = w1 ? (w1 & 0xFFFu) : ((static_cast<unsigned>(q0 + 1) < static_cast<unsigned>(pe.n_entries)) ? pe.estat[q0 + 1] : 0u);
  union {
    float f[4];
    pw_u32x4 v;
  } out;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int r = r0 + k;
    const uint32_t e = r < 9 ? e0 : e1;
    const int rr = r < 9 ? r : r - 9;
    const int px = rr >= 6 ? 2 : (rr >= 3 ? 1 : 0);
    out.f[k] = palf[((e >> (4 * px)) & 15u) * 4 + (rr - 3 * px)];
  }
  return out.v;
}

__device__ __forceinline__ pw_u32x4 page_chunk(const PageEnv& pe, int c, const uint32_t* win, const uint32_t* pal) {
  const int bias_q = (pe.shift_bytes > 0 ? pe.shift_bytes / 9 : 0) + 2;
  const unsigned o3 = static_cast<unsigned>(c * 16 - pe.shift_bytes + 9 * bias_q);
  const unsigned qb = o3 / 9u;
  const int b = static_cast<int>(o3 - qb * 9u);
  const int q0 = static_cast<int>(qb) - bias_q;
  uint32_t e0, e1, e2;
  {
    const uint32_t w0 = win[q0 - pe.q_lo], w1 = win[q0 + 1 - pe.q_lo], w2 = win[q0 + 2 - pe.q_lo];
    e0 = w0 ? (w0 & 0xFFFu) : ((static_cast<unsigned>(q0) < static_cast<unsigned>(pe.n_entries)) ? pe.estat[q0] : 0u);
    e1 = w1 ? (w1 & 0xFFFu) : ((static_cast<unsigned>(q0 + 1) < static_cast<unsigned>(pe.n_entries)) ? pe.estat[q0 + 1] : 0u);
    e2 = w2 ? (w2 & 0xFFFu) : ((static_cast<unsigned>(q0 + 2) < static_cast<unsigned>(pe.n_entries)) ? pe.estat[q0 + 2] : 0u);
  }
  const uint32_t r00 = pal[e0 & 15u], r01 = pal[(e0 >> 4) & 15u], r02 = pal[(e0 >> 8) & 15u];
  const uint32_t r10 = pal[e1 & 15u], r11 = pal[(e1 >> 4) & 15u], r12 = pal[(e1 >> 8) & 15u];
  const uint32_t r20 = pal[e2 & 15u], r21 = pal[(e2 >> 4) & 15u];
  const uint32_t d0 = r00 | (r01 << 24);
  const uint32_t d1 = (r01 >> 8) | (r02 << 16);
  const uint32_t d2 = (r02 >> 16) | (r10 << 8);
  const uint32_t d3 = r11 | (r12 << 24);
  const uint32_t d4 = (r12 >> 8) | (r20 << 16);
  const uint32_t d5 = (r20 >> 16) | (r21 << 8);
  const int sel = b >> 2;
  const uint32_t s0 = sel == 0 ? d0 : (sel == 1 ? d1 : d2);
  const uint32_t s1 = sel == 0 ? d1 : (sel == 1 ? d2 : d3);
  const uint32_t s2 = sel == 0 ? d2 : (sel == 1 ? d3 : d4);
  const uint32_t s3 = sel == 0 ? d3 : (sel == 1 ? d4 : d5);
  const uint32_t s4 = sel == 0 ? d4 : d5;
  const uint32_t bs = static_cast<uint32_t>(b & 3);
  return pw_u32x4{__builtin_amdgcn_alignbyte(s1, s0, bs), __builtin_amdgcn_alignbyte(s2, s1, bs),
                  __builtin_amdgcn_alignbyte(s3, s2, bs), __builtin_amdgcn_alignbyte(s4, s3, bs)};
}

#define PAGE_CHUNK(...) (ES == 1 ? page_chunk(__VA_ARGS__, pal) : page_chunk_f32(__VA_ARGS__, reinterpret_cast<const float*>(pal)))
// cell rows of `rows` whose pixels reach into the channel range [lo, hi) of the environment's image:
// row r covers channels [27 pad_w r + shift, 27 pad_w (r + 1) + shift + 9) (the + 9: entries are 9 channels wide)
__device__ __forceinline__ uint64_t page_rows_hit(uint64_t rows, int lo, int hi, int shift, uint32_t magic_cellrow) {
  const int top = hi - shift;      // rows r with 27 pad_w r < top
  const int bot = lo - shift - 9;  // rows r with 27 pad_w (r + 1) > bot
  if (top <= 0) return 0ull;
  const uint32_t r_hi = __umulhi(static_cast<uint32_t>(top - 1), magic_cellrow);  // floor((top - 1) / (27 pad_w))
  const uint32_t r_lo = bot > 0 ? __umulhi(static_cast<uint32_t>(bot), magic_cellrow) : 0u;
  if (r_lo >= 64u) return 0ull;
  const uint64_t upto = r_hi >= 63u ? ~0ull : ((2ull << r_hi) - 1ull);
  return rows & upto & (~0ull << r_lo);
}

// frame geometry of one environment from its page record (workgroup-uniform, no memory access)
struct PageGeom {
  int shift;   // channel of entry 0 (may be negative by < 9)
  int nz_lo;   // chunks [nz_lo, nz_hi) of the image hold the puzzle's own pixel rows; everything else is frame
  int nz_hi;   // padding (zero, env_utils.py:75-91) and is neither loaded nor computed
};

template <int ES>
__device__ __forceinline__ PageGeom page_geom_hw(int pad_h, int pad_w, int H, int W) {
  PageGeom g;
  const int pady = (pad_h - H) * 3 / 2, padx = (pad_w - W) * 3 / 2;
  const int c0 = (padx + 2) / 3;
  g.shift = 3 * (pady * pad_w * 3 + padx - 3 * c0);
  const int row_b = 9 * pad_w * ES;  // one pixel row of the frame in bytes
  g.nz_lo = (pady * row_b) >> 4;
  g.nz_hi = ((pady + 3 * H) * row_b + 15) >> 4;
  return g;
}

template <int ES>
__device__ __forceinline__ PageGeom page_geom(const RenderArgs& a, const PageRec& r) {
  return page_geom_hw<ES>(a.pad_h, a.pad_w, r.H, r.W);
}

// chunks [lo, hi) of an environment's image all lie in its frame padding (or there are none)
__device__ __forceinline__ bool page_chunks_padding(const PageGeom& g, int lo, int hi) {
  return lo >= hi || hi <= g.nz_lo || lo >= g.nz_hi;
}

// A page that holds the tail of one environment (its chunks from c_first on) and, with has_second, the head of the next
// (whose image starts at local chunk `split`): every chunk the page kernel stores there is frame padding
__device__ __forceinline__ bool page_tail_head_padding(const PageGeom& g0, const PageGeom& g1, int c_first, int split,
                                                       int n_chunks, bool has_second) {
  return page_chunks_padding(g0, c_first, n_chunks) && (!has_second || page_chunks_padding(g1, 0, min(256 - split, n_chunks)));
}

// The observation stores are NON-TEMPORAL: the written lines are not kept in L2, which keeps the static images
// there.  Measured on C3: plain / sc0 / sc1 / sc0 sc1 stores 0.85-0.90 ms, nt 0.65 ms, sc1 nt 0.635 ms
// in the default launch configuration but 3 % slower in the tuned ones (profiles/r02_page_xp.txt).  The policy is
// fixed at compile time on purpose: a RUNTIME choice between a
// non-temporal and a plain store makes hipcc merge the two and drop the hint.
#define PAGE_STORE(v, p) __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(p))

// kTag: 0 = launches of pw_render / pw_step_render, 1 = the trial launches of pw_engine_tune_render -- the same code
// under a second symbol, so that a kernel trace (rocprofv3 --stats) averages the two separately.
// kLoadAll (PW_OPT_PAGE_LOAD_ALL, a tuner candidate): every page issues four loads before it stores, also the pages of
// the frame padding that are known to be zero -- the zero pages then stop racing ahead of the others, and the chip-wide
// write front is less ragged: 2.3 % faster on the allocations of the slow class (profiles/r02_xcd_probe.txt,
// page_loadall), and the instance the tuner picks on most fast-class buffers too.  Padding pages load from ONE 4 KiB page
// of zeros (always cache resident: no HBM traffic, also for pools whose static images are not), the others their
// static-image chunks (zeros where the frame padding begins): the bytes are the same.
// kLive (PW_OPT_OBS_PADDING_ONCE, pw_step_render into a retained buffer whose frame padding is known to be written): 1 = the
// page order is applied to the index into the list of live pages, and the workgroup renders page live[i]; 2 = the grid of the
// full render, and the workgroups of padding pages return before they load or store anything (the comparison variant).  The
// pages that are rendered run the same code either way.  3 (PW_OPT_OBS_CHANGED_PAGES) = the list form, and the workgroups of pages
// none of whose pixel rows changed since the buffer was last written (CopyArgs::changed) return before any vector load or store.
template <typename T, int kTag = 0, bool kLoadAll = false, int kLive = 0>
__global__ __launch_bounds__(64) void pw_render_page_kernel(RenderArgs a, CopyArgs ca) {
  typedef pw_u32x4 u32x4;
  constexpr int ES = static_cast<int>(sizeof(T));
  __shared__ uint32_t pal[ES == 1 ? 16 : 64];  // uint8: packed RGB; float32: 16 x 4 float bit patterns
  __shared__ uint32_t dirty[8];
  __shared__ __align__(16) uint32_t win0[PW_PAGE_ENTRIES];
  __shared__ __align__(16) uint32_t win1[PW_PAGE_ENTRIES];
  // (the launch may add dynamic LDS that nothing references: it caps the workgroups per CU, i.e. the width of the
  // chip-wide write front -- 13-14 per CU instead of 32 measured 7-10 % faster, pw_engine_tune_render)
  const int lane = threadIdx.x;

  // ---- workgroup-uniform bookkeeping -------------------------------------------------------------
  uint32_t page = blockIdx.x;
  uint32_t n_sweep = ca.n_pages;  // indices the page order permutes
  if (kLive == 1 || kLive == 3) {
    n_sweep = ca.n_live;
    if (ca.live_n) {
      n_sweep = *ca.live_n;
      if (page >= page_grid(n_sweep, ca.order, ca.run_log2)) return;  // (beyond the range the order permutes onto itself)
    }
  }
  if (ca.order == 1u) {
    // 8 >> run_log2 contiguous parts: XCD k writes in part k mod parts, the XCDs sharing a part interleave its pages
    const uint32_t pl = 3u - ca.run_log2, parts = 1u << pl, k = page & 7u, j = page >> 3;
    const uint32_t per = ((n_sweep + 7u) >> 3) << ca.run_log2;  // pages per part
    page = (k & (parts - 1u)) * per + ((j << ca.run_log2) | (k >> pl));
  } else if (ca.order == 2u) {
    const uint32_t sb = ca.run_log2, j = page >> 3, k = page & 7u;
    page = ((((j >> sb) << 3) + k) << sb) | (j & ((1u << sb) - 1u));
  }
  if (page >= n_sweep) return;
  if (kLive == 1 || kLive == 3) page = ca.live[page];
  const uint32_t g0 = page * 256u;  // first 16-byte chunk of the page
  const uint32_t cpe = ca.chunks_per_env;
  // g0 / cpe without an integer division: float estimate (exact to +-1 for g0 < 2^31) + correction
  uint32_t env0 = static_cast<uint32_t>(static_cast<float>(g0) * ca.inv_cpe);
  {
    const int rr = static_cast<int>(g0 - env0 * cpe);
    if (rr < 0) env0 -= 1u;
    else if (rr >= static_cast<int>(cpe)) env0 += 1u;
  }
  env0 = __builtin_amdgcn_readfirstlane(env0);
  const uint32_t last = static_cast<uint32_t>(a.batch) - 1u;
  const int c_first = static_cast<int>(g0 - env0 * cpe);  // chunk index of the page start inside env0
  uint8_t* dst = a.obs + static_cast<int64_t>(g0) * 16 + lane * 16;
  const PageRec r0 = ca.rec[env0];  // ONE scalar load: puzzle, frame geometry, rows with movables
  const PageGeom g = page_geom<ES>(a, r0);
  uint64_t ch0 = 0ull;  // (kLive = 3: scalar loads next to the record's)
  if (kLive == 3) ch0 = ca.changed[env0];

  if (c_first + 256 <= static_cast<int>(ca.n_chunks)) {
    // ---- 13 of 14 pages: the whole page lies inside one environment's image ----------------------
    const u32x4 zero = u32x4{0u, 0u, 0u, 0u};
    u32x4 v0 = zero, v1 = zero, v2 = zero, v3 = zero;
    if (kLive == 2 && page_chunks_padding(g, c_first, c_first + 256)) return;
    if (kLive == 3 && page_rows_hit(ch0, (c_first * 16) / ES, (c_first * 16 + 4096) / ES, g.shift, ca.magic_cellrow) == 0ull) return;
    if (!kLoadAll && (c_first + 256 <= g.nz_lo || c_first >= g.nz_hi)) {  // frame padding above / below the puzzle: no loads at all
      PAGE_STORE(v0, dst);
      PAGE_STORE(v1, dst + 1024);
      PAGE_STORE(v2, dst + 2048);
      PAGE_STORE(v3, dst + 3072);
      return;
    }
    const bool pad_page = c_first + 256 <= g.nz_lo || c_first >= g.nz_hi;  // (only reached with kLoadAll when true)
    const uint8_t* src = (kLoadAll && pad_page)
                             ? ca.zero_page + lane * 16
                             : ca.simg + static_cast<int64_t>(r0.pid) * ca.simg_stride + static_cast<int64_t>(c_first) * 16 + lane * 16;
    const int c = c_first + lane;
    if (kLoadAll || (c >= g.nz_lo && c < g.nz_hi)) v0 = *reinterpret_cast<const u32x4*>(src);
    if (kLoadAll || (c + 64 >= g.nz_lo && c + 64 < g.nz_hi)) v1 = *reinterpret_cast<const u32x4*>(src + 1024);
    if (kLoadAll || (c + 128 >= g.nz_lo && c + 128 < g.nz_hi)) v2 = *reinterpret_cast<const u32x4*>(src + 2048);
    if (kLoadAll || (c + 192 >= g.nz_lo && c + 192 < g.nz_hi)) v3 = *reinterpret_cast<const u32x4*>(src + 3072);
    const int lo = (c_first * 16) / ES;
    if (page_rows_hit(r0.rows, lo, lo + 4096 / ES, g.shift, ca.magic_cellrow) != 0ull) {
      // ~40 % of the pages: some movable's rows cross this page
      const int xy = page_load_xy(a, env0, lane);
      const PageEnv pe = page_env<ES>(a, r0.pid, env0, c_first * 16);
      if (ES == 1) {
        if (lane < 16) pal[lane] = a.pal_rgb[lane];
      } else {
        pal[lane] = __float_as_uint(a.pal_f32[lane >> 2][lane & 3]);
      }
      if (lane < 8) dirty[lane] = 0;
      for (int i = lane; i < PW_PAGE_ENTRIES / 4; i += PW_WAVE) reinterpret_cast<uint4*>(win0)[i] = make_uint4(0u, 0u, 0u, 0u);
      __syncthreads();
      page_mark<ES>(a, pe, lane, xy, win0, dirty);
      __syncthreads();
      if (dirty[0] | dirty[1] | dirty[2] | dirty[3] | dirty[4] | dirty[5] | dirty[6] | dirty[7]) {
        const int bit = lane & 31, wsel = lane >> 5;
        if ((dirty[0 + wsel] >> bit) & 1u) v0 = PAGE_CHUNK(pe, c_first + lane, win0);
        if ((dirty[2 + wsel] >> bit) & 1u) v1 = PAGE_CHUNK(pe, c_first + lane + 64, win0);
        if ((dirty[4 + wsel] >> bit) & 1u) v2 = PAGE_CHUNK(pe, c_first + lane + 128, win0);
        if ((dirty[6 + wsel] >> bit) & 1u) v3 = PAGE_CHUNK(pe, c_first + lane + 192, win0);
      }
    }
    PAGE_STORE(v0, dst);
    PAGE_STORE(v1, dst + 1024);
    PAGE_STORE(v2, dst + 2048);
    PAGE_STORE(v3, dst + 3072);
    return;
  }

  // ---- the page holds the tail of env0 (and usually the head of env0 + 1) ------------------------
  // Mostly bottom / top padding rows: same shape as above (loads in flight first, LDS work only when a
  // movable's rows reach the page).
  const int split = static_cast<int>(cpe) - c_first;  // local chunk where the next environment starts
  const bool has_second = split < 256 && env0 + 1u <= last;
  const uint32_t env1 = min(env0 + 1u, last);
  const PageRec r1 = ca.rec[env1];
  const PageGeom g1 = page_geom<ES>(a, r1);
  if (kLive == 2 && page_tail_head_padding(g, g1, c_first, split, static_cast<int>(ca.n_chunks), has_second)) return;
  if (kLive == 3) {  // neither environment's changed rows reach the page: it holds what it has to
    const uint64_t ch1 = ca.changed[env1];
    const int l0 = (c_first * 16) / ES, l1 = (-split * 16) / ES;
    if (page_rows_hit(ch0, l0, l0 + 4096 / ES, g.shift, ca.magic_cellrow) == 0ull &&
        !(has_second && page_rows_hit(ch1, l1, l1 + 4096 / ES, g1.shift, ca.magic_cellrow) != 0ull))
      return;
  }
  const int valid0 = static_cast<int>(ca.n_chunks) - c_first;  // local chunks [0, valid0) of env0 carry image bytes
  const uint8_t* src0 = ca.simg + static_cast<int64_t>(r0.pid) * ca.simg_stride + static_cast<int64_t>(c_first) * 16;
  const uint8_t* src1 = ca.simg + static_cast<int64_t>(r1.pid) * ca.simg_stride - static_cast<int64_t>(split) * 16;
  u32x4 v[4];
  bool ok[4], second[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int lc = lane + 64 * k;
    second[k] = lc >= split;
    ok[k] = second[k] ? (has_second && lc - split < static_cast<int>(ca.n_chunks)) : (lc < valid0);
    v[k] = u32x4{0u, 0u, 0u, 0u};
    const int ce = second[k] ? lc - split : c_first + lc;  // chunk inside its environment's image
    const bool nz = second[k] ? (ce >= g1.nz_lo && ce < g1.nz_hi) : (ce >= g.nz_lo && ce < g.nz_hi);
    if (ok[k] && nz) v[k] = *reinterpret_cast<const u32x4*>((second[k] ? src1 : src0) + lc * 16);
  }
  const int lo0 = (c_first * 16) / ES, lo1 = (-split * 16) / ES;  // (exact: multiples of 16, also when negative)
  const bool hit0 = page_rows_hit(r0.rows, lo0, lo0 + 4096 / ES, g.shift, ca.magic_cellrow) != 0ull;
  const bool hit1 = has_second && page_rows_hit(r1.rows, lo1, lo1 + 4096 / ES, g1.shift, ca.magic_cellrow) != 0ull;
  if (hit0 || hit1) {
    const int xy0 = page_load_xy(a, env0, lane);
    const int xy1 = page_load_xy(a, env1, lane);
    const PageEnv pe0 = page_env<ES>(a, r0.pid, env0, c_first * 16);
    const PageEnv pe1 = page_env<ES>(a, r1.pid, env0 + 1u, -split * 16);
    if (ES == 1) {
      if (lane < 16) pal[lane] = a.pal_rgb[lane];
    } else {
      pal[lane] = __float_as_uint(a.pal_f32[lane >> 2][lane & 3]);
    }
    if (lane < 8) dirty[lane] = 0;
    for (int i = lane; i < PW_PAGE_ENTRIES / 4; i += PW_WAVE) {
      reinterpret_cast<uint4*>(win0)[i] = make_uint4(0u, 0u, 0u, 0u);
      reinterpret_cast<uint4*>(win1)[i] = make_uint4(0u, 0u, 0u, 0u);
    }
    __syncthreads();
    if (hit0) page_mark<ES>(a, pe0, lane, xy0, win0, dirty);
    if (hit1) page_mark<ES>(a, pe1, lane, xy1, win1, dirty);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int lc = lane + 64 * k;
      if (ok[k] && ((dirty[lc >> 5] >> (lc & 31)) & 1u))
        v[k] = second[k] ? PAGE_CHUNK(pe1, lc - split, win1) : PAGE_CHUNK(pe0, c_first + lc, win0);
    }
  }
#pragma unroll
  for (int k = 0; k < 4; k++)
    if (ok[k]) PAGE_STORE(v[k], dst + k * 1024);
}
#undef PAGE_STORE

// host side: the instance of the page kernel for (dtype, trial launch, every page loads, live form)
template <typename T, int kTag, bool kLoadAll>
static void launch_page_form(int live_form, unsigned grid, size_t lds_pad, hipStream_t st, const RenderArgs& rp, const CopyArgs& ca) {
  if (live_form == 1) hipLaunchKernelGGL((pw_render_page_kernel<T, kTag, kLoadAll, 1>), dim3(grid), dim3(64), lds_pad, st, rp, ca);
  else if (live_form == 2) hipLaunchKernelGGL((pw_render_page_kernel<T, kTag, kLoadAll, 2>), dim3(grid), dim3(64), lds_pad, st, rp, ca);
  else if (live_form == 3) hipLaunchKernelGGL((pw_render_page_kernel<T, kTag, kLoadAll, 3>), dim3(grid), dim3(64), lds_pad, st, rp, ca);
  else hipLaunchKernelGGL((pw_render_page_kernel<T, kTag, kLoadAll, 0>), dim3(grid), dim3(64), lds_pad, st, rp, ca);
}

template <typename T>
static void launch_page(bool tuning, bool load_all, int live_form, unsigned grid, size_t lds_pad, hipStream_t st, const RenderArgs& rp,
                        const CopyArgs& ca) {
  if (tuning && load_all) launch_page_form<T, 1, true>(live_form, grid, lds_pad, st, rp, ca);
  else if (tuning) launch_page_form<T, 1, false>(live_form, grid, lds_pad, st, rp, ca);
  else if (load_all) launch_page_form<T, 0, true>(live_form, grid, lds_pad, st, rp, ca);
  else launch_page_form<T, 0, false>(live_form, grid, lds_pad, st, rp, ca);
}


// ------------------------------------------------------------------------------------
// Live pages of a batch (PW_OPT_OBS_PADDING_ONCE): the pages of an observation buffer in which the page kernel stores at
// least one chunk that is not frame padding -- the kernel's own conditions, from the puzzle ids alone.  Count per 1 024
// pages, scan of the counts, scatter: `live` comes out in ascending page order, its length in *count.
// ------------------------------------------------------------------------------------
struct LiveArgs {
  const PwPuzzleHeader* hdrs;
  const int32_t* puzzle_id;
  int32_t num_puzzles;
  int32_t batch;
  int32_t pad_h, pad_w;
  uint32_t chunks_per_env;
  uint32_t n_chunks;
  uint32_t n_pages;
  uint32_t n_blk;     // ceil(n_pages / 1024)
  uint32_t* blk;      // [n_blk] live pages per 1 024 pages, then their exclusive prefix sums
  uint32_t* live;     // [n_pages]
  uint32_t* count;
};

template <int ES>
__device__ __forceinline__ bool page_is_live(const LiveArgs& a, uint32_t page) {
  const uint32_t g0 = page * 256u, cpe = a.chunks_per_env;
  const uint32_t env0 = g0 / cpe;  // (< batch: g0 < batch * cpe)
  const int c_first = static_cast<int>(g0 - env0 * cpe);
  const PwPuzzleHeader& h0 = a.hdrs[pw_clamp_pid(a.puzzle_id[env0], a.num_puzzles)];
  const PageGeom g = page_geom_hw<ES>(a.pad_h, a.pad_w, h0.H, h0.W);
  if (c_first + 256 <= static_cast<int>(a.n_chunks)) return !page_chunks_padding(g, c_first, c_first + 256);
  const int split = static_cast<int>(cpe) - c_first;
  const uint32_t last = static_cast<uint32_t>(a.batch) - 1u;
  const bool has_second = split < 256 && env0 + 1u <= last;
  const PwPuzzleHeader& h1 = a.hdrs[pw_clamp_pid(a.puzzle_id[min(env0 + 1u, last)], a.num_puzzles)];
  const PageGeom g1 = page_geom_hw<ES>(a.pad_h, a.pad_w, h1.H, h1.W);
  return !page_tail_head_padding(g, g1, c_first, split, static_cast<int>(a.n_chunks), has_second);
}

// thread t of workgroup b looks at pages 1024 b + 4 t .. + 3: bit k of the result = page k is live
template <int ES>
__device__ __forceinline__ uint32_t live_flags4(const LiveArgs& a) {
  const uint32_t p0 = blockIdx.x * 1024u + threadIdx.x * 4u;
  uint32_t f = 0u;
#pragma unroll
  for (uint32_t k = 0; k < 4u; k++)
    if (p0 + k < a.n_pages && page_is_live<ES>(a, p0 + k)) f |= 1u << k;
  return f;
}

template <int ES>
__global__ __launch_bounds__(256) void pw_live_count_kernel(LiveArgs a) {
  __shared__ uint32_t total;
  if (threadIdx.x == 0) total = 0u;
  __syncthreads();
  const uint32_t n = __popc(live_flags4<ES>(a));
  if (n) atomicAdd(&total, n);
  __syncthreads();
  if (threadIdx.x == 0) a.blk[blockIdx.x] = total;
}

// one workgroup: blk[] -> exclusive prefix sums, *count = the sum
__global__ __launch_bounds__(1024) void pw_live_scan_kernel(LiveArgs a) {
  __shared__ uint32_t buf[1024];
  __shared__ uint32_t carry;
  const uint32_t t = threadIdx.x;
  if (t == 0) carry = 0u;
  __syncthreads();
  for (uint32_t base = 0; base < a.n_blk; base += 1024u) {
    const uint32_t i = base + t;
    const uint32_t v = i < a.n_blk ? a.blk[i] : 0u;
    buf[t] = v;
    __syncthreads();
    for (uint32_t d = 1; d < 1024u; d <<= 1) {
      const uint32_t add = t >= d ? buf[t - d] : 0u;
      __syncthreads();
      buf[t] += add;
      __syncthreads();
    }
    const uint32_t c = carry;
    if (i < a.n_blk) a.blk[i] = c + buf[t] - v;
    __syncthreads();
    if (t == 1023u) carry = c + buf[1023];
    __syncthreads();
  }
  if (t == 0) *a.count = carry;
}

template <int ES>
__global__ __launch_bounds__(256) void pw_live_fill_kernel(LiveArgs a) {
  __shared__ uint32_t buf[256];
  const uint32_t t = threadIdx.x;
  const uint32_t f = live_flags4<ES>(a);
  const uint32_t n = __popc(f);
  buf[t] = n;
  __syncthreads();
  for (uint32_t d = 1; d < 256u; d <<= 1) {
    const uint32_t add = t >= d ? buf[t - d] : 0u;
    __syncthreads();
    buf[t] += add;
    __syncthreads();
  }
  uint32_t at = a.blk[blockIdx.x] + buf[t] - n;  // (< the sum of all counts <= n_pages)
  const uint32_t p0 = blockIdx.x * 1024u + t * 4u;
#pragma unroll
  for (uint32_t k = 0; k < 4u; k++)
    if ((f >> k) & 1u) a.live[at++] = p0 + k;
}

// ------------------------------------------------------------------------------------
// Row-page render: the page-ordered kernel for every other frame whose pixel rows are at least 512 bytes
// (e.g. the reference's default float32 / ppc 20 observation, uint8 at ppc 8 .. 20).
//
// With ppc > 3 a cell row is ppc pixel rows of which only three are different (the zones [0, bw) | middle |
// [ppc - bw, ppc), puzzle.py:614-638).  Per engine and puzzle a *static row table* keeps those 3 H pixel rows of
// the static layers plus one all-zero row for the frame padding (1.5 MB instead of the 10.3 MB image at float32 /
// ppc 20: L2 / MALL resident, and the ppc consecutive rows of a frame that share a source row are L2 hits).  One
// single-wavefront workgroup per 4 KiB page, in the page orders of the ppc-3 kernel: every 16-byte chunk of the
// page is one 16-byte load from its source row; only in pages that meet a movable's rows (page record) the wave
// builds an LDS window of the zone entries under the movables (atomicMax in painter order) and recomputes the
// chunks they touch, pixel by pixel.  Every byte is written once, non-temporally.
//   kAligned: pixel rows are whole chunks (row bytes a multiple of 16): aligned loads, cheap index arithmetic.
//   otherwise (e.g. uint8, ppc 20, 42 cells: 2 520-byte rows): byte-granular source addresses (the hardware
//   takes unaligned 16-byte global loads) and, for the one chunk per pixel row that straddles two rows, a second
//   load and a byte blend.
// ------------------------------------------------------------------------------------
#define PW_ROWPAGE_ROWS 10  // pixel rows a page can touch (rows are >= 512 bytes)

struct RowPageArgs {
  const uint8_t* srow;      // static row tables: puzzle p, source row r at srow + p * srow_stride + 16 + r * pitch
  int64_t srow_stride;
  uint32_t pitch;           // bytes between source rows: row bytes rounded up to 16, + 16 (reads past either end of a row
                            // stay inside the table)
  uint32_t zero_row;        // index of the all-zero row (frame padding, bytes beyond the image)
  const PageRec* rec;
  uint32_t chunks_per_env;  // env stride / 16
  uint32_t n_chunks;        // 16-byte chunks of one observation (the last one may be partial)
  float inv_cpe;
  uint32_t row_bytes;
  uint32_t cpr;             // kAligned: chunks per pixel row
  uint32_t magic_cpr;       // kAligned: ceil(2^32 / cpr)
  uint64_t magic_row;       // otherwise: ceil(2^64 / row_bytes)
  uint32_t magic_ppc;       // ceil(2^32 / ppc)
  uint32_t n_pages, order, run_log2;
};

struct StaticRowsArgs {
  const PwPuzzleHeader* hdrs;
  const uint16_t* estat;
  const uint32_t* estat_off;
  uint8_t* out;
  int64_t stride;
  int32_t pad_w, ppc, bw, pitch;
  uint32_t pal_rgb[16];
  float pal_f32[16][4];
};

// builds the static row tables once per engine (into zeroed memory): block (zone row, puzzle), thread = pixel
template <typename T>
__global__ __launch_bounds__(256) void pw_static_rows_kernel(StaticRowsArgs a) {
  const int pid = blockIdx.y, zr = blockIdx.x;
  const PwPuzzleHeader& h = a.hdrs[pid];
  if (zr >= 3 * h.H) return;
  const int cy = zr / 3, zy = zr - 3 * cy, W = h.W;
  const uint16_t* E = reinterpret_cast<const uint16_t*>(reinterpret_cast<const uint8_t*>(a.estat) + a.estat_off[pid]);
  const int wpx = a.pad_w * a.ppc, padx = (wpx - W * a.ppc) / 2;
  T* row = reinterpret_cast<T*>(a.out + static_cast<int64_t>(pid) * a.stride + 16 + static_cast<int64_t>(zr) * a.pitch);
  for (int X = threadIdx.x; X < wpx; X += blockDim.x) {
    const int xp = X - padx;
    uint32_t col = PW_C_PAD;
    if (static_cast<unsigned>(xp) < static_cast<unsigned>(W * a.ppc)) {
      const int cx = xp / a.ppc, sx = xp - cx * a.ppc;
      const int zx = sx < a.bw ? 0 : (sx >= a.ppc - a.bw ? 2 : 1);
      col = (E[(3 * cy + zy) * W + cx] >> (4 * zx)) & 15u;
    }
    for (int c = 0; c < 3; c++) {
      if (sizeof(T) == 1) row[3 * X + c] = static_cast<T>((a.pal_rgb[col] >> (8 * c)) & 0xffu);
      else row[3 * X + c] = static_cast<T>(a.pal_f32[col][c]);
    }
  }
}

// one environment's share of a page (workgroup-uniform)
struct RowSeg {
  int pid, H, W;
  uint64_t rows;
  int c_base;        // chunk index inside the environment's image of the page's local chunk 0 (negative for the second)
  int lc_lo, lc_hi;  // local chunks [lc_lo, lc_hi) of the page belong to this environment's image
  int pady, padx;    // pixels
  int Y0, Y1;        // first / last pixel row the segment's chunks touch
  const uint8_t* tab;  // the puzzle's static row table (source row 0)
};

typedef pw_u32x4 __attribute__((aligned(1))) pw_u32x4_unaligned;

// pixel row of chunk c of an image, and the byte offset of the chunk inside that row
template <bool kAligned>
__device__ __forceinline__ void rowpage_locate(const RowPageArgs& ra, int c, int& Y, int& jb) {
  if (kAligned) {
    Y = static_cast<int>(__umulhi(static_cast<uint32_t>(c), ra.magic_cpr));
    jb = (c - Y * static_cast<int>(ra.cpr)) * 16;
  } else {
    const uint32_t b0 = static_cast<uint32_t>(c) * 16u;
    Y = static_cast<int>(__umul64hi(static_cast<uint64_t>(b0), ra.magic_row));
    jb = static_cast<int>(b0 - static_cast<uint32_t>(Y) * ra.row_bytes);
  }
}

// source row of pixel row Y of a segment: the puzzle's zone row, or the zero row outside the puzzle
__device__ __forceinline__ const uint8_t* rowpage_source(const RowPageArgs& ra, const RowSeg& g, int Y, int ppc, int bw) {
  const int yp = Y - g.pady;
  uint32_t r = ra.zero_row;
  if (static_cast<unsigned>(yp) < static_cast<unsigned>(g.H * ppc)) {
    const int cy = static_cast<int>(__umulhi(static_cast<uint32_t>(yp), ra.magic_ppc));
    const int sy = yp - cy * ppc;
    r = static_cast<uint32_t>(3 * cy + (sy < bw ? 0 : (sy >= ppc - bw ? 2 : 1)));
  }
  return g.tab + static_cast<int64_t>(r) * ra.pitch;
}

template <typename T, bool kAligned, int kTag = 0>
__global__ __launch_bounds__(64) void pw_render_rowpage_kernel(RenderArgs a, RowPageArgs ra) {
  typedef pw_u32x4 u32x4;
  constexpr int ES = static_cast<int>(sizeof(T));
  constexpr int kPix = ES == 1 ? 7 : 2;  // pixels a 16-byte chunk can touch
  __shared__ uint32_t pal[ES == 1 ? 16 : 64];
  __shared__ uint32_t dirty[8];
  __shared__ uint32_t win[2][PW_ROWPAGE_ROWS][64];  // [segment][pixel row of the page][cell column]
  const int lane = threadIdx.x;

  uint32_t page = blockIdx.x;
  if (ra.order == 1u) {
    const uint32_t pl = 3u - ra.run_log2, parts = 1u << pl, k = page & 7u, j = page >> 3;
    const uint32_t per = ((ra.n_pages + 7u) >> 3) << ra.run_log2;
    page = (k & (parts - 1u)) * per + ((j << ra.run_log2) | (k >> pl));
  } else if (ra.order == 2u) {
    const uint32_t sb = ra.run_log2, j = page >> 3, k = page & 7u;
    page = ((((j >> sb) << 3) + k) << sb) | (j & ((1u << sb) - 1u));
  }
  if (page >= ra.n_pages) return;
  const uint32_t g0 = page * 256u;
  const uint32_t cpe = ra.chunks_per_env;
  uint32_t env0 = static_cast<uint32_t>(static_cast<float>(g0) * ra.inv_cpe);
  {
    const int rr = static_cast<int>(g0 - env0 * cpe);
    if (rr < 0) env0 -= 1u;
    else if (rr >= static_cast<int>(cpe)) env0 += 1u;
  }
  env0 = __builtin_amdgcn_readfirstlane(env0);
  const uint32_t last = static_cast<uint32_t>(a.batch) - 1u;
  const int c_first = static_cast<int>(g0 - env0 * cpe);
  uint8_t* dst = a.obs + static_cast<int64_t>(g0) * 16 + lane * 16;
  const int ppc = a.ppc, bw = a.bw, n_chunks = static_cast<int>(ra.n_chunks), RB = static_cast<int>(ra.row_bytes);
  const int wpx = a.pad_w * ppc;
  const int split = static_cast<int>(cpe) - c_first;  // local chunk where the next environment starts
  const int nseg = (split < 256 && env0 < last) ? 2 : 1;

  RowSeg seg[2];
#pragma unroll
  for (int s = 0; s < 2; s++) {
    const uint32_t env = min(env0 + static_cast<uint32_t>(s), last);
    const PageRec r = ra.rec[env];
    RowSeg& g = seg[s];
    g.pid = r.pid;
    g.H = r.H;
    g.W = r.W;
    g.rows = r.rows;
    g.c_base = s == 0 ? c_first : -split;
    g.lc_lo = s == 0 ? 0 : split;
    g.lc_hi = s == 0 ? min(256, n_chunks - c_first) : min(256, split + n_chunks);
    if (s >= nseg) g.lc_hi = g.lc_lo;
    g.pady = (a.pad_h - g.H) * ppc / 2;
    g.padx = (a.pad_w - g.W) * ppc / 2;
    g.tab = ra.srow + static_cast<int64_t>(g.pid) * ra.srow_stride + 16;
    int jb;
    rowpage_locate<kAligned>(ra, max(g.c_base + g.lc_lo, 0), g.Y0, jb);
    rowpage_locate<kAligned>(ra, max(g.c_base + g.lc_hi - 1, 0), g.Y1, jb);
    if (!kAligned && jb + 16 > RB) g.Y1 += 1;  // the segment's last chunk reaches into the next pixel row
  }

  // ---- copy pass: every chunk from its source row (the zero row in the frame padding) --------------------
  u32x4 v[4];
  bool ok[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int lc = lane + 64 * k;
    const RowSeg& g = lc >= split ? seg[1] : seg[0];
    ok[k] = lc >= g.lc_lo && lc < g.lc_hi;
    v[k] = u32x4{0u, 0u, 0u, 0u};
    if (ok[k]) {
      int Y, jb;
      rowpage_locate<kAligned>(ra, g.c_base + lc, Y, jb);
      const uint8_t* src = rowpage_source(ra, g, Y, ppc, bw) + jb;
      if (kAligned) {
        v[k] = *reinterpret_cast<const u32x4*>(src);
      } else {
        v[k] = *reinterpret_cast<const pw_u32x4_unaligned*>(src);
        const int kk = RB - jb;  // bytes of this chunk that belong to row Y
        if (kk < 16) {           // one chunk per pixel row: the rest comes from the start of row Y + 1
          const u32x4 w = *reinterpret_cast<const pw_u32x4_unaligned*>(rowpage_source(ra, g, Y + 1, ppc, bw) - kk);
#pragma unroll
          for (int d = 0; d < 4; d++) {
            const int nb = kk - 4 * d;  // bytes of dword d that come from row Y
            const uint32_t m = nb >= 4 ? 0xFFFFFFFFu : (nb <= 0 ? 0u : ((1u << (8 * nb)) - 1u));
            v[k][d] = (v[k][d] & m) | (w[d] & ~m);
          }
        }
      }
    }
  }
  // cell rows the page's pixel rows belong to, per segment (wave-uniform): do any of them carry a movable?
  uint64_t hit_rows[2] = {0ull, 0ull};
  bool any_hit = false;
#pragma unroll
  for (int s = 0; s < 2; s++) {
    const RowSeg& g = seg[s];
    if (g.lc_hi > g.lc_lo) {
      const int Ya = g.Y0 - g.pady, Yb = g.Y1 - g.pady;
      if (Yb >= 0 && Ya < g.H * ppc) {
        const int ca = static_cast<int>(__umulhi(static_cast<uint32_t>(max(Ya, 0)), ra.magic_ppc));
        const int cb = min(static_cast<int>(__umulhi(static_cast<uint32_t>(Yb), ra.magic_ppc)), g.H - 1);
        const uint64_t upto = cb >= 63 ? ~0ull : ((2ull << cb) - 1ull);
        hit_rows[s] = g.rows & upto & (~0ull << ca);
      }
    }
    any_hit = any_hit || hit_rows[s] != 0ull;
  }

  if (any_hit) {
    // ---- movables reach into the page: entry window + dirty chunks ---------------------------------------
    if (ES == 1) {
      if (lane < 16) pal[lane] = a.pal_rgb[lane];
    } else {
      pal[lane] = __float_as_uint(a.pal_f32[lane >> 2][lane & 3]);
    }
    if (lane < 8) dirty[lane] = 0;
#pragma unroll
    for (int s = 0; s < 2; s++) {  // only the window rows this page uses (lane = cell column)
      if (hit_rows[s] == 0ull) continue;
      for (int r = 0; r <= seg[s].Y1 - seg[s].Y0; r++) win[s][r][lane] = 0u;
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < 2; s++) {
      const RowSeg& g = seg[s];
      if (hit_rows[s] == 0ull) continue;
      const uint32_t env = min(env0 + static_cast<uint32_t>(s), last);
      const int xy = page_load_xy(a, env, lane);
      const PwPuzzleHeader* h = a.hdrs + g.pid;
      const uint16_t* E = reinterpret_cast<const uint16_t*>(reinterpret_cast<const uint8_t*>(a.estat) + a.estat_off[g.pid]);
      const uint32_t* mcells = reinterpret_cast<const uint32_t*>(a.blob + h->base + h->off_mcells);
      const int n_mcells = static_cast<int>(h->n_mcells), G = h->G;
      for (int m0 = 0; m0 < n_mcells; m0 += PW_WAVE) {
        const int m = m0 + lane;
        const uint32_t c = m < n_mcells ? mcells[m] : 0u;
        const int obj = c >> 24;
        const int p = __shfl(xy, obj, PW_WAVE);
        const int x = static_cast<int8_t>(p & 0xff) + static_cast<int>(c & 0xff);
        const int y = static_cast<int8_t>((p >> 8) & 0xff) + static_cast<int>((c >> 8) & 0xff);
        if (m >= n_mcells || static_cast<unsigned>(x) >= static_cast<unsigned>(g.W) ||
            static_cast<unsigned>(y) >= static_cast<unsigned>(g.H))
          continue;
        // pixel rows of the cell inside the segment's rows [Y0, Y1]
        const int Ya = max(g.pady + y * ppc, g.Y0), Yb = min(g.pady + (y + 1) * ppc - 1, g.Y1);
        if (Ya > Yb) continue;
        const uint32_t kind = obj == 0 ? 3u : (obj <= G ? 4u : 5u);
        const uint32_t om = (c >> 16) & 0xffu;
        // bytes of the cell inside a pixel row
        const int b_lo = (g.padx + x * ppc) * 3 * ES, b_hi = (g.padx + (x + 1) * ppc) * 3 * ES - 1;
        for (int Y = Ya; Y <= Yb; Y++) {
          const int sy = Y - g.pady - y * ppc;
          const int zy = sy < bw ? 0 : (sy >= ppc - bw ? 2 : 1);
          const uint32_t e = pw_zone_entry(kind, pw_zone_border_bits(om, zy), pw_entry_goal_bits(E[(3 * y + zy) * g.W + x]));
          atomicMax(&win[s][Y - g.Y0][x], (static_cast<uint32_t>(obj + 1) << 12) | e);
          const int base = Y * RB;  // byte offset of the pixel row inside the image
          const int l0 = max(((base + b_lo) >> 4) - g.c_base, g.lc_lo), l1 = min(((base + b_hi) >> 4) - g.c_base, g.lc_hi - 1);
          for (int l = l0; l <= l1; l++) atomicOr(&dirty[l >> 5], 1u << (l & 31));
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int lc = lane + 64 * k;
      if (!ok[k] || !((dirty[lc >> 5] >> (lc & 31)) & 1u)) continue;
      const int s = lc >= split ? 1 : 0;
      const RowSeg& g = s ? seg[1] : seg[0];
      const uint16_t* E = reinterpret_cast<const uint16_t*>(reinterpret_cast<const uint8_t*>(a.estat) + a.estat_off[g.pid]);
      int Y, jb;
      rowpage_locate<kAligned>(ra, g.c_base + lc, Y, jb);
      const int elem0 = jb / ES;  // first channel of the chunk inside pixel row Y
      int X = elem0 / 3;
      const int ch0 = elem0 - 3 * X;
      const int own_w = g.W * ppc, own_h = g.H * ppc;
      // per pixel row: zone row of the static table / the window, valid only inside the puzzle's rows
      int yp = Y - g.pady;
      bool in_row = static_cast<unsigned>(yp) < static_cast<unsigned>(own_h);
      int cy = in_row ? static_cast<int>(__umulhi(static_cast<uint32_t>(yp), ra.magic_ppc)) : 0;
      int sy = yp - cy * ppc;
      int zy = sy < bw ? 0 : (sy >= ppc - bw ? 2 : 1);
      const uint32_t* wrow = win[s][min(max(Y - g.Y0, 0), PW_ROWPAGE_ROWS - 1)];
      const uint16_t* erow = E + (3 * cy + zy) * g.W;
      int xp = X - g.padx;
      int cx = xp >= 0 ? static_cast<int>(__umulhi(static_cast<uint32_t>(xp), ra.magic_ppc)) : 0;
      int sx = xp - cx * ppc;  // negative while left of the puzzle
      uint32_t rgb[kPix];
#pragma unroll
      for (int q = 0; q < kPix; q++) {
        uint32_t col = PW_C_PAD;
        if (in_row && static_cast<unsigned>(xp) < static_cast<unsigned>(own_w)) {
          const int zx = sx < bw ? 0 : (sx >= ppc - bw ? 2 : 1);
          const uint32_t w = wrow[cx];
          const uint32_t e = w ? (w & 0xFFFu) : static_cast<uint32_t>(erow[cx]);
          col = (e >> (4 * zx)) & 15u;
        }
        rgb[q] = ES == 1 ? pal[col] : col;
        xp++;
        if (++sx == ppc) {  // (sx < 0 left of the puzzle reaches 0 together with xp)
          sx = 0;
          cx++;
        }
        if (!kAligned && ++X == wpx) {  // the chunk runs into the next pixel row
          X = 0;
          Y++;
          yp = Y - g.pady;
          in_row = static_cast<unsigned>(yp) < static_cast<unsigned>(own_h);
          cy = in_row ? static_cast<int>(__umulhi(static_cast<uint32_t>(yp), ra.magic_ppc)) : 0;
          sy = yp - cy * ppc;
          zy = sy < bw ? 0 : (sy >= ppc - bw ? 2 : 1);
          wrow = win[s][min(max(Y - g.Y0, 0), PW_ROWPAGE_ROWS - 1)];
          erow = E + (3 * cy + zy) * g.W;
          xp = -g.padx;
          cx = 0;
          sx = -g.padx;
        }
      }
      union {
        u32x4 v;
        uint32_t u32[4];
        float f32[4];
      } o;
      if (ES == 1) {
        const uint32_t d0 = rgb[0] | (rgb[1] << 24);
        const uint32_t d1 = (rgb[1] >> 8) | (rgb[2] << 16);
        const uint32_t d2 = (rgb[2] >> 16) | (rgb[3 < kPix ? 3 : 0] << 8);
        const uint32_t d3 = rgb[4 < kPix ? 4 : 0] | (rgb[5 < kPix ? 5 : 0] << 24);
        const uint32_t d4 = (rgb[5 < kPix ? 5 : 0] >> 8) | (rgb[6 < kPix ? 6 : 0] << 16);
        const uint32_t bs = static_cast<uint32_t>(ch0);
        o.u32[0] = __builtin_amdgcn_alignbyte(d1, d0, bs);
        o.u32[1] = __builtin_amdgcn_alignbyte(d2, d1, bs);
        o.u32[2] = __builtin_amdgcn_alignbyte(d3, d2, bs);
        o.u32[3] = __builtin_amdgcn_alignbyte(d4, d3, bs);
      } else {
        const float* palf = reinterpret_cast<const float*>(pal);
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const int e = ch0 + q;  // element q belongs to pixel e / 3, channel e % 3
          o.f32[q] = palf[rgb[e >= 3 ? 1 : 0] * 4 + (e >= 3 ? e - 3 : e)];
        }
      }
      v[k] = o.v;
    }
  }
#pragma unroll
  for (int k = 0; k < 4; k++)
    if (ok[k]) __builtin_nontemporal_store(v[k], reinterpret_cast<u32x4*>(dst + k * 1024));
}

// ------------------------------------------------------------------------------------
// Incremental render (uint8, ppc 3; pw_step_render_delta): the observation buffer already holds the
// observation of the state BEFORE the step, so only the pixel rows swept by the objects that moved
// (their old and new cells) change -- on the Level-1 mix ~5 % of an image, nothing at all for a
// blocked move.  One wavefront per environment reads the row interval the step kernel left in
// `dirty`, and rewrites that byte range with the page kernel's machinery (static image + LDS entry
// window over ALL movables that reach into the segment), 4 KiB at a time.  Environments that were
// reset carry the full interval and are redrawn completely.
// ------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(64) void pw_render_delta_kernel(RenderArgs a, CopyArgs ca, const uint32_t* dirty_rows) {
  typedef pw_u32x4 u32x4;
  constexpr int ES = static_cast<int>(sizeof(T));
  __shared__ uint32_t pal[ES == 1 ? 16 : 64];
  __shared__ uint32_t dirty[8];
  __shared__ __align__(16) uint32_t win0[PW_PAGE_ENTRIES];
  const int lane = threadIdx.x;
  const uint32_t env = blockIdx.x;
  // first level of loads, all independent: the record (rows + puzzle height), positions, puzzle id
  const uint32_t d = dirty_rows[env];
  const int xy = page_load_xy(a, env, lane);
  const int pid = pw_clamp_pid(a.puzzle_id[env], a.num_puzzles);
  const int ylo = static_cast<int>(d & 0xffu), yhi_raw = static_cast<int>((d >> 8) & 0xffu);
  if (yhi_raw <= ylo) return;  // nothing moved: the buffer is already right
  const int H = static_cast<int>(d >> 16);  // from the record: the chunk range needs no header load
  const int pady = (a.pad_h - H) * 3 / 2;
  const int row_bytes = 9 * a.pad_w * ES;
  const int yhi = min(yhi_raw, H);
  // a reset environment (interval 0 .. PW_MAX_DIM) may have changed puzzle: the whole frame, padding included
  const bool whole = yhi_raw >= PW_MAX_DIM;
  const int c_lo = whole ? 0 : ((pady + 3 * ylo) * row_bytes) >> 4;
  const int c_hi = whole ? static_cast<int>(ca.n_chunks)
                         : min(((pady + 3 * yhi) * row_bytes + 15) >> 4, static_cast<int>(ca.n_chunks));
  uint8_t* dst = a.obs + static_cast<int64_t>(env) * a.env_stride;
  const uint8_t* src = ca.simg + static_cast<int64_t>(pid) * ca.simg_stride;
  if (ES == 1) {
    if (lane < 16) pal[lane] = a.pal_rgb[lane];
  } else {
    pal[lane] = __float_as_uint(a.pal_f32[lane >> 2][lane & 3]);
  }
  for (int c0 = c_lo; c0 < c_hi; c0 += 256) {
    const PageEnv pe = page_env<ES>(a, pid, env, c0 * 16);
    u32x4 v[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int c = c0 + lane + 64 * k;
      v[k] = u32x4{0u, 0u, 0u, 0u};
      if (c < c_hi) v[k] = *reinterpret_cast<const u32x4*>(src + static_cast<int64_t>(c) * 16);
    }
    __syncthreads();  // the previous segment's window is no longer read
    if (page_prefilter<ES>(a, pe, lane, xy)) {
      if (lane < 8) dirty[lane] = 0;
      for (int i = lane; i < PW_PAGE_ENTRIES / 4; i += PW_WAVE) reinterpret_cast<uint4*>(win0)[i] = make_uint4(0u, 0u, 0u, 0u);
      __syncthreads();
      page_mark<ES>(a, pe, lane, xy, win0, dirty);
      __syncthreads();
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int lc = lane + 64 * k;
        if (c0 + lc < c_hi && ((dirty[lc >> 5] >> (lc & 31)) & 1u)) v[k] = PAGE_CHUNK(pe, c0 + lc, win0);
      }
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int c = c0 + lane + 64 * k;
      if (c < c_hi) *reinterpret_cast<u32x4*>(dst + static_cast<int64_t>(c) * 16) = v[k];
    }
  }
}

// ------------------------------------------------------------------------------------
// Changed-row render (ppc 3; uint8 and float32; launch_render's live_form 4, pw_engine_set_obs_changed_rows): the
// environment-major form of the changed-page launch.  The retained buffer shows PwRetained::d_shown, the record writers of
// this call left the grid rows in which the new state differs from it in CopyArgs::changed -- so per environment only the pixel
// rows of those cell rows are rewritten: every run of set bits [r0, r1) is one chunk range (pw_rows_chunk_range), walked
// 256 chunks per pass with the delta kernel's body.  The unit of work is the environment, not the page: ceil(batch / 4)
// workgroups of four wavefronts, wavefront w of workgroup b owns environment 4 b + w, with an LDS entry window of its own.
// On the Level-1 mix 18 % of the wavefronts return after three loads, 82 % walk one run, 89 % of the runs are one pass.
//
// The wavefronts of a workgroup differ in their pass counts and return early, so behind the one barrier that every thread
// reaches (the shared palette) each orders its own LDS traffic at wavefront scope: the LDS executes the operations of one
// wavefront in order, the fences only keep the compiler from moving them.
//   kNT: non-temporal stores (the page kernel's policy) instead of plain ones (the delta kernel's); fixed at compile time,
//   see PAGE_STORE above.
// ------------------------------------------------------------------------------------
__device__ __forceinline__ void rows_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// moves the 4 KiB window of a PageEnv to byte offset lo of the same environment's image (page_env's arithmetic)
template <int ES>
__device__ __forceinline__ void page_env_move(PageEnv& pe, int lo) {
  pe.lo = lo;
  const int t = (lo >= 0 ? lo / ES : -((-lo) / ES)) - pe.shift_bytes;
  pe.q_lo = (t >= 0 ? t / 9 : -((-t + 8) / 9)) - 2;
}

#define PW_ROWS_WAVES 4  // environments (wavefronts) per workgroup
// which store policy the changed-row launch runs with (kNT): 1 non-temporal, 0 plain; both measured, profiles/obs_rows.txt section 2
#ifndef PW_ROWS_STORE_NT
#define PW_ROWS_STORE_NT 1
#endif

template <typename T, bool kNT>
__global__ __launch_bounds__(64 * PW_ROWS_WAVES) void pw_render_rows_kernel(RenderArgs a, CopyArgs ca) {
  typedef pw_u32x4 u32x4;
  constexpr int ES = static_cast<int>(sizeof(T));
  __shared__ uint32_t pal[ES == 1 ? 16 : 64];
  __shared__ uint32_t dirty_w[PW_ROWS_WAVES][8];
  __shared__ __align__(16) uint32_t win_w[PW_ROWS_WAVES][PW_PAGE_ENTRIES];
  const int tid = threadIdx.x;
  const int lane = tid & (PW_WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const uint32_t env_raw = blockIdx.x * static_cast<uint32_t>(PW_ROWS_WAVES) + static_cast<uint32_t>(wave);
  // (the wavefronts behind the batch in the last workgroup load the last environment's words and return behind the barrier)
  const uint32_t env = min(env_raw, static_cast<uint32_t>(a.batch) - 1u);
  // first level of loads, all from the environment index alone: the changed rows, the record, the positions
  const uint64_t ch = ca.changed[env];
  const PageRec r = ca.rec[env];
  const int xy = page_load_xy(a, env, lane);
  if (ES == 1) {
    if (tid < 16) pal[tid] = a.pal_rgb[tid];
  } else {
    if (tid < 64) pal[tid] = __float_as_uint(a.pal_f32[tid >> 2][tid & 3]);
  }
  __syncthreads();  // the only workgroup barrier: nothing has returned yet
  if (env_raw >= static_cast<uint32_t>(a.batch)) return;
  const int H = r.H, W = r.W;
  uint64_t m = ch & (H >= 64 ? ~0ull : ((1ull << H) - 1ull));  // (a mask of all ones -- a y outside 0 .. 63 -- is rows [0, H))
  if (m == 0ull) return;  // nothing this environment shows has changed: no other load, no store

  uint32_t* win = win_w[wave];
  uint32_t* dirty = dirty_w[wave];
  const PageGeom g = page_geom_hw<ES>(a.pad_h, a.pad_w, H, W);
  uint8_t* dst = a.obs + static_cast<int64_t>(env) * a.env_stride;
  const uint8_t* src = ca.simg + static_cast<int64_t>(r.pid) * ca.simg_stride;
  PageEnv pe = page_env<ES>(a, r.pid, env, 0);
  while (m != 0ull) {
    // the lowest run of set bits [r0, r1)
    const int r0 = __builtin_ctzll(m);
    const uint64_t t = ~(m >> r0);
    const int r1 = t != 0ull ? r0 + __builtin_ctzll(t) : 64;
    m = r1 >= 64 ? 0ull : (m & (~0ull << r1));
    const PwChunkRange cr = pw_rows_chunk_range(a.pad_h, a.pad_w, H, W, ES, r0, r1, static_cast<int32_t>(ca.n_chunks));
    for (int c0 = cr.lo; c0 < cr.hi; c0 += 256) {
      page_env_move<ES>(pe, c0 * 16);
      u32x4 v[4];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int c = c0 + lane + 64 * k;
        v[k] = u32x4{0u, 0u, 0u, 0u};
        if (c < cr.hi && c >= g.nz_lo && c < g.nz_hi) v[k] = *reinterpret_cast<const u32x4*>(src + static_cast<int64_t>(c) * 16);
      }
      rows_wave_sync();  // the previous pass's window is no longer read
      if (page_prefilter<ES>(a, pe, lane, xy)) {
        if (lane < 8) dirty[lane] = 0;
        for (int i = lane; i < PW_PAGE_ENTRIES / 4; i += PW_WAVE) reinterpret_cast<uint4*>(win)[i] = make_uint4(0u, 0u, 0u, 0u);
        rows_wave_sync();
        page_mark<ES>(a, pe, lane, xy, win, dirty);
        rows_wave_sync();
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const int lc = lane + 64 * k;
          if (c0 + lc < cr.hi && ((dirty[lc >> 5] >> (lc & 31)) & 1u)) v[k] = PAGE_CHUNK(pe, c0 + lc, win);
        }
      }
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int c = c0 + lane + 64 * k;
        if (c < cr.hi) {
          u32x4* p = reinterpret_cast<u32x4*>(dst + static_cast<int64_t>(c) * 16);
          if (kNT) __builtin_nontemporal_store(v[k], p);
          else *p = v[k];
        }
      }
    }
  }
}

#undef PAGE_CHUNK

// Generic path: any pixels_per_cell / border_width, uint8 or float32 elements.
// One thread produces 16 bytes (16 uint8 or 4 float32 channel values) per iteration.
template <typename T>
__device__ __forceinline__ void render_generic_body(const RenderArgs& a, const int16_t* lds_xy = nullptr, const uint32_t* lds_rows = nullptr,
                                                    const uint32_t* lds_cols = nullptr) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int tid = threadIdx.x;
  const int bands = a.bands > 1 ? a.bands : 1;
  const int env = static_cast<int>(blockIdx.x) / bands;
  const int band = static_cast<int>(blockIdx.x) - env * bands;
  const int n_chunks_all = (a.obs_bytes + 15) >> 4;
  // incremental redraw (pw_step_render_delta): only the cell rows the step changed, nothing for a blocked
  // move, everything (frame padding included) for an environment that was reset
  int row_lo = 0, row_hi = PW_MAX_DIM;
  bool whole = true;
  const bool incremental = a.dirty_rows != nullptr || lds_rows != nullptr;
  if (incremental) {
    const uint32_t d = lds_rows ? *lds_rows : a.dirty_rows[env];
    row_lo = static_cast<int>(d & 0xffu);
    row_hi = static_cast<int>((d >> 8) & 0xffu);
    if (row_hi <= row_lo) return;
    whole = row_hi >= PW_MAX_DIM;
  }
  // several workgroups per environment (bands): of a full render each takes a contiguous band of the image; of an incremental
  // redraw each takes a part of the rows that changed (a batch of one writing over PCIe: one workgroup alone reaches ~10 GB/s)
  const bool split_dirty = bands > 1 && incremental && !whole;
  const int pid = pw_clamp_pid(a.puzzle_id[env], a.num_puzzles);
  const PuzzleView pv = view_of(a.hdrs, a.blob, pid);
  // band of a full render: chunks [band_lo, band_hi) of the image and the cell rows their pixels belong to
  int band_lo = 0, band_hi = n_chunks_all;
  if (bands > 1 && !split_dirty) {
    const int cpb = (n_chunks_all + bands - 1) / bands;
    band_lo = band * cpb;
    band_hi = min(n_chunks_all, band_lo + cpb);
    if (band_lo >= band_hi) return;
    const int64_t row_b = static_cast<int64_t>(a.pad_w) * a.ppc * 3 * static_cast<int>(sizeof(T));
    const int pady_b = (a.pad_h - pv.H) * a.ppc / 2;
    const int yp0 = static_cast<int>((static_cast<int64_t>(band_lo) * 16) / row_b) - pady_b;
    const int yp1 = static_cast<int>((static_cast<int64_t>(band_hi) * 16 - 1) / row_b) - pady_b;
    whole = false;
    if (yp1 < 0 || yp0 >= pv.H * a.ppc) {
      row_lo = row_hi = 0;  // the band lies in the frame padding: no zone rows needed
    } else {
      row_lo = max(yp0, 0) / a.ppc;
      row_hi = min(yp1, pv.H * a.ppc - 1) / a.ppc + 1;
    }
  }
  const int n_entries = 3 * pv.H * pv.W;
  const RenderLds l = carve_lds(smem, ((2 * (n_entries + 3) + 15) >> 4) << 4);
  // a 16-byte chunk at the edge of the range reaches into the neighbouring pixel row: one more cell row each side
  build_zone_table(a, pv, pid, env, l, pv.W, 0, whole ? 0 : row_lo - 1, whole ? PW_MAX_DIM : row_hi + 1, lds_xy);
  const uint16_t* E = l.E;
  const uint32_t* pal = l.pal;

  constexpr int kElems = 16 / sizeof(T);
  const int ppc = a.ppc, bw = a.bw;
  const int wpx = a.pad_w * ppc;
  const int own_w = pv.W * ppc, own_h = pv.H * ppc;
  const int pady = (a.pad_h * ppc - own_h) / 2;
  const int padx = (wpx - own_w) / 2;
  const int n_chunks = (a.obs_bytes + 15) >> 4;
  uint8_t* out = a.obs + static_cast<int64_t>(env) * a.env_stride;

  // float32: the palette as exact uint8/255 values, staged next to the uint8 palette in LDS
  float* palf = reinterpret_cast<float*>(l.flag + 4);
  if (sizeof(T) == 4 && tid < 64) palf[tid] = a.pal_f32[tid >> 2][tid & 3];
  __syncthreads();
  constexpr int kPix = sizeof(T) == 1 ? 7 : 2;  // pixels a 16-byte chunk can touch
  int chunk_lo = 0, chunk_hi = n_chunks;
  if (bands > 1 && !split_dirty) {
    chunk_lo = band_lo;
    chunk_hi = band_hi;
  } else if (!whole) {
    const int64_t row_b = static_cast<int64_t>(wpx) * 3 * static_cast<int>(sizeof(T));
    chunk_lo = static_cast<int>(((pady + row_lo * ppc) * row_b) >> 4);
    chunk_hi = min(n_chunks, static_cast<int>(((pady + min(row_hi, pv.H) * ppc) * row_b + 15) >> 4));
    if (split_dirty) {  // this workgroup's part of the changed rows
      const int per = (chunk_hi - chunk_lo + bands - 1) / bands;
      chunk_lo += band * per;
      chunk_hi = min(chunk_hi, chunk_lo + per);
    }
  }
  // pw_step_render_one_kernel also hands over the cell COLUMNS the step changed: of the changed pixel rows only the chunks that touch
  // those columns are written (an agent's move: 240 of a row's 1 680 bytes at 20 pixels per cell, float32 -- the rows of a batch of
  // one cross the link).  Work item = (pixel row, k-th chunk of the row's window); chunks at a row's edge may be written twice, with
  // the same bytes (every chunk is computed whole from the zone table, which holds all columns of the rows around the change).
  const bool window = lds_cols != nullptr && split_dirty;  // (not `!whole`: a band of a FULL redraw has narrowed its rows above)
  int it = chunk_lo + tid, it_end = chunk_hi, it_stride = PW_RENDER_THREADS;
  int win_y0 = 0, win_per = 1;
  int64_t win_row_b = 0, win_x0 = 0, win_x1 = 0;
  if (window) {
    const uint32_t c = *lds_cols;
    const int col_lo = static_cast<int>(c & 0xffu), col_hi = static_cast<int>((c >> 8) & 0xffu);
    win_row_b = static_cast<int64_t>(wpx) * 3 * static_cast<int>(sizeof(T));
    win_x0 = static_cast<int64_t>(padx + col_lo * ppc) * 3 * static_cast<int>(sizeof(T));
    win_x1 = static_cast<int64_t>(padx + col_hi * ppc) * 3 * static_cast<int>(sizeof(T));
    win_y0 = pady + row_lo * ppc;
    const int y1 = pady + min(row_hi, pv.H) * ppc;
    win_per = static_cast<int>((win_x1 - win_x0 + 15) >> 4) + 1;
    it = band * PW_RENDER_THREADS + tid;
    it_end = (y1 - win_y0) * win_per;
    it_stride = bands * PW_RENDER_THREADS;
  }
  for (; it < it_end; it += it_stride) {
    int chunk = it;
    if (window) {
      const int r = it / win_per, k = it - r * win_per;
      const int64_t row0 = static_cast<int64_t>(win_y0 + r) * win_row_b;
      chunk = static_cast<int>((row0 + win_x0) >> 4) + k;
      if (static_cast<int64_t>(chunk) * 16 >= row0 + win_x1 || chunk >= n_chunks) continue;
    }
    const int elem0 = chunk * kElems;
    const int pix = elem0 / 3;
    const int ch0 = elem0 - pix * 3;  // channel of the first element
    // position of the first pixel: three divisions per chunk, then the walk below is incremental
    int Y = pix / wpx;
    int X = pix - Y * wpx;
    int yp = Y - pady, xp = X - padx;
    bool in_row = static_cast<unsigned>(yp) < static_cast<unsigned>(own_h);
    int cy = in_row ? yp / ppc : 0;
    int sy = yp - cy * ppc;
    int zy = sy < bw ? 0 : (sy >= ppc - bw ? 2 : 1);
    int cx = xp >= 0 ? xp / ppc : 0;
    int sx = xp - cx * ppc;  // negative while left of the puzzle
    uint32_t rgb[kPix];
#pragma unroll
    for (int j = 0; j < kPix; j++) {
      uint32_t col = PW_C_PAD;
      if (in_row && static_cast<unsigned>(xp) < static_cast<unsigned>(own_w)) {
        const int zx = sx < bw ? 0 : (sx >= ppc - bw ? 2 : 1);
        col = (E[(3 * cy + zy) * pv.W + cx] >> (4 * zx)) & 15u;
      }
      rgb[j] = sizeof(T) == 1 ? pal[col] : col;
      // next pixel
      xp++;
      if (++sx == ppc) {  // sx < 0 while left of the puzzle: reaches 0 together with xp
        sx = 0;
        cx++;
      }
      if (xp == wpx - padx) {  // row wrap (X == wpx)
        xp = -padx;
        cx = 0;
        sx = -padx;
        yp++;
        in_row = static_cast<unsigned>(yp) < static_cast<unsigned>(own_h);
        if (in_row && ++sy == ppc) {
          sy = 0;
          cy++;
        }
        if (yp == 0) {
          sy = 0;
          cy = 0;
        }
        zy = sy < bw ? 0 : (sy >= ppc - bw ? 2 : 1);
      }
    }
    union {
      uint4 v;
      uint32_t u32[4];
      float f32[4];
    } o;
    if (sizeof(T) == 1) {
      // 7 pixels = 21 bytes, the chunk is bytes [ch0, ch0 + 16) of them
      const uint32_t d0 = rgb[0] | (rgb[1] << 24);
      const uint32_t d1 = (rgb[1] >> 8) | (rgb[2] << 16);
      const uint32_t d2 = (rgb[2] >> 16) | (rgb[3] << 8);
      const uint32_t d3 = rgb[4] | (rgb[5] << 24);
      const uint32_t d4 = (rgb[5] >> 8) | (rgb[6 < kPix ? 6 : 0] << 16);
      const uint32_t bs = static_cast<uint32_t>(ch0);
      o.u32[0] = __builtin_amdgcn_alignbyte(d1, d0, bs);
      o.u32[1] = __builtin_amdgcn_alignbyte(d2, d1, bs);
      o.u32[2] = __builtin_amdgcn_alignbyte(d3, d2, bs);
      o.u32[3] = __builtin_amdgcn_alignbyte(d4, d3, bs);
    } else {
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int e = ch0 + k;  // element k belongs to pixel e / 3, channel e % 3
        o.f32[k] = palf[rgb[e >= 3 ? 1 : 0] * 4 + (e >= 3 ? e - 3 : e)];
      }
    }
    *reinterpret_cast<uint4*>(out + static_cast<int64_t>(chunk) * 16) = o.v;
  }
}

// pw_step_render_delta on a batch of ONE with a completion word (the gym / dm_env adapters), as ONE launch (round 6; VERDICT r5 #7).
// A step was two launches -- the step kernel, then the redraw of the rows it changed through several workgroups -- or one replay of
// their captured graph: ~8 us of host time either way and a kernel boundary on the device.  Here workgroup 0's first wavefront steps
// the environment (step_one_env: what pw_step_kernel launches), writes the state where pw_step would (the adapter's pinned host
// memory) and hands positions + changed rows to the other workgroups through device memory: a word that carries the launch's number (`seq`, never repeated);
// every workgroup then redraws its share of the rows exactly as pw_render_generic_kernel does, the last one writes the completion
// word.  (All workgroups of the launch are resident -- at most 8 -- and workgroup 0 is dispatched first: nobody waits for a
// workgroup that cannot start.)  scratch: 18 words of 8 bytes (device memory; every access an agent-scope access of its own -- the
// workgroups sit on different XCDs --, so no fence invalidates or writes back an L2).
template <typename T>
__global__ __launch_bounds__(PW_RENDER_THREADS) void pw_step_render_one_kernel(RenderArgs a, uint32_t* scratch, unsigned long long seq, int use_cols, uint8_t* host_copy) {
  __shared__ int16_t s_xy[32];
  __shared__ uint32_t s_rows, s_cols;
  const int tid = threadIdx.x, lane = tid & (PW_WAVE - 1);
  if (blockIdx.x == 0) {
    if (tid < PW_WAVE) {
      const StepArgs& st = a.step;
      const int pid = __builtin_amdgcn_readfirstlane(pw_clamp_pid(a.puzzle_id[0], a.num_puzzles));
      const PuzzleView pv = view_of(a.hdrs, a.blob, pid);
      int old = 0;
      if (lane < st.np) old = static_cast<uint16_t>(reinterpret_cast<const int16_t*>(st.pos)[lane]);
      const int was_done = __builtin_amdgcn_readfirstlane(static_cast<int>(st.term[0] | st.trunc[0]));
      const int act = __builtin_amdgcn_readfirstlane(static_cast<int>(st.actions[0]));
      int xy;
      bool legal;
      step_one_env(st, 0, lane, pv, xy, legal);
      const bool was_reset = (st.flags & PW_STEP_AUTORESET) && was_done;
      int lo = 127, hi = -1;    // cell rows swept by the moved objects, old and new position (pushed objects touch: one interval)
      int clo = 127, chi = -1;  // ... and cell columns
      if (!was_reset && act <= 3 && lane < pv.N && xy != old) {
        const int y0 = static_cast<int8_t>((old >> 8) & 0xff), y1 = static_cast<int8_t>((xy >> 8) & 0xff);
        const int x0 = static_cast<int8_t>(old & 0xff), x1 = static_cast<int8_t>(xy & 0xff);
        lo = min(y0, y1);
        hi = max(y0, y1) + pv.h->objtab[lane].h;
        clo = min(x0, x1);
        chi = max(x0, x1) + pv.h->objtab[lane].w;
      }
#pragma unroll
      for (int o = PW_WAVE / 2; o > 0; o >>= 1) {
        lo = min(lo, __shfl_xor(lo, o, PW_WAVE));
        hi = max(hi, __shfl_xor(hi, o, PW_WAVE));
        clo = min(clo, __shfl_xor(clo, o, PW_WAVE));
        chi = max(chi, __shfl_xor(chi, o, PW_WAVE));
      }
      if (was_reset) lo = 0, hi = PW_MAX_DIM;
      lo = max(lo, 0), hi = min(hi, PW_MAX_DIM);
      clo = max(clo, 0), chi = min(max(chi, clo), static_cast<int>(pv.W));
      const uint32_t rows = hi > lo ? static_cast<uint32_t>(lo | (hi << 8) | (pv.H << 16)) : 0u;
      const uint32_t cols = static_cast<uint32_t>(clo | (chi << 8));
      // hand-over: 18 words of 8 bytes, low half = payload (two positions, the rows, the columns), high half = this launch's number -- a reader
      // takes a word when it carries the number.  No flag behind the payload: that needed a wait for EVERY store of this wavefront to
      // be acknowledged first, the state it has just written into the adapter's pinned host memory included (~1 us across the link).
      const int nxt = __shfl_down(xy, 1, PW_WAVE);  // (two positions per word)
      const unsigned long long tag = (seq & 0xffffffffull) << 32;
      unsigned long long* hand = reinterpret_cast<unsigned long long*>(scratch);
      if (lane < 32 && (lane & 1) == 0)
        __hip_atomic_store(hand + (lane >> 1), tag | static_cast<uint32_t>(xy & 0xffff) | (static_cast<uint32_t>(nxt & 0xffff) << 16), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
      if (lane == 0) __hip_atomic_store(hand + 16, tag | rows, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (lane == 0) __hip_atomic_store(hand + 17, tag | cols, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (lane < 32) s_xy[lane] = static_cast<int16_t>(xy);
      if (lane == 0) s_rows = rows, s_cols = cols;
      // pw_engine_set_step_host_copy: the state arrays are DEVICE memory (this kernel reads and writes them at the speed of the
      // L2 -- with the state in the adapter's pinned host memory the reads across the link alone were ~2 us of every step) and the host
      // gets a COPY of what the step left: reward float64 | steps int32 | terminated | truncated | dgoals | pad | (x, y) int8 pairs from
      // byte 16.  Posted writes: the fence before the completion word covers them like the rows of the observation.
      if (host_copy) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (this wavefront's own stores: the loads below read what step_one_env wrote)
        if (lane == 0) {
          *reinterpret_cast<double*>(host_copy) = st.reward ? st.reward[0] : 0.0;
          *reinterpret_cast<int32_t*>(host_copy + 8) = st.steps[0];
          host_copy[12] = st.term[0];
          host_copy[13] = st.trunc[0];
          host_copy[14] = st.dgoals ? static_cast<uint8_t>(st.dgoals[0]) : 0;
        }
        if (lane < st.np) reinterpret_cast<int16_t*>(host_copy + 16)[lane] = static_cast<int16_t>(xy);
      }
    }
  } else if (tid < PW_WAVE) {
    const unsigned long long* hand = reinterpret_cast<const unsigned long long*>(scratch);
    unsigned long long w = 0ull;
    for (;;) {
      if (lane < 18) w = __hip_atomic_load(hand + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (__ballot(lane < 18 && (w >> 32) != (seq & 0xffffffffull)) == 0ull) break;
      __builtin_amdgcn_s_sleep(1);
    }
    if (lane < 16) {
      s_xy[2 * lane] = static_cast<int16_t>(w & 0xffffu);
      s_xy[2 * lane + 1] = static_cast<int16_t>((w >> 16) & 0xffffu);
    }
    if (lane == 16) s_rows = static_cast<uint32_t>(w & 0xffffffffull);
    if (lane == 17) s_cols = static_cast<uint32_t>(w & 0xffffffffull);
  }
  __syncthreads();
  render_generic_body<T>(a, s_xy, &s_rows, use_cols ? &s_cols : nullptr);
  __threadfence_system();
  __syncthreads();
  if (threadIdx.x == 0) {
    if (atomicAdd(a.signal_count, 1u) == gridDim.x - 1u) {
      __hip_atomic_store(a.signal_count, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (the next launch is behind this one in the stream)
      __hip_atomic_store(a.signal, a.signal_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

template <typename T>
__global__ __launch_bounds__(PW_RENDER_THREADS) void pw_render_generic_kernel(RenderArgs a) {
  render_generic_body<T>(a);
  if (a.signal) {  // (the step kernel before it in the stream has finished; the last workgroup of this one to get here reports)
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) {
      bool last = gridDim.x == 1;
      if (!last && atomicAdd(a.signal_count, 1u) == gridDim.x - 1u) {
        __hip_atomic_store(a.signal_count, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (the next launch is behind this one in the stream)
        last = true;
      }
      if (last) __hip_atomic_store(a.signal, a.signal_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

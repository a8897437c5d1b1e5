// pw_generate.inc -- level-0 puzzle generation, dihedral transforms and the puzzle packer ON THE DEVICE
// (SURVEY 8-f4).  Part of the single translation unit pw_kernels.hip.
//
// The reference generates training puzzles as text (python3/src/pushworld/generate.py:28-259), transforms
// text (transform.py:21-48) and parses text in every constructor (puzzle.py:130-311).  Here a puzzle travels as
// a *symbol grid* -- one byte per cell of the file's grid (PW_SYM_*) -- from the generator kernel through the
// transform kernel into the packer kernel, which writes the PwPuzzleHeader + table blob the step / render
// kernels read: generate -> (transform) -> pack -> train never touches host text.  The packer reproduces
// pw_puzzle_parse + pack_puzzle (csrc/pw_host.cpp) byte for byte on the same puzzle
// (tests/test_gpu_generate.py compares every section).

namespace {

struct GenShape {
  int8_t n;
  int8_t cell[3][2];  // (row offset, column offset), generate.py:215-225
};

__host__ __device__ inline GenShape gen_shape(int k) {
  // the monomino, the dominoes and the trominoes (generate.py:215-225), same order
  const GenShape kShapes[9] = {
      {1, {{0, 0}, {0, 0}, {0, 0}}}, {2, {{0, 0}, {0, 1}, {0, 0}}}, {2, {{0, 0}, {1, 0}, {0, 0}}},
      {3, {{0, 0}, {1, 0}, {1, 1}}}, {3, {{0, 0}, {0, 1}, {1, 1}}}, {3, {{0, 0}, {0, 1}, {1, 0}}},
      {3, {{1, 0}, {0, 1}, {1, 1}}}, {3, {{0, 0}, {0, 1}, {0, 2}}}, {3, {{0, 0}, {1, 0}, {2, 0}}},
  };
  return kShapes[k];
}

// counter-based random stream of one puzzle: draw c of puzzle p = mix64(seed, p, c) (the hash of pw_resample)
struct GenRng {
  uint64_t seed, puzzle, counter;
  __host__ __device__ uint32_t below(uint32_t n) {  // uniform in [0, n)
    const uint64_t r = mix64(seed, puzzle, counter++);
#if defined(__HIP_DEVICE_COMPILE__)
    return static_cast<uint32_t>(__umul64hi(r, static_cast<uint64_t>(n)));
#else
    return static_cast<uint32_t>((static_cast<unsigned __int128>(r) * n) >> 64);
#endif
  }
  __host__ __device__ int range(int lo, int hi) { return lo + static_cast<int>(below(static_cast<uint32_t>(hi - lo + 1))); }
};

// place_object (generate.py:28-71): 100 uniformly random positions, first free one wins
__host__ __device__ inline bool gen_drop(uint8_t* grid, int slot_w, int w, int h, uint8_t sym, const GenShape& s, GenRng& rng) {
  int rows = 0, cols = 0;
  for (int i = 0; i < s.n; i++) {
    rows = s.cell[i][0] + 1 > rows ? s.cell[i][0] + 1 : rows;
    cols = s.cell[i][1] + 1 > cols ? s.cell[i][1] + 1 : cols;
  }
  if (cols > w || rows > h) return false;
  for (int attempt = 0; attempt < 100; attempt++) {
    const int x = static_cast<int>(rng.below(static_cast<uint32_t>(w + 1 - cols)));
    const int y = static_cast<int>(rng.below(static_cast<uint32_t>(h + 1 - rows)));
    bool free_ = true;
    for (int i = 0; i < s.n; i++) free_ = free_ && grid[(y + s.cell[i][0]) * slot_w + x + s.cell[i][1]] == PW_SYM_EMPTY;
    if (!free_) continue;
    for (int i = 0; i < s.n; i++) grid[(y + s.cell[i][0]) * slot_w + x + s.cell[i][1]] = sym;
    return true;
  }
  return false;
}

// One puzzle of generate_level0_puzzles (generate.py:136-259): parameters drawn from the configured ranges,
// generate_puzzle (generate.py:74-133) retried until every object found a place.  Same recipe and argument
// meaning as the reference, own random stream.  Returns false after 1000 failed attempts (impossible ranges).
// *failed (optional): the number of generate_puzzle attempts that raised FailedToGenerateError before the one kept.
__host__ __device__ inline bool gen_level0(const PwGenConfig& c, uint64_t index, uint8_t* grid, int slot_w, int32_t* dims,
                                           int32_t* failed = nullptr) {
  GenRng rng{c.seed, index, 0};
  const int n_shapes = c.complex_shapes ? 9 : 1;
  for (int attempt = 0; attempt < 1000; attempt++) {
    if (failed) *failed = attempt;
    const int w = rng.range(c.min_size, c.max_size), h = rng.range(c.min_size, c.max_size);
    const int n_walls = rng.range(c.min_walls, c.max_walls);
    const int n_obst = rng.range(c.min_obstacles, c.max_obstacles);
    const int n_goals = rng.range(c.min_goal_objects, c.max_goal_objects);
    for (int i = 0; i < slot_w * slot_w; i++) grid[i] = PW_SYM_EMPTY;
    const int first = static_cast<int>(rng.below(n_shapes));
    bool ok = gen_drop(grid, slot_w, w, h, PW_SYM_MOVABLE | 1, gen_shape(first), rng) &&
              gen_drop(grid, slot_w, w, h, PW_SYM_GOAL | 1, gen_shape(first), rng);
    if (ok && n_goals == 2) {
      int second = static_cast<int>(rng.below(n_shapes));
      while (second == first) second = static_cast<int>(rng.below(n_shapes));
      ok = gen_drop(grid, slot_w, w, h, PW_SYM_MOVABLE | 2, gen_shape(second), rng) &&
           gen_drop(grid, slot_w, w, h, PW_SYM_GOAL | 2, gen_shape(second), rng);
    }
    ok = ok && gen_drop(grid, slot_w, w, h, PW_SYM_AGENT, gen_shape(static_cast<int>(rng.below(n_shapes))), rng);
    for (int i = 0; ok && i < n_obst; i++)
      ok = gen_drop(grid, slot_w, w, h, static_cast<uint8_t>(PW_SYM_MOVABLE | (1 + i + n_goals)),
                    gen_shape(static_cast<int>(rng.below(n_shapes))), rng);
    for (int i = 0; ok && i < n_walls; i++) ok = gen_drop(grid, slot_w, w, h, PW_SYM_WALL, gen_shape(0), rng);
    if (ok) {
      dims[0] = w;
      dims[1] = h;
      return true;
    }
  }
  dims[0] = dims[1] = 0;
  return false;
}

struct GenArgs {
  PwGenConfig cfg;
  uint64_t first;
  int32_t count;
  int32_t slot_w;
  uint8_t* grids;
  int32_t* dims;
};

__global__ __launch_bounds__(64) void pw_generate_level0_kernel(GenArgs a) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= a.count) return;
  gen_level0(a.cfg, a.first + static_cast<uint64_t>(i), a.grids + static_cast<int64_t>(i) * a.slot_w * a.slot_w, a.slot_w,
             a.dims + 2 * i);
}

// ------------------------------------------------------------------------------------
// The 8 dihedral variants (transform.py:21-48): variant v = 4 * flipped + quarter turns; the flip is top-bottom
// and applied BEFORE the clockwise rotation.  Thread per output cell.
// ------------------------------------------------------------------------------------
struct TransformArgs {
  const uint8_t* in;
  const int32_t* in_dims;
  uint8_t* out;       // [count][8][slot_w * slot_w]
  int32_t* out_dims;  // [count][8][2]
  int32_t count, slot_w;
};

__global__ __launch_bounds__(256) void pw_transform_grids_kernel(TransformArgs a) {
  const int cells = a.slot_w * a.slot_w;
  const int64_t t = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (t >= static_cast<int64_t>(a.count) * 8 * cells) return;
  const int c = static_cast<int>(t % cells);
  const int v = static_cast<int>((t / cells) % 8);
  const int p = static_cast<int>(t / (static_cast<int64_t>(cells) * 8));
  const int w = a.in_dims[2 * p], h = a.in_dims[2 * p + 1];
  const int turns = v & 3;
  const bool flip = v >= 4;
  const int ow = (turns & 1) ? h : w, oh = (turns & 1) ? w : h;
  if (c == 0) {
    a.out_dims[(p * 8 + v) * 2] = ow;
    a.out_dims[(p * 8 + v) * 2 + 1] = oh;
  }
  const int oy = c / a.slot_w, ox = c - oy * a.slot_w;
  uint8_t sym = PW_SYM_EMPTY;
  if (ox < ow && oy < oh) {
    // undo the clockwise quarter turns: new[r][c] = old[rows - 1 - c][r]
    int x = ox, y = oy, cw = ow, ch = oh;
    for (int k = 0; k < turns; k++) {
      const int px = y, py = cw - 1 - x;  // position before one clockwise turn (its grid was ch wide, cw high)
      x = px;
      y = py;
      const int t2 = cw;
      cw = ch;
      ch = t2;
    }
    if (flip) y = h - 1 - y;
    sym = a.in[static_cast<int64_t>(p) * cells + y * a.slot_w + x];
  }
  a.out[t] = sym;
}

// ------------------------------------------------------------------------------------
// Packer: symbol grid -> PwPuzzleHeader + table blob, one wavefront per puzzle (lane = grid row, H <= 64).
// ------------------------------------------------------------------------------------
#define PW_PACK_IDS 48  // element numbers 0 .. 47 ("M47", "G47")

struct PackArgs {
  const uint8_t* grids;
  const int32_t* dims;
  int32_t count, slot_w, order;
  PwPuzzleHeader* hdrs;
  uint8_t* blob;
  uint32_t blob_slot;  // bytes per puzzle in the blob (multiple of 16)
  int32_t* status;     // PW_OK or the error pw_puzzle_parse would report
};

// sort key of an element number under the string comparison the parsers apply to "m<k>" / "g<k>" ("10" < "2")
__device__ __forceinline__ int pack_string_key(int k) { return k < 10 ? k * 100 : (k / 10) * 100 + 10 + (k % 10) + 1; }

// absent-neighbour mask (pw_format.h) of cell (x, y) of the set whose rows are up / mid / down
__device__ __forceinline__ uint32_t pack_absent(uint64_t up, uint64_t mid, uint64_t down, int x) {
  const auto bit = [](uint64_t r, int xx) { return (xx >= 0 && xx < 64) ? ((r >> xx) & 1ull) : 0ull; };
  uint32_t m = 0;
  if (!bit(mid, x - 1)) m |= PW_NB_L;
  if (!bit(mid, x + 1)) m |= PW_NB_R;
  if (!bit(up, x)) m |= PW_NB_U;
  if (!bit(down, x)) m |= PW_NB_D;
  if (!bit(up, x - 1)) m |= PW_NB_UL;
  if (!bit(up, x + 1)) m |= PW_NB_UR;
  if (!bit(down, x - 1)) m |= PW_NB_DL;
  if (!bit(down, x + 1)) m |= PW_NB_DR;
  return m;
}

__global__ __launch_bounds__(64) void pw_pack_grid_kernel(PackArgs a) {
  __shared__ uint64_t rows_m[PW_PACK_IDS][64];
  __shared__ uint64_t rows_g[PW_PACK_IDS][64];
  __shared__ uint64_t rows_a[64], rows_w[64], rows_aw[64];
  __shared__ int32_t first_m[PW_PACK_IDS];  // row-major position of the element's first cell, -1 = absent
  __shared__ int32_t first_g[PW_PACK_IDS];
  __shared__ int32_t obj_id[PW_MAX_OBJECTS];   // movable j: element number, -1 = the agent
  __shared__ int32_t goal_id[PW_MAX_OBJECTS];
  __shared__ int32_t obj_geo[PW_MAX_OBJECTS][4];  // min x, min y, w, h
  __shared__ int32_t obj_cells[PW_MAX_OBJECTS + 1], obj_rowoff[PW_MAX_OBJECTS + 1];
  __shared__ int32_t counts[4];  // N, G, status, has_aw
  const int p = blockIdx.x, lane = threadIdx.x;
  const int W0 = a.dims[2 * p], H0 = a.dims[2 * p + 1];
  const int W = W0 + 2, H = H0 + 2;
  const uint8_t* grid = a.grids + static_cast<int64_t>(p) * a.slot_w * a.slot_w;
  PwPuzzleHeader* hdr = a.hdrs + p;
  uint8_t* blob = a.blob + static_cast<int64_t>(p) * a.blob_slot;

  // ---- 1. row bitboards of every element (lane y owns row y of all of them) ---------------------------------
  for (int k = 0; k < PW_PACK_IDS; k++) {
    rows_m[k][lane] = 0;
    rows_g[k][lane] = 0;
  }
  uint64_t w_row = 0, aw_row = 0, a_row = 0;
  bool bad_symbol = false;
  if (lane < H) {
    const uint64_t full = W >= 64 ? ~0ull : ((1ull << W) - 1ull);
    w_row = (lane == 0 || lane == H - 1) ? full : (1ull | (1ull << (W - 1)));  // the border walls, puzzle.py:160-168
    if (lane >= 1 && lane <= H0) {
      for (int x0 = 0; x0 < W0; x0++) {
        const uint8_t sym = grid[(lane - 1) * a.slot_w + x0];
        const uint64_t bit = 1ull << (x0 + 1);
        const int k = sym & 0x3f;
        if (sym == PW_SYM_WALL) w_row |= bit;
        else if (sym == PW_SYM_AWALL) aw_row |= bit;
        else if (sym == PW_SYM_AGENT) a_row |= bit;
        else if ((sym & 0xc0) == PW_SYM_MOVABLE && k < PW_PACK_IDS) rows_m[k][lane] |= bit;
        else if ((sym & 0xc0) == PW_SYM_GOAL && k < PW_PACK_IDS) rows_g[k][lane] |= bit;
        else if (sym != PW_SYM_EMPTY) bad_symbol = true;
      }
    }
  }
  rows_w[lane] = w_row;
  rows_aw[lane] = aw_row;
  rows_a[lane] = a_row;
  __syncthreads();

  // ---- 2. which elements exist, where each one is first seen (lane k < 48: movable k and goal k) -------------
  if (lane < PW_PACK_IDS) {
    int fm = -1, fg = -1;
    for (int y = 0; y < H; y++) {
      if (fm < 0 && rows_m[lane][y]) fm = y * 64 + __ffsll(static_cast<long long>(rows_m[lane][y])) - 1;
      if (fg < 0 && rows_g[lane][y]) fg = y * 64 + __ffsll(static_cast<long long>(rows_g[lane][y])) - 1;
    }
    first_m[lane] = fm;
    first_g[lane] = fg;
  }
  const bool has_agent = __ballot(a_row != 0ull) != 0ull;
  const bool has_aw = __ballot(aw_row != 0ull) != 0ull;
  const bool any_bad = __ballot(bad_symbol) != 0ull;
  __syncthreads();

  // ---- 3. object order (lane 0; at most 32 objects): pw_host.cpp parse_puzzle -------------------------------
  if (lane == 0) {
    int status = PW_OK, N = 0, G = 0;
    if (any_bad || W > PW_MAX_DIM || H > PW_MAX_DIM || W0 < 1 || H0 < 1) status = PW_ELIMIT;
    if (status == PW_OK && !has_agent) status = PW_EPARSE;
    // goals ascending by name (string order), reversed for the Python order (puzzle.py:178-179)
    int gl[PW_PACK_IDS], ng = 0;
    for (int k = 0; k < PW_PACK_IDS; k++)
      if (first_g[k] >= 0) gl[ng++] = k;
    for (int i = 1; i < ng; i++)  // insertion sort by string key
      for (int j = i; j > 0 && pack_string_key(gl[j - 1]) > pack_string_key(gl[j]); j--) {
        const int t = gl[j];
        gl[j] = gl[j - 1];
        gl[j - 1] = t;
      }
    if (a.order == PW_ORDER_PYTHON)
      for (int i = 0; i < ng / 2; i++) {
        const int t = gl[i];
        gl[i] = gl[ng - 1 - i];
        gl[ng - 1 - i] = t;
      }
    uint64_t listed = 0;
    if (status == PW_OK) {
      obj_id[N++] = -1;
      for (int i = 0; i < ng && status == PW_OK; i++) {
        if (first_m[gl[i]] < 0) status = PW_EGOAL;  // puzzle.py:230-232
        else if (N >= PW_MAX_OBJECTS) status = PW_ELIMIT;
        else {
          goal_id[G++] = gl[i];
          obj_id[N++] = gl[i];
          listed |= 1ull << gl[i];
        }
      }
    }
    // the remaining movables: in file order for Python (dict insertion order, puzzle.py:235-237), ascending
    // names for C++ (std::map, pushworld_puzzle.cc:274)
    int rest[PW_PACK_IDS], nr = 0;
    for (int k = 0; k < PW_PACK_IDS; k++)
      if (first_m[k] >= 0 && !((listed >> k) & 1ull)) rest[nr++] = k;
    for (int i = 1; i < nr; i++)
      for (int j = i; j > 0; j--) {
        const bool gt = a.order == PW_ORDER_PYTHON ? first_m[rest[j - 1]] > first_m[rest[j]]
                                                    : pack_string_key(rest[j - 1]) > pack_string_key(rest[j]);
        if (!gt) break;
        const int t = rest[j];
        rest[j] = rest[j - 1];
        rest[j - 1] = t;
      }
    for (int i = 0; i < nr && status == PW_OK; i++) {
      if (N >= PW_MAX_OBJECTS) status = PW_ELIMIT;
      else obj_id[N++] = rest[i];
    }
    counts[0] = N;
    counts[1] = G;
    counts[2] = status;
    counts[3] = has_aw ? 1 : 0;
    a.status[p] = status;
  }
  __syncthreads();
  const int N = counts[0], G = counts[1];
  if (counts[2] != PW_OK) return;

  // ---- 4. geometry of every movable (lane j) and goal ---------------------------------------------------------
  if (lane < N) {
    const uint64_t* rows = obj_id[lane] < 0 ? rows_a : rows_m[obj_id[lane]];
    int minx = 64, maxx = -1, miny = 64, maxy = -1, cells = 0;
    for (int y = 0; y < H; y++) {
      const uint64_t r = rows[y];
      if (!r) continue;
      miny = min(miny, y);
      maxy = y;
      minx = min(minx, __ffsll(static_cast<long long>(r)) - 1);
      maxx = max(maxx, 63 - __clzll(static_cast<long long>(r)));
      cells += __popcll(r);
    }
    obj_geo[lane][0] = minx;
    obj_geo[lane][1] = miny;
    obj_geo[lane][2] = maxx - minx + 1;
    obj_geo[lane][3] = maxy - miny + 1;
    obj_cells[lane] = cells;
  }
  __syncthreads();
  if (lane == 0) {  // exclusive prefix sums: shape-row offsets and movable-cell offsets
    int ro = 0, co = 0;
    for (int j = 0; j < N; j++) {
      const int h = obj_geo[j][3], c = obj_cells[j];
      obj_rowoff[j] = ro;
      obj_cells[j] = co;
      ro += h;
      co += c;
    }
    obj_rowoff[N] = ro;
    obj_cells[N] = co;
  }
  __syncthreads();
  const int S = obj_rowoff[N], n_mcells = obj_cells[N];
  // section offsets exactly as pack_puzzle's append() lays them out (every section 8-byte aligned)
  const uint32_t off_wall = 0, off_awall = 8u * H, off_shapes = 16u * H, off_static = 16u * H + 8u * S;
  const uint32_t off_mcells = (off_static + 4u * W * H + 7u) & ~7u;
  const uint32_t off_small = (off_mcells + 4u * static_cast<uint32_t>(max(n_mcells, 1)) + 7u) & ~7u;

  // ---- 5. header ------------------------------------------------------------------------------------------------
  for (int i = lane; i < static_cast<int>(sizeof(PwPuzzleHeader) / 4); i += 64) reinterpret_cast<uint32_t*>(hdr)[i] = 0u;
  __syncthreads();
  if (lane == 0) {
    hdr->base = static_cast<uint32_t>(static_cast<int64_t>(p) * a.blob_slot);
    hdr->W = static_cast<uint8_t>(W);
    hdr->H = static_cast<uint8_t>(H);
    hdr->N = static_cast<uint8_t>(N);
    hdr->G = static_cast<uint8_t>(G);
    hdr->off_wall = off_wall;
    hdr->off_awall = off_awall;
    hdr->off_shapes = off_shapes;
    hdr->off_static = off_static;
    hdr->off_mcells = off_mcells;
    hdr->n_mcells = static_cast<uint32_t>(n_mcells);
    hdr->has_aw = static_cast<uint32_t>(counts[3]);
    hdr->off_small = off_small;
  }
  if (lane < N) {
    hdr->objtab[lane].w = static_cast<uint8_t>(obj_geo[lane][2]);
    hdr->objtab[lane].h = static_cast<uint8_t>(obj_geo[lane][3]);
    hdr->objtab[lane].row_off = static_cast<uint16_t>(obj_rowoff[lane]);
    hdr->init[lane][0] = static_cast<int8_t>(obj_geo[lane][0]);
    hdr->init[lane][1] = static_cast<int8_t>(obj_geo[lane][1]);
  }
  if (lane < G) {  // goal origin = (min x, min y) of its cells, puzzle.py:187-188
    const uint64_t* rows = rows_g[goal_id[lane]];
    int minx = 64, miny = 64;
    for (int y = 0; y < H; y++)
      if (rows[y]) {
        miny = min(miny, y);
        minx = min(minx, __ffsll(static_cast<long long>(rows[y])) - 1);
      }
    hdr->goal[lane][0] = static_cast<int8_t>(minx);
    hdr->goal[lane][1] = static_cast<int8_t>(miny);
  }

  // ---- 6. blob: wall rows, wall | agent-wall rows (trap T2), shape rows ---------------------------------------
  for (uint32_t i = lane; i < a.blob_slot / 4; i += 64) reinterpret_cast<uint32_t*>(blob)[i] = 0u;
  __syncthreads();
  if (lane < H) {
    reinterpret_cast<uint64_t*>(blob + off_wall)[lane] = w_row;
    reinterpret_cast<uint64_t*>(blob + off_awall)[lane] = w_row | aw_row;
  }
  for (int j = 0; j < N; j++) {
    const uint64_t* rows = obj_id[j] < 0 ? rows_a : rows_m[obj_id[j]];
    if (lane < obj_geo[j][3])
      reinterpret_cast<uint64_t*>(blob + off_shapes)[obj_rowoff[j] + lane] = rows[obj_geo[j][1] + lane] >> obj_geo[j][0];
  }
  if (lane < N) {  // 8x8 boards of the movables that fit (pw_small_board of the shape rows above)
    const uint64_t* rows = obj_id[lane] < 0 ? rows_a : rows_m[obj_id[lane]];
    uint64_t s = 0;
    if (obj_geo[lane][2] <= 8 && obj_geo[lane][3] <= 8)
      for (int r = 0; r < obj_geo[lane][3]; r++) s |= ((rows[obj_geo[lane][1] + r] >> obj_geo[lane][0]) & 0xffull) << (8 * r);
    reinterpret_cast<uint64_t*>(blob + off_small)[lane] = s;
  }
  // ---- 7. static render codes (pack_puzzle: agent walls u walls, then walls on top, goal outlines in the top byte)
  if (lane < H) {
    const int y = lane;
    const uint64_t w_up = y > 0 ? rows_w[y - 1] : 0ull, w_dn = y + 1 < H ? rows_w[y + 1] : 0ull;
    const uint64_t aw_mid = w_row | aw_row;
    const uint64_t aw_up = y > 0 ? (rows_w[y - 1] | rows_aw[y - 1]) : 0ull;
    const uint64_t aw_dn = y + 1 < H ? (rows_w[y + 1] | rows_aw[y + 1]) : 0ull;
    uint32_t* codes = reinterpret_cast<uint32_t*>(blob + off_static) + y * W;
    for (int x = 0; x < W; x++) {
      uint32_t code = 0;
      if (counts[3] && ((aw_mid >> x) & 1ull)) code = (1u << PW_CODE_KIND_SHIFT) | pack_absent(aw_up, aw_mid, aw_dn, x);
      if ((w_row >> x) & 1ull) code = (2u << PW_CODE_KIND_SHIFT) | pack_absent(w_up, w_row, w_dn, x);
      for (int g = 0; g < G; g++) {
        const uint64_t* rows = rows_g[goal_id[g]];
        if ((rows[y] >> x) & 1ull)
          code |= pack_absent(y > 0 ? rows[y - 1] : 0ull, rows[y], y + 1 < H ? rows[y + 1] : 0ull, x) << PW_CODE_GOAL_SHIFT;
      }
      codes[x] = code;
    }
  }
  // ---- 8. movable cells: object by object, cells sorted by (x, y) like std::set<std::pair<int, int>> ------------
  if (lane < N) {
    const uint64_t* rows = obj_id[lane] < 0 ? rows_a : rows_m[obj_id[lane]];
    const int minx = obj_geo[lane][0], miny = obj_geo[lane][1], w = obj_geo[lane][2], h = obj_geo[lane][3];
    uint32_t* out = reinterpret_cast<uint32_t*>(blob + off_mcells) + obj_cells[lane];
    for (int cx = 0; cx < w; cx++)
      for (int cy = 0; cy < h; cy++) {
        const int x = minx + cx, y = miny + cy;
        if (!((rows[y] >> x) & 1ull)) continue;
        const uint32_t m = pack_absent(y > 0 ? rows[y - 1] : 0ull, rows[y], y + 1 < H ? rows[y + 1] : 0ull, x);
        *out++ = static_cast<uint32_t>(cx) | (static_cast<uint32_t>(cy) << 8) | (m << 16) | (static_cast<uint32_t>(lane) << 24);
      }
  }
}

// bytes one puzzle of at most w0 x h0 file cells can need in the blob (pack_puzzle's sections, rounded up to 16)
uint32_t pack_slot_bytes(int w0, int h0) {
  const uint32_t W = w0 + 2, H = h0 + 2, inner = static_cast<uint32_t>(w0) * h0;
  const uint32_t bytes = 16u * H + 8u * inner + 4u * W * H + 8u + 4u * std::max<uint32_t>(inner, 1u) + 8u +
                         8u * std::min<uint32_t>(std::max<uint32_t>(inner, 1u), PW_MAX_OBJECTS) + 16u;
  return (bytes + 15u) & ~15u;
}

}  // namespace

extern "C" {

static int gen_check(const PwGenConfig* c) {
  if (!c) return pw_fail(PW_EINVAL, "null config");
  if (c->min_size < 1 || c->max_size > PW_MAX_DIM - 2 || c->min_size > c->max_size)
    return pw_fail(PW_EINVAL, "puzzle sizes must satisfy 1 <= min_size <= max_size <= 62");
  if (c->min_walls < 0 || c->min_walls > c->max_walls) return pw_fail(PW_EINVAL, "min_walls must be >= 0 and <= max_walls");
  if (c->min_obstacles < 0 || c->min_obstacles > c->max_obstacles)
    return pw_fail(PW_EINVAL, "min_obstacles must be >= 0 and <= max_obstacles");
  if (c->min_goal_objects < 1 || c->max_goal_objects > 2 || c->min_goal_objects > c->max_goal_objects)
    return pw_fail(PW_EINVAL, "goal objects: 1 <= min <= max <= 2");  // generate.py:200-208
  if (!c->complex_shapes && c->max_goal_objects > 1)
    return pw_fail(PW_EINVAL, "two goal objects need two distinct shapes: use complex shapes");  // generate.py:98-100
  if (c->max_goal_objects + c->max_obstacles + 1 >= PW_PACK_IDS) return pw_fail(PW_ELIMIT, "too many obstacles");
  return PW_OK;
}

int pw_generate_level0(int device, const PwGenConfig* cfg, uint64_t first, int32_t count, uint8_t* grids, int32_t* dims,
                       void* stream) try {
  if (int rc = gen_check(cfg)) return rc;
  if (!grids || !dims) return pw_fail(PW_EINVAL, "null argument");
  if (count <= 0) return PW_OK;
  if (device < 0) {  // host copy of the same function (tests, text export)
    for (int32_t i = 0; i < count; i++)
      gen_level0(*cfg, first + static_cast<uint64_t>(i), grids + static_cast<int64_t>(i) * cfg->max_size * cfg->max_size,
                 cfg->max_size, dims + 2 * i);
    return PW_OK;
  }
  PwDeviceGuard guard(device);
  GenArgs a{*cfg, first, count, cfg->max_size, grids, dims};
  hipLaunchKernelGGL(pw_generate_level0_kernel, dim3((count + 63) / 64), dim3(64), 0, static_cast<hipStream_t>(stream), a);
  return check_launch("pw_generate_level0");
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_generate_level0_attempts(const PwGenConfig* cfg, uint64_t first, int32_t count, int32_t* failed) try {
  if (int rc = gen_check(cfg)) return rc;
  if (!failed) return pw_fail(PW_EINVAL, "null argument");
  std::vector<uint8_t> grid(static_cast<size_t>(cfg->max_size) * cfg->max_size);
  int32_t dims[2];
  for (int32_t i = 0; i < count; i++) {
    failed[i] = 0;
    if (!gen_level0(*cfg, first + static_cast<uint64_t>(i), grid.data(), cfg->max_size, dims, failed + i)) failed[i] = 1000;
  }
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_transform_grids(int device, const uint8_t* grids, const int32_t* dims, int32_t count, int32_t slot_w, uint8_t* out,
                       int32_t* out_dims, void* stream) try {
  if (!grids || !dims || !out || !out_dims) return pw_fail(PW_EINVAL, "null argument");
  if (slot_w < 1 || slot_w > PW_MAX_DIM - 2) return pw_fail(PW_EINVAL, "slot_w must be in 1 .. 62");
  if (count <= 0) return PW_OK;
  PwDeviceGuard guard(device);
  TransformArgs a{grids, dims, out, out_dims, count, slot_w};
  const int64_t threads = static_cast<int64_t>(count) * 8 * slot_w * slot_w;
  hipLaunchKernelGGL(pw_transform_grids_kernel, dim3(static_cast<unsigned>((threads + 255) / 256)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), a);
  return check_launch("pw_transform_grids");
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_puzzleset_from_grids(int device, const uint8_t* grids, const int32_t* dims, int32_t count, int32_t slot_w, int order,
                            PwPuzzleSet** out, void* stream) try {
  if (!grids || !dims || !out) return pw_fail(PW_EINVAL, "null argument");
  if (device < 0) return pw_fail(PW_EDEVICE, "pw_puzzleset_from_grids packs on a HIP device");
  if (count <= 0) return pw_fail(PW_EINVAL, "empty puzzle set");
  if (slot_w < 1 || slot_w > PW_MAX_DIM - 2) return pw_fail(PW_EINVAL, "slot_w must be in 1 .. 62");
  if (order != PW_ORDER_PYTHON && order != PW_ORDER_CPP) return pw_fail(PW_EINVAL, "order must be PW_ORDER_PYTHON or PW_ORDER_CPP");
  PwDeviceGuard guard(device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  // the dimensions come to the host (8 bytes per puzzle) to size the blob; the puzzles themselves never do
  std::vector<int32_t> hdims(static_cast<size_t>(count) * 2);
  hipError_t err = hipMemcpyAsync(hdims.data(), dims, hdims.size() * 4, hipMemcpyDeviceToHost, st);
  if (err == hipSuccess) err = hipStreamSynchronize(st);
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string("pw_puzzleset_from_grids: ") + hipGetErrorString(err));
  int max_w0 = 0, max_h0 = 0;
  for (int32_t i = 0; i < count; i++) {
    if (hdims[2 * i] < 1 || hdims[2 * i + 1] < 1 || hdims[2 * i] > slot_w || hdims[2 * i + 1] > slot_w)
      return pw_fail(PW_EINVAL, "puzzle " + std::to_string(i) + " has no valid dimensions (generation failed?)");
    max_w0 = std::max(max_w0, hdims[2 * i]);
    max_h0 = std::max(max_h0, hdims[2 * i + 1]);
  }
  const uint32_t slot = pack_slot_bytes(max_w0, max_h0);
  if (static_cast<uint64_t>(slot) * count > (1ull << 32) - 16) return pw_fail(PW_ELIMIT, "packed tables would exceed 4 GiB");
  // owners: an exception from the host vectors below (the host copy of the blob can be GBs) frees everything
  struct SetOwner {
    PwPuzzleSet* s;
    ~SetOwner() { if (s) pw_puzzleset_destroy(s); }
  } owner{new (std::nothrow) PwPuzzleSet()};
  struct DevOwner {
    int32_t* p;
    ~DevOwner() { if (p) (void)hipFree(p); }
  } status_owner{nullptr};
  PwPuzzleSet* s = owner.s;
  if (!s) return pw_fail(PW_ENOMEM, "out of memory");
  s->device = device;
  s->count = count;
  int32_t*& d_status = status_owner.p;
  const size_t hb = static_cast<size_t>(count) * sizeof(PwPuzzleHeader), bb = static_cast<size_t>(slot) * count;
  err = hipMalloc(reinterpret_cast<void**>(&s->d_headers), hb);
  if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&s->d_blob), bb);
  if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&d_status), static_cast<size_t>(count) * 4);
  // alignment gaps and the unused tail of every blob slot are zero, like the host packer's: deterministic files
  // and checksums, nothing of the device's previous contents leaks into them
  if (err == hipSuccess) err = hipMemsetAsync(s->d_blob, 0, bb, st);
  if (err == hipSuccess) {
    PackArgs a{grids, dims, count, slot_w, order, s->d_headers, s->d_blob, slot, d_status};
    hipLaunchKernelGGL(pw_pack_grid_kernel, dim3(static_cast<unsigned>(count)), dim3(64), 0, st, a);
    err = hipGetLastError();
  }
  std::vector<int32_t> status(static_cast<size_t>(count), PW_OK);
  s->headers.resize(count);
  s->blob.resize(bb);
  if (err == hipSuccess) err = hipMemcpyAsync(status.data(), d_status, status.size() * 4, hipMemcpyDeviceToHost, st);
  // host copies of the packed tables (engine creation reads dimensions and static codes): binary, not text
  if (err == hipSuccess) err = hipMemcpyAsync(s->headers.data(), s->d_headers, hb, hipMemcpyDeviceToHost, st);
  if (err == hipSuccess) err = hipMemcpyAsync(s->blob.data(), s->d_blob, bb, hipMemcpyDeviceToHost, st);
  if (err == hipSuccess) err = hipStreamSynchronize(st);
  if (err != hipSuccess) return pw_hip_fail("pw_puzzleset_from_grids", err);
  for (int32_t i = 0; i < count; i++)
    if (status[i] != PW_OK) {
      const int code = status[i];
      const char* why = code == PW_EGOAL ? "Goal has no associated movable object"
                        : code == PW_EPARSE ? "Every puzzle must have an agent object, indicated by 'a'."
                                            : "puzzle exceeds the engine limits (64 x 64 cells, 32 movables, element numbers < 48)";
      return pw_fail(code, "puzzle " + std::to_string(i) + ": " + why);
    }
  for (const PwPuzzleHeader& h : s->headers) {
    s->max_w = std::max<int>(s->max_w, h.W);
    s->max_h = std::max<int>(s->max_h, h.H);
    s->max_n = std::max<int>(s->max_n, h.N);
  }
  owner.s = nullptr;
  *out = s;
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_grid_to_text(const uint8_t* grid, int32_t width, int32_t height, int32_t slot_w, char* buf, int32_t cap) try {
  if (!grid || width < 1 || height < 1 || slot_w < width) return pw_fail(PW_EINVAL, "bad grid");
  std::string out;
  for (int y = 0; y < height; y++) {
    for (int x = 0; x < width; x++) {
      const uint8_t sym = grid[y * slot_w + x];
      if (x) out += "  ";  // two spaces between tokens, generate.py:133 / transform.py:44
      if (sym == PW_SYM_EMPTY) out += ".";
      else if (sym == PW_SYM_WALL) out += "W";
      else if (sym == PW_SYM_AWALL) out += "AW";
      else if (sym == PW_SYM_AGENT) out += "A";
      else if ((sym & 0xc0) == PW_SYM_MOVABLE) out += "M" + std::to_string(sym & 0x3f);
      else if ((sym & 0xc0) == PW_SYM_GOAL) out += "G" + std::to_string(sym & 0x3f);
      else return pw_fail(PW_EINVAL, "unknown symbol in the grid");
    }
    if (y + 1 < height) out += "\n";
  }
  const int n = static_cast<int>(out.size());
  if (buf && cap > 0) {
    const int m = std::min(n, cap - 1);
    std::memcpy(buf, out.data(), m);
    buf[m] = 0;
  }
  return n;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_puzzleset_headers(const PwPuzzleSet* s, const void** data, size_t* bytes) try {
  if (!s || !data || !bytes) return pw_fail(PW_EINVAL, "null argument");
  *data = s->headers.data();
  *bytes = s->headers.size() * sizeof(PwPuzzleHeader);
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

}  // extern "C"

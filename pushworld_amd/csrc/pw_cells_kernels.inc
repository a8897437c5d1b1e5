// pw_cells_kernels.inc -- the compact cell-grid observation (pw_render_cells / pw_step_cells, DESIGN.md K10).
// Part of the single translation unit pw_kernels.hip.
//
// One environment's observation is uint8 [3][Hc][Wc]: plane 0 static kind (0 padding, 1 floor, 2 agent wall,
// 3 wall), plane 1 occupant (1 + movable index), plane 2 goal (1 + index of the movable that belongs there).
// Planes 0 and 2 depend on the puzzle alone: the engine keeps one BASE IMAGE per puzzle (the whole observation
// with plane 1 empty, built on the host by csrc/pw_cells.inc) and the kernel only composes plane 1 per environment.
//
// One WAVEFRONT per environment, up to four per workgroup:
//   1. paint plane 1 into the wavefront's LDS window (zeroed first): objects in ascending index order, one lane per
//      bounding-box cell, so that the largest index wins where objects overlap (the LDS executes one wavefront's writes
//      in program order).  The window covers the 16-byte chunks of the observation that hold plane-1 bytes, ~Hc Wc bytes;
//   2. stream the observation to HBM: 16-byte chunk c of the observation is base chunk c (a cache-resident load: few
//      puzzles) OR'ed with window chunk c (zero outside plane 1).  Every 16-byte aligned chunk of the environment's
//      byte range is ONE non-temporal store.  Environments need not start on a 16-byte boundary (a tight stride 3 Hc Wc
//      is rarely a multiple of 16): an output chunk straddles two observation chunks -- the lane's own and its left
//      neighbour's, passed across the wavefront -- and is assembled with one 128-bit funnel shift; only the two end
//      chunks of an environment, shared with its neighbours or the gap bytes, are written byte by byte.  Every output byte
//      is written exactly once, no byte outside [0, 3 Hc Wc) of an environment is touched.

struct CellsArgs {
  const PwPuzzleHeader* hdrs;
  const uint8_t* blob;
  const uint8_t* base;     // base images: puzzle p at base + p * base_stride (16-byte aligned, zero tail)
  const int32_t* puzzle_id;
  const int8_t* pos;
  uint8_t* out;
  int64_t env_stride;      // bytes, >= obs_bytes
  int32_t base_stride;     // obs_bytes rounded up to 16
  int32_t obs_bytes;       // 3 * Hc * Wc
  int32_t batch;
  int32_t np;
  int32_t hc, wc;
  int32_t num_puzzles;
  int32_t occ_first;       // first observation chunk holding plane-1 bytes: (Hc Wc) / 16
  int32_t occ_chunks;      // chunks of the LDS window: up to the chunk that holds the last plane-1 byte
  int32_t epw;             // environments (wavefronts) per workgroup
};

__device__ __forceinline__ pw_u32x4 pw_shfl_up1(pw_u32x4 v, pw_u32x4 lane0) {
  pw_u32x4 r;
  const int lane = threadIdx.x & 63;
  for (int k = 0; k < 4; k++) {
    const unsigned u = static_cast<unsigned>(__shfl_up(static_cast<int>(v[k]), 1, 64));
    r[k] = lane ? u : lane0[k];
  }
  return r;
}

__global__ __launch_bounds__(256) void pw_cells_kernel(CellsArgs a) {
  extern __shared__ pw_u32x4 cells_lds[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t env = static_cast<int64_t>(blockIdx.x) * a.epw + wave;
  const bool live = env < a.batch;
  pw_u32x4* win = cells_lds + static_cast<size_t>(wave) * a.occ_chunks;
  const int plane = a.hc * a.wc;
  int pid = 0;
  if (live) {
    pid = __builtin_amdgcn_readfirstlane(pw_clamp_pid(a.puzzle_id[env], a.num_puzzles));
    for (int c = lane; c < a.occ_chunks; c += 64) win[c] = pw_u32x4{0u, 0u, 0u, 0u};
  }
  __syncthreads();
  if (live) {
    const PwPuzzleHeader& h = a.hdrs[pid];
    const int N = h.N;
    const int oy = (a.hc - static_cast<int>(h.H)) / 2, ox = (a.wc - static_cast<int>(h.W)) / 2;
    const uint64_t* shapes = reinterpret_cast<const uint64_t*>(a.blob + h.base + h.off_shapes);
    const int8_t* p = a.pos + env * a.np * 2;
    uint8_t* occ = reinterpret_cast<uint8_t*>(win) + (plane - 16 * a.occ_first);  // plane-1 byte 0
    for (int k = 0; k < N; k++) {
      const PwObjEntry o = h.objtab[k];
      const int w = o.w, n = o.w * o.h;
      const int px = p[2 * k] + ox, py = p[2 * k + 1] + oy;
      for (int i = lane; i < n; i += 64) {
        const int y = i / w, x = i - y * w;
        const int cx = px + x, cy = py + y;
        if (((shapes[o.row_off + y] >> x) & 1u) && cx >= 0 && cx < a.wc && cy >= 0 && cy < a.hc)
          occ[cy * a.wc + cx] = static_cast<uint8_t>(k + 1);
      }
    }
  }
  __syncthreads();
  if (!live) return;
  uint8_t* dst = a.out + env * a.env_stride;
  const int mis = static_cast<int>(reinterpret_cast<uintptr_t>(dst) & 15);
  uint8_t* dst0 = dst - mis;  // output chunk g = dst0[16 g, 16 g + 16) = observation bytes [16 g - mis, ...)
  const int S = a.obs_bytes;
  const int nch = (mis + S + 15) >> 4;
  const int nbase = a.base_stride >> 4;
  const pw_u32x4* base = reinterpret_cast<const pw_u32x4*>(a.base + static_cast<size_t>(pid) * a.base_stride);
  pw_u32x4 carry = pw_u32x4{0u, 0u, 0u, 0u};  // observation chunk g0 - 1 (from lane 63 of the previous round)
  for (int g0 = 0; g0 < nch; g0 += 64) {
    const int g = g0 + lane;
    pw_u32x4 r = pw_u32x4{0u, 0u, 0u, 0u};  // observation chunk g
    if (g < nbase) r = base[g];
    const int wc_ = g - a.occ_first;
    if (wc_ >= 0 && wc_ < a.occ_chunks) r |= win[wc_];
    const pw_u32x4 l = pw_shfl_up1(r, carry);  // observation chunk g - 1
    for (int k = 0; k < 4; k++) carry[k] = static_cast<unsigned>(__builtin_amdgcn_readlane(static_cast<int>(r[k]), 63));
    if (g >= nch) continue;
    unsigned __int128 R, L;
    __builtin_memcpy(&R, &r, 16);
    __builtin_memcpy(&L, &l, 16);
    const unsigned __int128 v = mis ? (R << (8 * mis)) | (L >> (128 - 8 * mis)) : R;
    const int lo = 16 * g - mis;  // observation byte of the chunk's first byte
    if (lo >= 0 && lo + 16 <= S) {
      pw_u32x4 o;
      __builtin_memcpy(&o, &v, 16);
      __builtin_nontemporal_store(o, reinterpret_cast<pw_u32x4*>(dst0 + 16 * g));
    } else {  // an end chunk: only the environment's own bytes
      uint8_t b[16];
      __builtin_memcpy(b, &v, 16);
      for (int j = 0; j < 16; j++)
        if (lo + j >= 0 && lo + j < S) dst0[16 * g + j] = b[j];
    }
  }
}

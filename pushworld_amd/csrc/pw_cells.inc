// pw_cells.inc -- host half of the cell-grid observations (include/pushworld_amd.h pw_engine_cells_shape,
// pw_render_cells, pw_step_cells; kernel: csrc/pw_cells_kernels.inc).  Part of the single translation unit pw_kernels.hip.

namespace {

constexpr int kCellsLdsMax = 65536;  // LDS of one workgroup the cells kernel may use

int64_t cells_obs_bytes(const PwEngine* e) { return static_cast<int64_t>(3) * e->pad_h * e->pad_w; }
int64_t cells_base_stride(const PwEngine* e) { return (cells_obs_bytes(e) + 15) & ~int64_t(15); }

// The base image of every puzzle -- the observation with plane 1 empty -- built on the host from the packed tables and
// copied to the device once, by the first cells call of the engine (the caller holds the device guard).
int ensure_cells_base(PwEngine* e) {
  if (e->d_cells_base) return PW_OK;
  const PwPuzzleSet* s = e->set;
  if (static_cast<int64_t>(e->pad_h) * e->pad_w + 32 > kCellsLdsMax)  // (the LDS window of plane 1)
    return pw_fail(PW_ELIMIT, "cell-grid observations: pad_cell_height * pad_cell_width exceeds 65504 cells");
  const int hc = e->pad_h, wc = e->pad_w, plane = hc * wc;
  const size_t stride = static_cast<size_t>(cells_base_stride(e));
  std::vector<uint8_t> img(stride * s->count, 0);
  for (int p = 0; p < s->count; p++) {
    const PwPuzzleHeader& h = s->headers[p];
    const int W = h.W, H = h.H, oy = (hc - H) / 2, ox = (wc - W) / 2;
    const uint8_t* b = s->blob.data() + h.base;
    const uint32_t* codes = reinterpret_cast<const uint32_t*>(b + h.off_static);
    const uint64_t* shapes = reinterpret_cast<const uint64_t*>(b + h.off_shapes);
    uint8_t* out = img.data() + stride * p;
    for (int y = 0; y < H; y++)
      for (int x = 0; x < W; x++) {
        // static kind of the top layer: 0 floor, 1 agent wall, 2 wall (walls are painted over agent walls)
        const uint32_t kind = (codes[y * W + x] >> PW_CODE_KIND_SHIFT) & 0xfu;
        out[(y + oy) * wc + x + ox] = static_cast<uint8_t>(kind == 2 ? 3 : (kind == 1 ? 2 : 1));
      }
    for (int g = 0; g < h.G; g++) {  // ascending: the largest movable index wins where goals overlap
      const int k = g + 1;
      const PwObjEntry o = h.objtab[k];
      for (int y = 0; y < o.h; y++)
        for (int x = 0; x < o.w; x++) {
          if (!((shapes[o.row_off + y] >> x) & 1u)) continue;
          const int cx = h.goal[g][0] + x + ox, cy = h.goal[g][1] + y + oy;
          if (cx >= 0 && cx < wc && cy >= 0 && cy < hc) out[2 * plane + cy * wc + cx] = static_cast<uint8_t>(k + 1);
        }
    }
  }
  uint8_t* d = nullptr;
  if (hipMalloc(reinterpret_cast<void**>(&d), img.size()) != hipSuccess) {
    (void)hipGetLastError();
    return pw_fail(PW_ENOMEM, "cell-grid observations: cannot allocate the base images");
  }
  if (hipMemcpy(d, img.data(), img.size(), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(d);
    return pw_fail(PW_EDEVICE, "cell-grid observations: cannot upload the base images");
  }
  e->d_cells_base = d;
  e->cells_base_bytes = static_cast<int64_t>(img.size());
  return PW_OK;
}

int fill_cells_args(const PwEngine* e, const int32_t* puzzle_id, const int8_t* pos, void* cells, int64_t stride,
                    int32_t batch, CellsArgs* ca) {
  if (!puzzle_id || !pos || !cells) return pw_fail(PW_EINVAL, "null device pointer");
  if (stride < cells_obs_bytes(e)) return pw_fail(PW_EINVAL, "env_stride_bytes must be >= 3 * Hc * Wc");
  ca->hdrs = e->set->d_headers;
  ca->blob = e->set->d_blob;
  ca->base = e->d_cells_base;
  ca->puzzle_id = puzzle_id;
  ca->pos = pos;
  ca->out = static_cast<uint8_t*>(cells);
  ca->env_stride = stride;
  ca->base_stride = static_cast<int32_t>(cells_base_stride(e));
  ca->obs_bytes = static_cast<int32_t>(cells_obs_bytes(e));
  ca->batch = batch;
  ca->np = e->np;
  ca->hc = e->pad_h;
  ca->wc = e->pad_w;
  ca->num_puzzles = e->set->count;
  const int plane = e->pad_h * e->pad_w;
  ca->occ_first = plane >> 4;
  ca->occ_chunks = ((2 * plane + 15) >> 4) - ca->occ_first;
  ca->epw = std::min(4, kCellsLdsMax / (16 * ca->occ_chunks));
  return PW_OK;
}

void launch_cells(const CellsArgs& ca, hipStream_t st) {
  const unsigned grid = static_cast<unsigned>((static_cast<int64_t>(ca.batch) + ca.epw - 1) / ca.epw);
  hipLaunchKernelGGL(pw_cells_kernel, dim3(grid), dim3(64 * ca.epw), static_cast<size_t>(16) * ca.occ_chunks * ca.epw, st, ca);
}

}  // namespace

int pw_engine_cells_shape(PwEngine* e, int* h, int* w) try {
  if (!e) return pw_fail(PW_EINVAL, "null engine");
  PwDeviceGuard guard(e->set->device);
  if (int rc = ensure_cells_base(e)) return rc;
  if (h) *h = e->pad_h;
  if (w) *w = e->pad_w;
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_render_cells(PwEngine* e, const int32_t* puzzle_id, const int8_t* pos, void* cells, int64_t env_stride_bytes,
                    int32_t batch, void* stream) try {
  if (!e) return pw_fail(PW_EINVAL, "null engine");
  if (batch <= 0) return PW_OK;
  CellsArgs ca;
  if (int rc = fill_cells_args(e, puzzle_id, pos, cells, env_stride_bytes, batch, &ca)) return rc;
  PwDeviceGuard guard(e->set->device);
  if (int rc = ensure_cells_base(e)) return rc;
  ca.base = e->d_cells_base;
  launch_cells(ca, static_cast<hipStream_t>(stream));
  return check_launch("pw_render_cells");
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int pw_step_cells(PwEngine* e, const int32_t* puzzle_id, const uint8_t* actions, int8_t* pos, int32_t* steps,
                  double* reward, int8_t* dgoals, uint8_t* terminated, uint8_t* truncated, void* cells,
                  int64_t env_stride_bytes, int32_t batch, uint32_t flags, void* stream) try {
  StepArgs a;
  int rc = fill_step_args(e, puzzle_id, actions, pos, steps, reward, dgoals, terminated, truncated, batch, flags, &a);
  if (rc != PW_OK) return rc;
  if (batch <= 0) return PW_OK;
  CellsArgs ca;
  if ((rc = fill_cells_args(e, puzzle_id, pos, cells, env_stride_bytes, batch, &ca))) return rc;
  PwDeviceGuard guard(e->set->device);
  if ((rc = ensure_cells_base(e))) return rc;
  ca.base = e->d_cells_base;
  attach_binding(e, &a);
  hipStream_t st = static_cast<hipStream_t>(stream);
  launch_one_step(e, a, batch, st);  // exactly pw_step's launch
  launch_cells(ca, st);
  return check_launch("pw_step_cells");
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

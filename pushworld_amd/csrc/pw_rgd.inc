// ====================================================================================================
// Recursive graph distance heuristic (cpp/src/heuristics/recursive_graph_distance.cc, domain_transition_graph.cc)
//
// pw_rgd_create: feasible-movement graphs on the host (pw_host.cpp pw_movement_graphs), then ONE device allocation:
//   counter   uint64: states that ran out of budget
//   masks     uint8 [N][H][W]    bits 0..3 edges L, R, U, D, bit 4 node
//   map       int16 [N][H][W]    node index of a cell in its movable's graph (row-major order), -1 = not a node
//   cells     uint16 [sum n_o]   x | y << 8 of every node (the breadth-first searches start there)
//   edges     uint64 [N][4][H]   edge rows per direction (bit x of row y = the edge from (x, y))
//   offs      uint2 [4][N][N]    (first, count) of the push offsets of pusher i against pushee j (pushworld_puzzle.cc:123-138)
//   off       uint16 [...]       int8 dx | int8 dy << 8
//   obj       RgdObj [N]         distance table of each graph
//   dist      uint16 [n_o][n_o] per movable, target-major: dist[t][s] = edges on a shortest path s -> t, 0xFFFF = none
// The tables fill by one wavefront per (movable, target): lane y holds row y of the frontier as a 64-bit mask, moves
// left / right are shifts masked by the edge rows, moves up / down cross-lane shuffles, and the level count is the distance.
//
// pw_rgd_eval: one lane per state.  The recursion of get_goal_cost / get_recursive_pushing_cost runs on an explicit stack
// in LDS (one 16-byte frame per level of pushing depth, lane-interleaved); the top frame stays in registers.  Costs are
// integers; RGD_INF plays +inf: bounds are passed down as best - c and a child that finds nothing returns its bound, so
// c + (RGD_INF - c) gives RGD_INF back exactly, as inf - c + c does in float.  Pruning keeps the true minimum whatever the
// visiting order (movables ascending, directions L, R, U, D), so the result equals the reference's hash-order traversal.
// ====================================================================================================
#define RGD_INF 0x40000000u

struct RgdObj {
  uint64_t dist_off;  // element offset of this movable's table in dist
  uint32_t n;         // nodes
  uint32_t first;     // index of its first node in cells
};

struct PwRgd {
  PwEngine* eng;
  int device;
  int32_t puzzle;
  int W, H, N, G;
  int fewest;
  int64_t budget;
  uint8_t* d_base;     // the one allocation
  unsigned long long* d_exceeded;
  const uint8_t* d_masks;
  const int16_t* d_map;
  const uint16_t* d_cells;
  const uint64_t* d_edges;
  const uint2* d_offs;
  const uint16_t* d_off;
  const RgdObj* d_obj;
  uint16_t* d_dist;
  std::vector<RgdObj> obj;
  uint16_t goal[32];   // x | y << 8
  size_t bytes;
};

// ---- distance tables -----------------------------------------------------------------------------------------------
struct RgdBfsArgs {
  const int16_t* map;      // this movable's [H][W]
  const uint16_t* cells;   // this movable's nodes
  const uint64_t* edges;   // this movable's [4][H]
  uint16_t* dist;          // this movable's [n][n]
  int32_t n, W, H;
};

__global__ __launch_bounds__(256) void pw_rgd_bfs_kernel(RgdBfsArgs a) {
  const int lane = threadIdx.x & (PW_WAVE - 1);
  const int t = blockIdx.x * 4 + static_cast<int>(threadIdx.x) / PW_WAVE;  // target node (wave-uniform)
  if (t >= a.n) return;
  const int y = lane;
  uint64_t eL = 0, eR = 0, eU = 0, eD = 0;
  if (y < a.H) {
    eL = a.edges[0 * a.H + y];
    eR = a.edges[1 * a.H + y];
    eU = a.edges[2 * a.H + y];
    eD = a.edges[3 * a.H + y];
  }
  const uint32_t tc = a.cells[t];
  const int tx = tc & 0xff, ty = tc >> 8;
  uint64_t f = y == ty ? (1ull << tx) : 0ull;
  uint64_t seen = f;
  uint16_t* row = a.dist + static_cast<int64_t>(t) * a.n;
  if (y == ty) row[t] = 0;
  for (uint32_t level = 1;; level++) {
    // s reaches the frontier in one move in direction d when the frontier holds s + d and s has that edge
    uint64_t up = __shfl(f, (lane + PW_WAVE - 1) & (PW_WAVE - 1), PW_WAVE);  // row y - 1
    uint64_t dn = __shfl(f, (lane + 1) & (PW_WAVE - 1), PW_WAVE);            // row y + 1
    if (lane == 0) up = 0;
    if (lane == PW_WAVE - 1) dn = 0;
    uint64_t nx = ((f << 1) & eL) | ((f >> 1) & eR) | (up & eU) | (dn & eD);
    nx &= ~seen;
    if (__ballot(nx != 0ull) == 0ull) break;
    seen |= nx;
    f = nx;
    const int16_t* mrow = a.map + y * a.W;
    while (nx) {
      const int x = __builtin_ctzll(nx);
      nx &= nx - 1;
      row[mrow[x]] = static_cast<uint16_t>(level);  // level < n <= 4096
    }
  }
}

// ---- evaluation ----------------------------------------------------------------------------------------------------
struct RgdEvalArgs {
  const int32_t* states;
  float* cost;
  int32_t count;
  int32_t W, H, N, G;
  int32_t fewest;
  int32_t levels;          // LDS frames per lane (max(N - 2, 1))
  int64_t budget;
  const uint8_t* masks;
  const int16_t* map;
  const uint16_t* dist;
  const RgdObj* obj;
  const uint2* offs;
  const uint16_t* off;
  unsigned long long* exceeded;
  const unsigned long long* dcount;  // the count in device memory instead (the planner's new states), or NULL
  const unsigned long long* halt;    // returns at once while *halt != 0, or NULL
  uint16_t goal[32];
};

__device__ __forceinline__ int rgd_dx(int a) { return a == 0 ? -1 : (a == 1 ? 1 : 0); }
__device__ __forceinline__ int rgd_dy(int a) { return a == 2 ? -1 : (a == 3 ? 1 : 0); }

__device__ __forceinline__ uint32_t rgd_mask(const RgdEvalArgs& a, int o, int x, int y) {
  if (static_cast<unsigned>(x) >= static_cast<unsigned>(a.W) || static_cast<unsigned>(y) >= static_cast<unsigned>(a.H))
    return 0u;
  return a.masks[(o * a.H + y) * a.W + x];
}

// PathDistances::getDistance(s, t) of movable o; s must be a node
__device__ __forceinline__ uint32_t rgd_dist(const RgdEvalArgs& a, int o, int sx, int sy, int tx, int ty) {
  if (static_cast<unsigned>(tx) >= static_cast<unsigned>(a.W) || static_cast<unsigned>(ty) >= static_cast<unsigned>(a.H))
    return RGD_INF;
  const int ti = a.map[(o * a.H + ty) * a.W + tx];
  if (ti < 0) return RGD_INF;
  const int si = a.map[(o * a.H + sy) * a.W + sx];
  const RgdObj ob = a.obj[o];
  const uint16_t d = a.dist[ob.dist_off + static_cast<uint64_t>(ti) * ob.n + si];
  return d == 0xFFFFu ? RGD_INF : d;
}

// get_pushing_costs (recursive_graph_distance.cc:190-252) for ONE next position (nx, ny) of pusher p at (px, py): the
// cheapest way for p to make contact and push pushee o from (cx, cy) one step in action ae.  RGD_INF when p cannot.
__device__ __forceinline__ uint32_t rgd_push_cost(const RgdEvalArgs& a, int p, int px, int py, int nx, int ny, int o,
                                                  int cx, int cy, int ae) {
  const uint2 r = a.offs[(ae * a.N + p) * a.N + o];
  const int dx = rgd_dx(ae), dy = rgd_dy(ae);
  uint32_t best = RGD_INF;
  for (uint32_t k = 0; k < r.y; k++) {
    const uint32_t v = a.off[r.x + k];
    const int sx = cx + static_cast<int8_t>(v & 0xffu), sy = cy + static_cast<int8_t>(v >> 8);
    if (!((rgd_mask(a, p, sx, sy) >> ae) & 1u)) continue;  // the pushing move itself must be feasible
    uint32_t c;
    if (sx == px && sy == py && sx + dx == nx && sy + dy == ny) {
      c = 0u;  // the push happens in this very move
    } else {
      const uint32_t d = rgd_dist(a, p, nx, ny, sx, sy);
      if (d >= RGD_INF) continue;
      c = d + 1u;
    }
    best = c < best ? c : best;
  }
  return best;
}

// frame word 0: o (5) | x (6) << 5 | y (6) << 11 | effect direction (2) << 17 | pusher cursor (5) << 19 |
//               next-direction cursor (3) << 24 | depth (5) << 27
struct RgdFrame {
  int o, cx, cy, ae, p, nd, depth;
  uint32_t skip, best, c;
};

__device__ __forceinline__ uint4 rgd_pack(const RgdFrame& f) {
  const uint32_t w = static_cast<uint32_t>(f.o) | (static_cast<uint32_t>(f.cx) << 5) | (static_cast<uint32_t>(f.cy) << 11) |
                     (static_cast<uint32_t>(f.ae) << 17) | (static_cast<uint32_t>(f.p) << 19) |
                     (static_cast<uint32_t>(f.nd) << 24) | (static_cast<uint32_t>(f.depth) << 27);
  return make_uint4(w, f.skip, f.best, f.c);
}
__device__ __forceinline__ RgdFrame rgd_unpack(uint4 v) {
  RgdFrame f;
  f.o = v.x & 31u;
  f.cx = (v.x >> 5) & 63u;
  f.cy = (v.x >> 11) & 63u;
  f.ae = (v.x >> 17) & 3u;
  f.p = (v.x >> 19) & 31u;
  f.nd = (v.x >> 24) & 7u;
  f.depth = (v.x >> 27) & 31u;
  f.skip = v.y;
  f.best = v.z;
  f.c = v.w;
  return f;
}

// get_recursive_pushing_cost (recursive_graph_distance.cc:114-188) of movable o moving from (cx, cy) in direction ae, with
// the explicit stack `stk` (lane-interleaved, stride 64).  Returns min(bound, cost); sets `over` when the budget runs out.
__device__ uint32_t rgd_pushing_cost(const RgdEvalArgs& a, const uint16_t* pos, uint4* stk, int o, int cx, int cy, int ae,
                                     int depth, uint32_t bound, int64_t& frames, bool& over) {
  RgdFrame f;
  f.o = o;
  f.cx = cx;
  f.cy = cy;
  f.ae = ae;
  f.depth = depth;
  f.skip = 1u << o;
  f.best = bound;
  f.p = depth == 0 ? 0 : 1;  // depth 0: the agent alone; deeper: every other movable, never the agent (:129-135)
  f.nd = 0;
  f.c = 0;
  int level = 0;
  if (++frames > a.budget) {
    over = true;
    return 0;
  }
  for (;;) {
    const int pend = f.depth == 0 ? 1 : a.N;
    bool descend = false;
    while (f.p < pend) {
      if ((f.skip >> f.p) & 1u) {
        f.p++;
        f.nd = 0;
        continue;
      }
      const uint32_t pp = pos[f.p * PW_WAVE];
      const int px = pp & 0xff, py = pp >> 8;
      const uint32_t succ = rgd_mask(a, f.p, px, py) & 15u & (0xFu << f.nd);
      if (!succ) {
        f.p++;
        f.nd = 0;
        continue;
      }
      const int an = __builtin_ctz(succ);
      f.nd = an + 1;
      const int nx = px + rgd_dx(an), ny = py + rgd_dy(an);
      const uint32_t c = rgd_push_cost(a, f.p, px, py, nx, ny, f.o, f.cx, f.cy, f.ae);
      if (c >= f.best) continue;
      if (f.p == 0) {  // the agent pushes directly: + 1 for its own move (:154-161)
        f.best = c + 1u < f.best ? c + 1u : f.best;
        continue;
      }
      // the pusher must itself be pushed from (px, py) to (nx, ny): one level deeper
      f.c = c;
      stk[level * PW_WAVE] = rgd_pack(f);
      level++;
      if (++frames > a.budget) {
        over = true;
        return 0;
      }
      const uint32_t child_bound = f.best - c;
      const uint32_t child_skip = f.skip | (1u << f.p);
      f.o = f.p;
      f.cx = px;
      f.cy = py;
      f.ae = an;
      f.depth = f.depth - 1;
      f.skip = child_skip;
      f.best = child_bound;
      f.p = f.depth == 0 ? 0 : 1;
      f.nd = 0;
      descend = true;
      break;
    }
    if (descend) continue;
    const uint32_t r = f.best;
    if (level == 0) return r;
    level--;
    f = rgd_unpack(stk[level * PW_WAVE]);
    f.best = f.c + r;  // r <= parent best - c
  }
}

// get_goal_cost (recursive_graph_distance.cc:68-98)
__device__ uint32_t rgd_goal_cost(const RgdEvalArgs& a, const uint16_t* pos, uint4* stk, int o, int gx, int gy, int depth,
                                  int64_t& frames, bool& over) {
  const uint32_t cp = pos[o * PW_WAVE];
  const int cx = cp & 0xff, cy = cp >> 8;
  if (cx == gx && cy == gy) return 0u;
  uint32_t best = RGD_INF;
  const uint32_t succ = rgd_mask(a, o, cx, cy) & 15u;
  for (int ae = 0; ae < 4; ae++) {
    if (!((succ >> ae) & 1u)) continue;
    const uint32_t gd = rgd_dist(a, o, cx + rgd_dx(ae), cy + rgd_dy(ae), gx, gy);
    if (gd >= best) continue;
    const uint32_t r = rgd_pushing_cost(a, pos, stk, o, cx, cy, ae, depth, best - gd, frames, over);
    if (over) return 0u;
    best = gd + r;
  }
  return best;
}

// estimate_cost_to_goal (:43-66) of the state whose positions (x | y << 8, every one a node of its graph) are at pos[j * 64];
// NaN with `over` set when the budget runs out.  Goal k belongs to movable k + 1; the sum stops at the first infinite goal.
__device__ __forceinline__ float rgd_eval_pos(const RgdEvalArgs& a, const uint16_t* pos, uint4* stk, bool& over) {
  int64_t frames = 0;
  uint32_t total = 0;
  bool dead = false;
  for (int g = 0; g < a.G && !dead && !over; g++) {
    const int gx = a.goal[g] & 0xff, gy = a.goal[g] >> 8;
    uint32_t gc;
    if (a.fewest) {  // get_fewest_tools_goal_cost (:100-112): the first pushing depth with a finite cost
      gc = RGD_INF;
      for (int d = 0; d < a.N - 1 && !over; d++) {
        gc = rgd_goal_cost(a, pos, stk, g + 1, gx, gy, d, frames, over);
        if (gc < RGD_INF) break;
      }
    } else {
      gc = rgd_goal_cost(a, pos, stk, g + 1, gx, gy, a.N - 2, frames, over);
    }
    if (gc >= RGD_INF) dead = true;
    else total += gc;
  }
  if (over) return __builtin_nanf("");
  return dead ? __builtin_inff() : static_cast<float>(total);
}

__global__ __launch_bounds__(64) void pw_rgd_eval_kernel(RgdEvalArgs a) {
  extern __shared__ uint4 rgd_lds[];
  const int lane = threadIdx.x;
  const int64_t s = static_cast<int64_t>(blockIdx.x) * PW_WAVE + lane;
  if (a.halt && *a.halt) return;
  if (s >= (a.dcount ? static_cast<int64_t>(*a.dcount) : static_cast<int64_t>(a.count))) return;
  uint4* stk = rgd_lds + lane;
  uint16_t* pos = reinterpret_cast<uint16_t*>(rgd_lds + a.levels * PW_WAVE) + lane;
  // every movable must stand on a node of its own graph; otherwise NaN, decided before any evaluation
  bool on_graph = true;
  for (int j = 0; j < a.N; j++) {
    const int32_t v = a.states[s * a.N + j];
    const int x = v / PW_POSITION_LIMIT, y = v - x * PW_POSITION_LIMIT;
    const bool ok = v >= 0 && x < a.W && y < a.H && (rgd_mask(a, j, x, y) & PW_RGD_NODE);
    on_graph = on_graph && ok;
    pos[j * PW_WAVE] = ok ? static_cast<uint16_t>(x | (y << 8)) : 0;
  }
  if (!on_graph) {
    a.cost[s] = __builtin_nanf("");
    return;
  }
  bool over = false;
  const float c = rgd_eval_pos(a, pos, stk, over);
  if (over) atomicAdd(a.exceeded, 1ull);
  a.cost[s] = c;
}

struct RgdDistArgs {
  const int32_t* src;
  const int32_t* dst;
  float* d;
  int32_t count, W, H, obj;
  const int16_t* map;  // this movable's [H][W]
  const uint16_t* dist;  // this movable's [n][n]
  uint32_t n;
};

__global__ __launch_bounds__(256) void pw_rgd_dist_kernel(RgdDistArgs a) {
  const int64_t k = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
  if (k >= a.count) return;
  auto index = [&](int32_t v) -> int {
    const int x = v / PW_POSITION_LIMIT, y = v - x * PW_POSITION_LIMIT;
    if (v < 0 || x >= a.W || y >= a.H) return -1;
    return a.map[y * a.W + x];
  };
  const int si = index(a.src[k]), ti = index(a.dst[k]);
  float out = __builtin_inff();
  if (si >= 0 && ti >= 0) {
    const uint16_t v = a.dist[static_cast<uint64_t>(ti) * a.n + si];
    if (v != 0xFFFFu) out = static_cast<float>(v);
  }
  a.d[k] = out;
}

extern "C" {

void pw_rgd_destroy(PwRgd* r) {
  if (!r) return;
  if (r->d_base) {
    PwDeviceGuard guard(r->device);
    (void)hipFree(r->d_base);
  }
  delete r;
}

int pw_rgd_create(PwEngine* e, int32_t puzzle, int32_t fewest_tools, int64_t budget, PwRgd** out) try {
  if (!e || !out) return pw_fail(PW_EINVAL, "null argument");
  if (puzzle < 0 || puzzle >= e->set->count) return pw_fail(PW_EINVAL, "puzzle index out of range");
  if (budget < 0) return pw_fail(PW_EINVAL, "budget must be >= 0 (0 = PW_RGD_DEFAULT_BUDGET)");
  const PwPuzzleHeader& h = e->set->headers[puzzle];
  const int W = h.W, H = h.H, N = h.N, G = h.G;
  std::vector<uint8_t> masks;
  pw_movement_graphs(h, e->set->blob.data(), masks);
  std::vector<std::vector<PwCell>> offs;
  pw_push_offsets(h, e->set->blob.data(), offs);

  const size_t plane = static_cast<size_t>(W) * H;
  std::vector<int16_t> map(N * plane, -1);
  std::vector<uint16_t> cells;
  std::vector<uint64_t> edges(static_cast<size_t>(N) * 4 * H, 0);
  std::vector<RgdObj> obj(N);
  uint64_t dist_elems = 0;
  for (int j = 0; j < N; j++) {
    obj[j].first = static_cast<uint32_t>(cells.size());
    obj[j].dist_off = dist_elems;
    uint32_t n = 0;
    for (int y = 0; y < H; y++)
      for (int x = 0; x < W; x++) {
        const uint8_t m = masks[j * plane + y * W + x];
        if (!(m & PW_RGD_NODE)) continue;
        map[j * plane + y * W + x] = static_cast<int16_t>(n++);
        cells.push_back(static_cast<uint16_t>(x | (y << 8)));
        for (int a = 0; a < 4; a++)
          if ((m >> a) & 1u) edges[(static_cast<size_t>(j) * 4 + a) * H + y] |= 1ull << x;
      }
    obj[j].n = n;
    dist_elems += static_cast<uint64_t>(n) * n;
  }
  std::vector<uint2> odir(static_cast<size_t>(4) * N * N, make_uint2(0, 0));
  std::vector<uint16_t> off;
  for (size_t k = 0; k < odir.size(); k++) {
    odir[k] = make_uint2(static_cast<uint32_t>(off.size()), static_cast<uint32_t>(offs[k].size()));
    for (const auto& c : offs[k])
      off.push_back(static_cast<uint16_t>(static_cast<uint8_t>(c.first) | (static_cast<uint8_t>(c.second) << 8)));
  }
  if (off.empty()) off.push_back(0);
  if (cells.empty()) cells.push_back(0);

  // sections of the one allocation, 256-byte aligned
  size_t bytes = 0;
  auto section = [&](size_t n) {
    const size_t at = bytes;
    bytes += pw_pad256(n);
    return at;
  };
  const size_t o_cnt = section(8), o_masks = section(masks.size()), o_map = section(map.size() * 2),
               o_cells = section(cells.size() * 2), o_edges = section(edges.size() * 8), o_odir = section(odir.size() * 8),
               o_off = section(off.size() * 2), o_obj = section(obj.size() * sizeof(RgdObj));
  const size_t head = bytes;
  const size_t o_dist = section(dist_elems * 2);
  if (static_cast<int64_t>(bytes) > PW_RGD_MAX_BYTES)
    return pw_fail(PW_ELIMIT, "rgd tables would take " + std::to_string(bytes) + " bytes (limit PW_RGD_MAX_BYTES = 1 GiB)");
  std::vector<uint8_t> host(head, 0);
  std::memcpy(host.data() + o_masks, masks.data(), masks.size());
  std::memcpy(host.data() + o_map, map.data(), map.size() * 2);
  std::memcpy(host.data() + o_cells, cells.data(), cells.size() * 2);
  std::memcpy(host.data() + o_edges, edges.data(), edges.size() * 8);
  std::memcpy(host.data() + o_odir, odir.data(), odir.size() * 8);
  std::memcpy(host.data() + o_off, off.data(), off.size() * 2);
  std::memcpy(host.data() + o_obj, obj.data(), obj.size() * sizeof(RgdObj));

  PwRgd* r = new (std::nothrow) PwRgd();
  if (!r) return pw_fail(PW_ENOMEM, "out of memory");
  r->eng = e;
  r->device = e->set->device;
  r->puzzle = puzzle;
  r->W = W;
  r->H = H;
  r->N = N;
  r->G = G;
  r->fewest = fewest_tools ? 1 : 0;
  r->budget = budget > 0 ? budget : PW_RGD_DEFAULT_BUDGET;
  r->obj = obj;
  r->bytes = bytes;
  std::memset(r->goal, 0, sizeof(r->goal));
  for (int g = 0; g < G; g++) r->goal[g] = static_cast<uint16_t>(h.goal[g][0] | (h.goal[g][1] << 8));

  PwDeviceGuard guard(r->device);
  hipError_t err = guard.status();
  if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&r->d_base), bytes);
  if (err == hipSuccess) err = hipMemcpy(r->d_base, host.data(), head, hipMemcpyHostToDevice);
  if (err == hipSuccess && bytes > head) err = hipMemsetAsync(r->d_base + o_dist, 0xFF, bytes - head, nullptr);
  if (err != hipSuccess) {
    pw_rgd_destroy(r);
    return pw_hip_fail("pw_rgd_create", err);
  }
  r->d_exceeded = reinterpret_cast<unsigned long long*>(r->d_base + o_cnt);
  r->d_masks = r->d_base + o_masks;
  r->d_map = reinterpret_cast<const int16_t*>(r->d_base + o_map);
  r->d_cells = reinterpret_cast<const uint16_t*>(r->d_base + o_cells);
  r->d_edges = reinterpret_cast<const uint64_t*>(r->d_base + o_edges);
  r->d_offs = reinterpret_cast<const uint2*>(r->d_base + o_odir);
  r->d_off = reinterpret_cast<const uint16_t*>(r->d_base + o_off);
  r->d_obj = reinterpret_cast<const RgdObj*>(r->d_base + o_obj);
  r->d_dist = reinterpret_cast<uint16_t*>(r->d_base + o_dist);
  for (int j = 0; j < N; j++) {
    if (!obj[j].n) continue;
    RgdBfsArgs b{r->d_map + j * plane, r->d_cells + obj[j].first, r->d_edges + static_cast<size_t>(j) * 4 * H,
                 r->d_dist + obj[j].dist_off, static_cast<int32_t>(obj[j].n), W, H};
    hipLaunchKernelGGL(pw_rgd_bfs_kernel, dim3((obj[j].n + 3) / 4), dim3(256), 0, nullptr, b);
  }
  err = hipGetLastError();
  if (err == hipSuccess) err = hipStreamSynchronize(nullptr);
  if (err != hipSuccess) {
    const std::string msg = std::string("pw_rgd_create: ") + hipGetErrorString(err);
    pw_rgd_destroy(r);
    return pw_fail(PW_EDEVICE, msg);
  }
  *out = r;
  return PW_OK;
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

}  // extern "C"

static RgdEvalArgs rgd_eval_args(PwRgd* r, const int32_t* states, float* cost, int32_t count) {
  RgdEvalArgs a;
  a.states = states;
  a.cost = cost;
  a.count = count;
  a.W = r->W;
  a.H = r->H;
  a.N = r->N;
  a.G = r->G;
  a.fewest = r->fewest;
  a.levels = std::max(r->N - 2, 1);
  a.budget = r->budget;
  a.masks = r->d_masks;
  a.map = r->d_map;
  a.dist = r->d_dist;
  a.obj = r->d_obj;
  a.offs = r->d_offs;
  a.off = r->d_off;
  a.exceeded = r->d_exceeded;
  a.dcount = nullptr;
  a.halt = nullptr;
  std::memcpy(a.goal, r->goal, sizeof(a.goal));
  return a;
}

// frames (16 B per level) + positions (2 B per movable), per lane
static size_t rgd_eval_lds(const PwRgd* r) { return static_cast<size_t>(PW_WAVE) * (16 * std::max(r->N - 2, 1) + 2 * r->N); }

extern "C" int pw_rgd_eval(PwRgd* r, const int32_t* states, float* cost, int32_t count, void* stream) try {
  if (!r) return pw_fail(PW_EINVAL, "null argument");
  if (count < 0) return pw_fail(PW_EINVAL, "count must be >= 0");
  if (count == 0) return PW_OK;
  if (!states || !cost) return pw_fail(PW_EINVAL, "null device pointer");
  PwDeviceGuard guard(r->device);
  const RgdEvalArgs a = rgd_eval_args(r, states, cost, count);
  const size_t lds = rgd_eval_lds(r);
  const unsigned blocks = static_cast<unsigned>((static_cast<int64_t>(count) + PW_WAVE - 1) / PW_WAVE);
  hipLaunchKernelGGL(pw_rgd_eval_kernel, dim3(blocks), dim3(PW_WAVE), lds, static_cast<hipStream_t>(stream), a);
  return check_launch("pw_rgd_eval");
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

extern "C" {

int pw_rgd_distances(PwRgd* r, int32_t obj, const int32_t* src, const int32_t* dst, float* d, int32_t count,
                     void* stream) try {
  if (!r) return pw_fail(PW_EINVAL, "null argument");
  if (obj < 0 || obj >= r->N) return pw_fail(PW_EINVAL, "bad object index");
  if (count < 0) return pw_fail(PW_EINVAL, "count must be >= 0");
  if (count == 0) return PW_OK;
  if (!src || !dst || !d) return pw_fail(PW_EINVAL, "null device pointer");
  PwDeviceGuard guard(r->device);
  const size_t plane = static_cast<size_t>(r->W) * r->H;
  RgdDistArgs a{src, dst, d, count, r->W, r->H, obj, r->d_map + obj * plane, r->d_dist + r->obj[obj].dist_off,
                r->obj[obj].n};
  const unsigned blocks = static_cast<unsigned>((static_cast<int64_t>(count) + 255) / 256);
  hipLaunchKernelGGL(pw_rgd_dist_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  return check_launch("pw_rgd_distances");
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

int64_t pw_rgd_exceeded(PwRgd* r, void* stream) try {
  if (!r) return pw_fail(PW_EINVAL, "null argument");
  PwDeviceGuard guard(r->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  unsigned long long v = 0;
  hipError_t err = hipMemcpyAsync(&v, r->d_exceeded, 8, hipMemcpyDeviceToHost, st);
  if (err == hipSuccess) err = hipStreamSynchronize(st);
  if (err != hipSuccess) return pw_fail(PW_EDEVICE, std::string("pw_rgd_exceeded: ") + hipGetErrorString(err));
  return static_cast<int64_t>(v);
} catch (...) {
  return pw_current_exception();  // nothing C++ leaves the C ABI
}

}  // extern "C"

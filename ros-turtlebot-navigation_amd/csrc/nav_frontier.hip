// nav_frontier.hip — exploration frontiers of a filter particle's map as goals of the goal field (tbnav_nav.h G10-G16).  On the device:
// the frontier bits of every 32 x 32 tile from the particle's log-odds (nav_frontier_mark), their 8-connected clusters by minimum-label
// propagation (nav_frontier_label: nav_tiles.hpp's tile_fixed_point, nav_relax_tiles's body, under the min rule), the clusters' sizes and the seed bits (nav_frontier_sizes,
// nav_frontier_seeds), and the start of a solve from many goals (nav_reset_goals).  On the host: the visited mask (G14), the list of
// clusters (G16), and the calls' checks.  Integers and comparisons only; compiled without contraction like the rest of the planner.
#include <cstring>
#include <vector>

#include "rbpf_host.hpp"
#include "nav_host.hpp"

namespace tbnav_nk {

struct FrontierArgs {
  const double* lo;            // TilePool::lo
  ParticleRef p;
  double half_lo, half_hi, free_cut;   // ExportCuts: UNKNOWN is half_lo <= l <= half_hi, FREE is l <= free_cut (G10)
  const uint8_t* cost;         // [side][side] the grid the next solve would use
  const unsigned int* visited; // [side][TW]
  unsigned int* front;         // [side][TW] out
  unsigned int* label;         // [side][side] out: own index on a frontier cell, UNREACHED elsewhere
  unsigned int* size;          // [side][side] out: zero
  unsigned int* flags;         // [2][TT] out: round 0's active tiles, and zeros for round 1
  unsigned int* count;         // [0] += frontier cells
};

// One workgroup per tile.  Rows are ix (the slow index), bits within a row iy — the tiles' own layout.
__global__ __launch_bounds__(kThreads) void nav_frontier_mark(FrontierArgs a) {
  __shared__ unsigned int s_unk[kHalo];      // UNKNOWN bits of rows -1 .. 32 (own columns)
  __shared__ unsigned int s_free[kTile], s_pass[kTile], s_front[kTile];
  __shared__ unsigned int s_side[2];           // bit r: the cell left (iy = -1) / right (iy = 32) of row r is UNKNOWN
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tile_x = blockIdx.y, tile_y = blockIdx.x, tile = tile_x * a.p.TW + tile_y;
  const unsigned int* __restrict__ tab_p = particle_row(a.p);
  const unsigned int id = tab_p[tile];
  const int lx0 = tid >> 5, ly = tid & (kTile - 1), gy = tile_y * kTile + ly;
  if (id == 0u) {   // nobody has written this tile: unknown throughout, so no cell of it is FREE, whatever lies next door
#pragma unroll
    for (int j = 0; j < kOwn; ++j) {
      const int gx = tile_x * kTile + lx0 + j * kRowStep;
      if (gx < a.p.side && gy < a.p.side) { a.label[(size_t)gx * a.p.side + gy] = kInf; a.size[(size_t)gx * a.p.side + gy] = 0u; }
    }
    if (tid < kTile && tile_x * kTile + tid < a.p.side) a.front[(size_t)(tile_x * kTile + tid) * a.p.TW + tile_y] = 0u;
    if (tid == 0) { a.flags[tile] = 0u; a.flags[a.p.TT + tile] = 0u; }
    return;
  }
  // the tile's own 1024 log-odds, classified; a cell of a ragged last tile that is outside the map has no class
  const double* __restrict__ t_lo = a.lo + (size_t)id * (kTile * kTile);
#pragma unroll
  for (int j = 0; j < kOwn; ++j) {
    const int r = lx0 + j * kRowStep, gx = tile_x * kTile + r;
    const bool in = gx < a.p.side && gy < a.p.side;
    const double l = t_lo[r * kTile + ly];
    const unsigned long long bu = __ballot(in && l >= a.half_lo && l <= a.half_hi);
    const unsigned long long bf = __ballot(in && l <= a.free_cut);
    const unsigned long long bp = __ballot(in && a.cost[in ? (size_t)gx * a.p.side + gy : 0] != 0);
    if (lane == 0) {   // (lane 0's row is the even one of the wave's two)
      s_unk[1 + r] = (unsigned int)bu; s_unk[2 + r] = (unsigned int)(bu >> 32);
      s_free[r] = (unsigned int)bf; s_free[r + 1] = (unsigned int)(bf >> 32);
      s_pass[r] = (unsigned int)bp; s_pass[r + 1] = (unsigned int)(bp >> 32);
    }
  }
  // the facing row of the tiles above and below (wave 0) and the facing column of the tiles left and right (wave 1)
  if (wave == 0) {
    const bool up = lane < kTile;
    const int gx = up ? tile_x * kTile - 1 : tile_x * kTile + kTile, gyy = tile_y * kTile + (lane & (kTile - 1));
    bool u = false;
    if (gx >= 0 && gx < a.p.side && gyy < a.p.side) {
      const unsigned int nid = tab_p[(gx >> 5) * a.p.TW + tile_y];
      u = true;
      if (nid != 0u) { const double l = a.lo[(size_t)nid * (kTile * kTile) + (gx & (kTile - 1)) * kTile + (lane & (kTile - 1))]; u = l >= a.half_lo && l <= a.half_hi; }
    }
    const unsigned long long b = __ballot(u);
    if (lane == 0) { s_unk[0] = (unsigned int)b; s_unk[kHalo - 1] = (unsigned int)(b >> 32); }
  } else if (wave == 1) {
    const bool left = lane < kTile;
    const int r = lane & (kTile - 1), gx = tile_x * kTile + r, gyy = left ? tile_y * kTile - 1 : tile_y * kTile + kTile;
    bool u = false;
    if (gyy >= 0 && gyy < a.p.side && gx < a.p.side) {
      const unsigned int nid = tab_p[tile_x * a.p.TW + (gyy >> 5)];
      u = true;
      if (nid != 0u) { const double l = a.lo[(size_t)nid * (kTile * kTile) + r * kTile + (gyy & (kTile - 1))]; u = l >= a.half_lo && l <= a.half_hi; }
    }
    const unsigned long long b = __ballot(u);
    if (lane == 0) { s_side[0] = (unsigned int)b; s_side[1] = (unsigned int)(b >> 32); }
  }
  __syncthreads();
  // G11, a row per thread: FREE, passable, not visited, and UNKNOWN above, below, left or right
  if (tid < kTile) {
    const int r = tid, gx = tile_x * kTile + r;
    const unsigned int u = s_unk[1 + r];
    const unsigned int near = s_unk[r] | s_unk[2 + r] | (u << 1) | ((s_side[0] >> r) & 1u) | (u >> 1) | (((s_side[1] >> r) & 1u) << 31);
    unsigned int f = s_free[r] & s_pass[r] & near;
    if (gx < a.p.side) {
      f &= ~a.visited[(size_t)gx * a.p.TW + tile_y];
      a.front[(size_t)gx * a.p.TW + tile_y] = f;
    }
    s_front[r] = f;   // (a row outside the map has no FREE cell: f is 0 there)
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kOwn; ++j) {
    const int r = lx0 + j * kRowStep, gx = tile_x * kTile + r;
    if (gx < a.p.side && gy < a.p.side) {
      const unsigned int g = (unsigned int)gx * (unsigned int)a.p.side + (unsigned int)gy;
      a.label[g] = (s_front[r] >> ly) & 1u ? g : kInf;
      a.size[g] = 0u;
    }
  }
  if (tid == 0) {
    unsigned int total = 0u;
    for (int r = 0; r < kTile; ++r) total += __popc(s_front[r]);
    a.flags[tile] = total != 0u ? 1u : 0u;
    a.flags[a.p.TT + tile] = 0u;
    if (total) atomicAdd(&a.count[0], total);
  }
}

// tile_fixed_point's rule for G12: a frontier cell's label becomes the least label among itself and its eight neighbours
struct LabelRule {
  struct Cell {};
  __device__ __forceinline__ void stage(int, bool, int) const {}
  __device__ __forceinline__ void prepare(int, Cell&) const {}
  __device__ __forceinline__ bool idle(unsigned mine) const { return mine == kInf; }   // not a frontier cell: it has no label and hands none on
  __device__ __forceinline__ unsigned lower(const Cell&, int c, unsigned best, const unsigned* s_l) const {
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx)
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy) {
        const unsigned v = s_l[c + dx * kHalo + dy];   // (UNREACHED is the largest value there is)
        best = v < best ? v : best;
      }
    return best;
  }
};

__global__ __launch_bounds__(kThreads) void nav_frontier_label(TileArgs a) {
  __shared__ unsigned s_l[kHalo * kHalo];
  __shared__ unsigned s_wake;
  tile_fixed_point(a, s_l, &s_wake, LabelRule{});
}

// G12's sizes: one integer add per frontier cell into its cluster's root — order-free, hence exact
__global__ void nav_frontier_sizes(const unsigned* __restrict__ label, int n, unsigned* __restrict__ size) {
  const int stride = gridDim.x * blockDim.x;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const unsigned l = label[i];
    if (l != kInf) atomicAdd(&size[l], 1u);
  }
}

// G13: a thread per bit of seed[nx][tiles_y]; a wave's ballot is two of its words.  count[1..3] += clusters, seed clusters, seed cells.
__global__ __launch_bounds__(kThreads) void nav_frontier_seeds(const unsigned* __restrict__ label, const unsigned* __restrict__ size, int nx, int ny,
                                                                  int tiles_y, unsigned min_cells, unsigned* __restrict__ seed, unsigned* __restrict__ count) {
  __shared__ unsigned s_c[3];
  const int tid = threadIdx.x, lane = tid & 63;
  if (tid < 3) s_c[tid] = 0u;
  __syncthreads();
  const int gid = blockIdx.x * kThreads + tid, word = gid >> 5, words = nx * tiles_y;
  const int ix = word / tiles_y, iy = (word - ix * tiles_y) * kTile + (gid & 31);
  const bool in = word < words && iy < ny;
  const unsigned cell = (unsigned)(ix * ny + iy);
  const unsigned l = in ? label[cell] : kInf;
  const bool is_seed = l != kInf && size[l] >= min_cells, is_root = l != kInf && l == cell;
  const unsigned long long bs = __ballot(is_seed), br = __ballot(is_root), bsr = __ballot(is_root && is_seed);
  if (lane == 0) {
    if (word < words) seed[word] = (unsigned)bs;
    if (word + 1 < words) seed[word + 1] = (unsigned)(bs >> 32);
    if (br) atomicAdd(&s_c[0], (unsigned)__popcll(br));
    if (bsr) atomicAdd(&s_c[1], (unsigned)__popcll(bsr));
    if (bs) atomicAdd(&s_c[2], (unsigned)__popcll(bs));
  }
  __syncthreads();
  if (tid < 3 && s_c[tid]) atomicAdd(&count[1 + tid], s_c[tid]);
}

// A solve's start from many goals: d = 0 at the goals and UNREACHED elsewhere, and active in round 0 every tile that SEES a goal in its
// interior or halo (nav_reset's rule).  The goals are the set bits of `seed` ([nx][tiles_y]), or, where `cells` is given, the n_cells
// listed pairs; the host has zeroed `flags` before, and with a list it has filled d with UNREACHED.
__global__ void nav_reset_goals(unsigned* __restrict__ d, int nx, int ny, int tiles_y, const unsigned* __restrict__ seed, const int* __restrict__ cells,
                                int n_cells, unsigned* __restrict__ flags) {
  const int stride = gridDim.x * blockDim.x, total = cells ? n_cells : nx * ny;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    int gx, gy;
    if (cells) {
      gx = cells[2 * i]; gy = cells[2 * i + 1];
      d[gx * ny + gy] = 0u;
    } else {
      gx = i / ny; gy = i - gx * ny;
      const bool goal = (seed[gx * tiles_y + (gy >> 5)] >> (gy & 31)) & 1u;
      d[i] = goal ? 0u : kInf;
      if (!goal) continue;
    }
    // the tiles whose interior or halo holds (gx, gy) are those of gx - 1, gx, gx + 1 by gy - 1, gy, gy + 1 (every writer stores the same 1)
    for (int dx = -1; dx <= 1; ++dx)
      for (int dy = -1; dy <= 1; ++dy) {
        const int x = gx + dx, y = gy + dy;
        if (x >= 0 && x < nx && y >= 0 && y < ny) flags[(x >> 5) * tiles_y + (y >> 5)] = 1u;
      }
  }
}

}  // namespace tbnav_nk

using namespace tbnav_nk;

namespace {

const char kFrontierKernels[] = "nav_frontier_mark;nav_frontier_label;nav_frontier_sizes;nav_frontier_seeds";

void visited_host(tbnav_nav* h) { if (h->visited.empty()) h->visited.assign(mask_words(h), 0u); }

// the device side of G10-G16, at the first call that needs it (the handle's device is current)
int ensure_buffers(tbnav_nav* h) {
  if (h->d_fcount) return TBNAV_OK;
  const size_t tiles = (size_t)h->tiles_x * h->tiles_y;
  TBNAV_HIP(dev_alloc(h, h->d_front, mask_words(h)));
  TBNAV_HIP(dev_alloc(h, h->d_seed, mask_words(h)));
  TBNAV_HIP(dev_alloc(h, h->d_visited, mask_words(h)));
  TBNAV_HIP(dev_alloc(h, h->d_label, (size_t)h->n));
  TBNAV_HIP(dev_alloc(h, h->d_size, (size_t)h->n));
  TBNAV_HIP(dev_alloc(h, h->d_fflags, 2 * tiles));
  TBNAV_HIP(dev_alloc(h, h->d_frec, 2 * (size_t)kMaxBatch));
  TBNAV_HIP(dev_alloc(h, h->d_fcount, 4));   // (the last: what it holds says that all of them stand)
  h->visited_dirty = true;
  return TBNAV_OK;
}

}  // namespace

// G13, with the stages' times where they are asked for (ms[4]: mark, label rounds with the host's reads, sizes, seeds)
int tbnav_nk::find_frontiers(tbnav_nav* h, tbnav_rbpf* pf, int32_t particle, int32_t min_cells, tbnav_nav_frontier_info* info, float* ms) {
  if (!h || !pf || !particle_ok(pf, particle) || min_cells < 1 || !h->cost_set) return TBNAV_ERR_INVALID_ARG;
  int rc = same_grid(h, pf);
  if (rc != TBNAV_OK) return rc;
  tbnav::DeviceGuard guard(pf->device);
  if (!guard.ok) return TBNAV_ERR_NO_DEVICE;
  rc = ensure_buffers(h);
  if (rc != TBNAV_OK) return rc;
  hipStream_t st = pf->stream;   // G9: behind whatever the filter has in flight
  visited_host(h);
  if (h->visited_dirty) {
    TBNAV_HIP(hipMemcpyAsync(h->d_visited, h->visited.data(), sizeof(unsigned) * mask_words(h), hipMemcpyHostToDevice, st));
    TBNAV_HIP(hipStreamSynchronize(st));   // (the host vector may change as soon as this call returns)
    h->visited_dirty = false;
  }
  StageTimer timer(ms != nullptr, 5, st);
  TBNAV_HIP(timer.create());
  h->finfo.found = 0; h->label_host_valid = false;   // from here on the last find's results are being overwritten
  h->ginfo = tbnav_nav_gain_info{0, 0, 0, 0, 0, 0, {-1, -1}}; h->gain_rmax = 0; h->gain_host_valid = false;   // (G19: the gain belonged to that find)
  TBNAV_HIP(hipMemsetAsync(h->d_fcount, 0, sizeof(unsigned) * 4, st));
  rc = enqueue_best(pf, particle);
  if (rc != TBNAV_OK) return rc;
  TBNAV_HIP(timer.stamp(0));
  const FrontierArgs fa{pf->pool.lo, particle_ref(pf, particle), pf->cuts.half_lo, pf->cuts.half_hi, pf->cuts.free_cut, h->d_cost, h->d_visited,
                        h->d_front, h->d_label, h->d_size, h->d_fflags, h->d_fcount};
  hipLaunchKernelGGL(nav_frontier_mark, dim3(pf->TW, pf->TW), dim3(kThreads), 0, st, fa);
  TBNAV_HIP(hipGetLastError());
  TBNAV_HIP(timer.stamp(1));
  int rounds = 0, launches = 0;
  long long visits = 0;
  rc = run_rounds(h, h->d_fflags, h->d_frec, st, [&](unsigned* cur, unsigned* nxt, unsigned* rec) {
    const TileArgs la{h->d_label, cur, nxt, rec, h->p.nx, h->p.ny, h->tiles_y};
    hipLaunchKernelGGL(nav_frontier_label, dim3(h->tiles_y, h->tiles_x), dim3(kThreads), 0, st, la);
  }, &rounds, &launches, &visits);
  if (rc != TBNAV_OK) return rc;
  TBNAV_HIP(timer.stamp(2));
  hipLaunchKernelGGL(nav_frontier_sizes, dim3(256), dim3(256), 0, st, h->d_label, h->n, h->d_size);
  TBNAV_HIP(hipGetLastError());
  TBNAV_HIP(timer.stamp(3));
  const int bits = (int)mask_words(h) * kTile;
  hipLaunchKernelGGL(nav_frontier_seeds, dim3((bits + kThreads - 1) / kThreads), dim3(kThreads), 0, st, h->d_label, h->d_size, h->p.nx, h->p.ny,
                     h->tiles_y, (unsigned)min_cells, h->d_seed, h->d_fcount);
  TBNAV_HIP(hipGetLastError());
  TBNAV_HIP(timer.stamp(4));
  unsigned cnt[4] = {0, 0, 0, 0};
  TBNAV_HIP(hipMemcpyAsync(cnt, h->d_fcount, sizeof cnt, hipMemcpyDeviceToHost, st));
  TBNAV_HIP(hipStreamSynchronize(st));
  for (int i = 0; ms && i < 4; ++i) { ms[i] = 0.0f; (void)timer.elapsed(i, &ms[i]); }
  h->finfo = tbnav_nav_frontier_info{1, min_cells, (int32_t)cnt[0], (int32_t)cnt[1], (int32_t)cnt[2], (int32_t)cnt[3], rounds, launches, visits};
  h->found_cost_epoch = h->cost_epoch; h->found_visited_epoch = h->visited_epoch;
  if (info) *info = h->finfo;
  return TBNAV_OK;
}

namespace {

// d_d and d_flags from the goals (the seed bits, or d_goals' n_cells pairs), then the rounds (the handle's device is current)
int solve_from_goals(tbnav_nav* h, int n_cells, int goal_ix, int goal_iy) {
  h->solved = false; h->d_host_valid = false;   // from here on the last solution is being overwritten
  const size_t tiles = (size_t)h->tiles_x * h->tiles_y;
  TBNAV_HIP(hipMemsetAsync(h->d_flags, 0, sizeof(unsigned) * 2 * tiles, nullptr));
  if (n_cells) TBNAV_HIP(hipMemsetAsync(h->d_d, 0xFF, sizeof(unsigned) * (size_t)h->n, nullptr));
  hipLaunchKernelGGL(nav_reset_goals, dim3(256), dim3(256), 0, nullptr, h->d_d, h->p.nx, h->p.ny, h->tiles_y, h->d_seed, n_cells ? h->d_goals : nullptr,
                     n_cells, h->d_flags);
  TBNAV_HIP(hipGetLastError());
  return relax_from_start(h, goal_ix, goal_iy);
}

}  // namespace

extern "C" {

int tbnav_nav_find_frontiers(tbnav_nav* h, tbnav_rbpf* pf, int32_t particle, int32_t min_cells, tbnav_nav_frontier_info* info) {
  return find_frontiers(h, pf, particle, min_cells, info, nullptr);
}

int tbnav_nav_profile_find_frontiers(tbnav_nav* h, tbnav_rbpf* pf, int32_t particle, int32_t min_cells, tbnav_nav_frontier_info* info, float* stage_ms) {
  if (!stage_ms) return TBNAV_ERR_INVALID_ARG;
  return find_frontiers(h, pf, particle, min_cells, info, stage_ms);
}

int tbnav_nav_last_frontiers(const tbnav_nav* h, tbnav_nav_frontier_info* info) {
  if (!h || !info) return TBNAV_ERR_INVALID_ARG;
  *info = h->finfo;
  return TBNAV_OK;
}

int tbnav_nav_last_frontier_kernels(const tbnav_nav* h, char* kernels, int32_t kernels_cap) {
  if (!h || !kernels || kernels_cap <= 0) return TBNAV_ERR_INVALID_ARG;
  std::snprintf(kernels, (size_t)kernels_cap, "%s", h->finfo.found ? kFrontierKernels : "");
  return TBNAV_OK;
}

int tbnav_nav_mark_visited(tbnav_nav* h, int32_t ix, int32_t iy, int32_t radius_cells) {
  if (!h || !in_grid(h, ix, iy) || radius_cells < 0 || radius_cells > TBNAV_NAV_MAX_VISIT_RADIUS) return TBNAV_ERR_INVALID_ARG;
  visited_host(h);
  const int r = radius_cells;
  for (int dx = -r; dx <= r; ++dx)
    for (int dy = -r; dy <= r; ++dy) {
      const int x = ix + dx, y = iy + dy;
      if (dx * dx + dy * dy <= r * r && in_grid(h, x, y)) h->visited[(size_t)x * h->tiles_y + (y >> 5)] |= 1u << (y & 31);
    }
  h->visited_dirty = true; ++h->visited_epoch;
  return TBNAV_OK;
}

int tbnav_nav_clear_visited(tbnav_nav* h) {
  if (!h) return TBNAV_ERR_INVALID_ARG;
  h->visited.assign(mask_words(h), 0u);
  h->visited_dirty = true; ++h->visited_epoch;
  return TBNAV_OK;
}

int tbnav_nav_get_visited(tbnav_nav* h, uint8_t* visited_host_out) {
  if (!h || !visited_host_out) return TBNAV_ERR_INVALID_ARG;
  visited_host(h);
  for (int x = 0; x < h->p.nx; ++x)
    for (int y = 0; y < h->p.ny; ++y) visited_host_out[(size_t)x * h->p.ny + y] = (uint8_t)((h->visited[(size_t)x * h->tiles_y + (y >> 5)] >> (y & 31)) & 1u);
  return TBNAV_OK;
}

int tbnav_nav_get_frontier_labels(tbnav_nav* h, uint32_t* labels_host) {
  if (!h || !labels_host || !h->finfo.found) return TBNAV_ERR_INVALID_ARG;
  const int rc = fetch_once(h, h->d_label, h->label_host, h->label_host_valid);
  if (rc != TBNAV_OK) return rc;
  std::memcpy(labels_host, h->label_host.data(), sizeof(uint32_t) * (size_t)h->n);
  return TBNAV_OK;
}

int tbnav_nav_frontier_list(tbnav_nav* h, tbnav_nav_frontier* out, int32_t cap, int32_t* n) {
  if (!h || !n || cap < 0 || (cap > 0 && !out) || !h->finfo.found) return TBNAV_ERR_INVALID_ARG;
  const int rc = fetch_once(h, h->d_label, h->label_host, h->label_host_valid);
  if (rc != TBNAV_OK) return rc;
  *n = h->finfo.clusters;
  if (cap < h->finfo.clusters) return TBNAV_ERR_INVALID_ARG;
  // a root is its cluster's least index, so the walk meets it before any other cell of the cluster, and the roots in ascending order
  std::vector<int32_t> slot((size_t)h->n, -1);
  const int ny = h->p.ny;
  int32_t k = 0;
  for (int i = 0; i < h->n; ++i) {
    const unsigned l = h->label_host[(size_t)i];
    if (l == kInf) continue;
    const int ix = i / ny, iy = i - ix * ny;
    if (l == (unsigned)i) {
      if (k >= cap) return TBNAV_ERR_UNSUPPORTED;   // (more roots than the device counted: cannot happen after a find)
      slot[(size_t)i] = k;
      out[k++] = tbnav_nav_frontier{{ix, iy}, 0, 0, {ix, iy, ix, iy}, 0, 0};
    }
    const int32_t s = slot[(size_t)l];
    if (s < 0) return TBNAV_ERR_UNSUPPORTED;        // (a label that is no root: not a fixed point of G12)
    tbnav_nav_frontier& f = out[s];
    ++f.size;
    f.box[0] = ix < f.box[0] ? ix : f.box[0]; f.box[1] = iy < f.box[1] ? iy : f.box[1];
    f.box[2] = ix > f.box[2] ? ix : f.box[2]; f.box[3] = iy > f.box[3] ? iy : f.box[3];
    f.sum_ix += ix; f.sum_iy += iy;
  }
  for (int32_t s = 0; s < k; ++s) out[s].seeds = out[s].size >= h->finfo.min_cells ? 1 : 0;
  return TBNAV_OK;
}

int tbnav_nav_solve_goals(tbnav_nav* h, const int32_t* cells, int32_t n) {
  if (!h || !cells || n < 1 || !h->cost_set) return TBNAV_ERR_INVALID_ARG;
  for (int i = 0; i < n; ++i) if (!in_grid(h, cells[2 * i], cells[2 * i + 1])) return TBNAV_ERR_INVALID_ARG;
  tbnav::DeviceGuard guard(h->device);
  if (!guard.ok) return TBNAV_ERR_NO_DEVICE;
  int rc = fetch_once(h, h->d_cost, h->cost, h->cost_host_valid);   // a grid set on the device: fetched to look at the goals' cells
  if (rc != TBNAV_OK) return rc;
  for (int i = 0; i < n; ++i) if (h->cost[(size_t)cells[2 * i] * h->p.ny + cells[2 * i + 1]] == 0) return TBNAV_ERR_INVALID_ARG;
  rc = ensure_buffers(h);
  if (rc != TBNAV_OK) return rc;
  if (n > h->goals_cap) {
    TBNAV_HIP(dev_alloc(h, h->d_goals, 2 * (size_t)n));
    h->goals_cap = n;
  }
  TBNAV_HIP(hipMemcpy(h->d_goals, cells, sizeof(int) * 2 * (size_t)n, hipMemcpyHostToDevice));
  return solve_from_goals(h, n, cells[0], cells[1]);
}

int tbnav_nav_solve_frontiers(tbnav_nav* h) {
  if (!h || !h->finfo.found || h->found_cost_epoch != h->cost_epoch || h->found_visited_epoch != h->visited_epoch) return TBNAV_ERR_INVALID_ARG;
  if (h->finfo.seed_cells == 0) return TBNAV_ERR_UNSUPPORTED;   // nothing left to explore
  tbnav::DeviceGuard guard(h->device);
  if (!guard.ok) return TBNAV_ERR_NO_DEVICE;
  return solve_from_goals(h, 0, -1, -1);
}

}  // extern "C"

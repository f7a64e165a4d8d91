// nav_frontier.hip — exploration frontiers of a filter particle's map as goals of the goal field (tbnav_nav.h G10-G16).  On the device:
// the frontier bits of every 32 x 32 tile from the particle's log-odds (nav_frontier_mark), their 8-connected clusters by minimum-label
// propagation in the shape of nav_relax_tiles (nav_frontier_label), the clusters' sizes and the seed bits (nav_frontier_sizes,
// nav_frontier_seeds), and the start of a solve from many goals (nav_reset_goals).  On the host: the visited mask (G14), the list of
// clusters (G16), and the calls' checks.  Integers and comparisons only; compiled without contraction like the rest of the planner.
#include <cstring>
#include <vector>

#include "rbpf_host.hpp"
#include "nav_host.hpp"

namespace tbnav_nk {

constexpr int kFrTile = 32;                    // cells per tile side: a tile of the filter's pool, and of nav_relax_tiles
constexpr int kFrHalo = kFrTile + 2;
constexpr int kFrThreads = 256;                // four waves; a wave's 64 lanes are two rows of 32 consecutive iy, so one ballot is two row words
constexpr int kFrOwn = kFrTile * kFrTile / kFrThreads;
constexpr int kFrRowStep = kFrThreads / kFrTile;
constexpr int kFrMaxSweeps = 4 * kFrTile;      // nav_relax_tiles's bound: a chain that winds through a tile runs into it and the tile stays active
constexpr unsigned kFrNone = TBNAV_NAV_UNREACHED;
constexpr int kFrSelfBit = 4, kFrChangedBit = 9;   // a tile's wake word, as in nav.hip
static_assert(kFrTile == tbnav_rk::kTS, "a workgroup's tile is a tile of the filter's pool");

struct FrontierArgs {
  const double* lo;            // TilePool::lo
  const unsigned int* table;   // [N][TT] the particles' tile tables
  const int* best;             // where the particle's index is on the device (rbpf_argmax), or null: `particle`
  int particle;
  int TW, TT;                  // tiles per side, per map
  int side;                    // cells per side of the map and of the nav grid (G8)
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
__global__ __launch_bounds__(kFrThreads) void nav_frontier_mark(FrontierArgs a) {
  __shared__ unsigned int s_unk[kFrHalo];      // UNKNOWN bits of rows -1 .. 32 (own columns)
  __shared__ unsigned int s_free[kFrTile], s_pass[kFrTile], s_front[kFrTile];
  __shared__ unsigned int s_side[2];           // bit r: the cell left (iy = -1) / right (iy = 32) of row r is UNKNOWN
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tile_x = blockIdx.y, tile_y = blockIdx.x, tile = tile_x * a.TW + tile_y;
  const int p = a.best ? *a.best : a.particle;
  const unsigned int* __restrict__ tab_p = a.table + (size_t)p * a.TT;
  const unsigned int id = tab_p[tile];
  const int lx0 = tid >> 5, ly = tid & (kFrTile - 1), gy = tile_y * kFrTile + ly;
  if (id == 0u) {   // nobody has written this tile: unknown throughout, so no cell of it is FREE, whatever lies next door
#pragma unroll
    for (int j = 0; j < kFrOwn; ++j) {
      const int gx = tile_x * kFrTile + lx0 + j * kFrRowStep;
      if (gx < a.side && gy < a.side) { a.label[(size_t)gx * a.side + gy] = kFrNone; a.size[(size_t)gx * a.side + gy] = 0u; }
    }
    if (tid < kFrTile && tile_x * kFrTile + tid < a.side) a.front[(size_t)(tile_x * kFrTile + tid) * a.TW + tile_y] = 0u;
    if (tid == 0) { a.flags[tile] = 0u; a.flags[a.TT + tile] = 0u; }
    return;
  }
  // the tile's own 1024 log-odds, classified; a cell of a ragged last tile that is outside the map has no class
  const double* __restrict__ t_lo = a.lo + (size_t)id * (kFrTile * kFrTile);
#pragma unroll
  for (int j = 0; j < kFrOwn; ++j) {
    const int r = lx0 + j * kFrRowStep, gx = tile_x * kFrTile + r;
    const bool in = gx < a.side && gy < a.side;
    const double l = t_lo[r * kFrTile + ly];
    const unsigned long long bu = __ballot(in && l >= a.half_lo && l <= a.half_hi);
    const unsigned long long bf = __ballot(in && l <= a.free_cut);
    const unsigned long long bp = __ballot(in && a.cost[in ? (size_t)gx * a.side + gy : 0] != 0);
    if (lane == 0) {   // (lane 0's row is the even one of the wave's two)
      s_unk[1 + r] = (unsigned int)bu; s_unk[2 + r] = (unsigned int)(bu >> 32);
      s_free[r] = (unsigned int)bf; s_free[r + 1] = (unsigned int)(bf >> 32);
      s_pass[r] = (unsigned int)bp; s_pass[r + 1] = (unsigned int)(bp >> 32);
    }
  }
  // the facing row of the tiles above and below (wave 0) and the facing column of the tiles left and right (wave 1)
  if (wave == 0) {
    const bool up = lane < kFrTile;
    const int gx = up ? tile_x * kFrTile - 1 : tile_x * kFrTile + kFrTile, gyy = tile_y * kFrTile + (lane & (kFrTile - 1));
    bool u = false;
    if (gx >= 0 && gx < a.side && gyy < a.side) {
      const unsigned int nid = tab_p[(gx >> 5) * a.TW + tile_y];
      u = true;
      if (nid != 0u) { const double l = a.lo[(size_t)nid * (kFrTile * kFrTile) + (gx & (kFrTile - 1)) * kFrTile + (lane & (kFrTile - 1))]; u = l >= a.half_lo && l <= a.half_hi; }
    }
    const unsigned long long b = __ballot(u);
    if (lane == 0) { s_unk[0] = (unsigned int)b; s_unk[kFrHalo - 1] = (unsigned int)(b >> 32); }
  } else if (wave == 1) {
    const bool left = lane < kFrTile;
    const int r = lane & (kFrTile - 1), gx = tile_x * kFrTile + r, gyy = left ? tile_y * kFrTile - 1 : tile_y * kFrTile + kFrTile;
    bool u = false;
    if (gyy >= 0 && gyy < a.side && gx < a.side) {
      const unsigned int nid = tab_p[tile_x * a.TW + (gyy >> 5)];
      u = true;
      if (nid != 0u) { const double l = a.lo[(size_t)nid * (kFrTile * kFrTile) + r * kFrTile + (gyy & (kFrTile - 1))]; u = l >= a.half_lo && l <= a.half_hi; }
    }
    const unsigned long long b = __ballot(u);
    if (lane == 0) { s_side[0] = (unsigned int)b; s_side[1] = (unsigned int)(b >> 32); }
  }
  __syncthreads();
  // G11, a row per thread: FREE, passable, not visited, and UNKNOWN above, below, left or right
  if (tid < kFrTile) {
    const int r = tid, gx = tile_x * kFrTile + r;
    const unsigned int u = s_unk[1 + r];
    const unsigned int near = s_unk[r] | s_unk[2 + r] | (u << 1) | ((s_side[0] >> r) & 1u) | (u >> 1) | (((s_side[1] >> r) & 1u) << 31);
    unsigned int f = s_free[r] & s_pass[r] & near;
    if (gx < a.side) {
      f &= ~a.visited[(size_t)gx * a.TW + tile_y];
      a.front[(size_t)gx * a.TW + tile_y] = f;
    }
    s_front[r] = f;   // (a row outside the map has no FREE cell: f is 0 there)
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kFrOwn; ++j) {
    const int r = lx0 + j * kFrRowStep, gx = tile_x * kFrTile + r;
    if (gx < a.side && gy < a.side) {
      const unsigned int g = (unsigned int)gx * (unsigned int)a.side + (unsigned int)gy;
      a.label[g] = (s_front[r] >> ly) & 1u ? g : kFrNone;
      a.size[g] = 0u;
    }
  }
  if (tid == 0) {
    unsigned int total = 0u;
    for (int r = 0; r < kFrTile; ++r) total += __popc(s_front[r]);
    a.flags[tile] = total != 0u ? 1u : 0u;
    a.flags[a.TT + tile] = 0u;
    if (total) atomicAdd(&a.count[0], total);
  }
}

struct LabelArgs {
  unsigned* label;       // [nx][ny]
  unsigned* cur;         // [tiles_x][tiles_y] 1 = active this round (cleared by the workgroup that takes the tile)
  unsigned* nxt;         // ... next round
  unsigned* rec;         // this round's record: [0] tiles visited, [1] tiles in which something changed
  int nx, ny, tiles_y;
};

// G12: a frontier cell's label becomes the least label among itself and its eight neighbours, until nothing changes.  nav_relax_tiles
// with min in place of min-plus: a thread owns its cells and only ever lowers them, so stale reads of a neighbour are harmless, the
// fixed point — every cell of a component holding the component's least index — is unique, and no atomics are needed on the labels.
__global__ __launch_bounds__(kFrThreads) void nav_frontier_label(LabelArgs a) {
  __shared__ unsigned s_l[kFrHalo * kFrHalo];
  __shared__ unsigned s_wake;
  const int tile_x = blockIdx.y, tile_y = blockIdx.x, tile = tile_x * a.tiles_y + tile_y;
  if (a.cur[tile] == 0) return;   // (the whole workgroup alike)
  const int tid = threadIdx.x;
  const int x0 = tile_x * kFrTile - 1, y0 = tile_y * kFrTile - 1;   // the grid cell of LDS cell (0, 0)
  for (int i = tid; i < kFrHalo * kFrHalo; i += kFrThreads) {
    const int lx = i / kFrHalo, ly = i - lx * kFrHalo, gx = x0 + lx, gy = y0 + ly;
    const bool in = gx >= 0 && gx < a.nx && gy >= 0 && gy < a.ny;
    s_l[i] = in ? a.label[gx * a.ny + gy] : kFrNone;
  }
  if (tid == 0) s_wake = 0;
  __syncthreads();

  const int c0 = (1 + (tid >> 5)) * kFrHalo + 1 + (tid & 31);
  unsigned mine[kFrOwn], first[kFrOwn];
#pragma unroll
  for (int j = 0; j < kFrOwn; ++j) first[j] = mine[j] = s_l[c0 + j * kFrRowStep * kFrHalo];

  int more = 1;
  for (int s = 0; s < kFrMaxSweeps && more; ++s) {
    int changed = 0;
#pragma unroll
    for (int j = 0; j < kFrOwn; ++j) {
      if (mine[j] == kFrNone) continue;   // not a frontier cell: it has no label and hands none on
      const int c = c0 + j * kFrRowStep * kFrHalo;
      unsigned best = mine[j];
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx)
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
          const unsigned v = s_l[c + dx * kFrHalo + dy];   // (UNREACHED is the largest value there is)
          best = v < best ? v : best;
        }
      if (best < mine[j]) { mine[j] = best; s_l[c] = best; changed = 1; }
    }
    more = __syncthreads_or(changed);
  }

  unsigned wake = more ? 1u << kFrSelfBit : 0u;   // the sweep bound was hit: this tile stays active
#pragma unroll
  for (int j = 0; j < kFrOwn; ++j) {
    if (mine[j] != first[j]) {   // (only a cell inside the grid ever changes)
      const int ix = (tid >> 5) + j * kFrRowStep, iy = tid & 31;
      a.label[(x0 + 1 + ix) * a.ny + (y0 + 1 + iy)] = mine[j];
      const int ex = ix == 0 ? -1 : (ix == kFrTile - 1 ? 1 : 0), ey = iy == 0 ? -1 : (iy == kFrTile - 1 ? 1 : 0);
      wake |= 1u << kFrChangedBit;
      if (ex != 0) wake |= 1u << ((ex + 1) * 3 + 1);
      if (ey != 0) wake |= 1u << (3 + ey + 1);
      if (ex != 0 && ey != 0) wake |= 1u << ((ex + 1) * 3 + ey + 1);
    }
  }
  if (wake) atomicOr(&s_wake, wake);
  __syncthreads();
  const unsigned w = s_wake;
  if (tid < 9 && ((w >> tid) & 1u)) {
    const int tx = tile_x + tid / 3 - 1, ty = tile_y + tid % 3 - 1;
    if (tx >= 0 && tx < (int)gridDim.y && ty >= 0 && ty < a.tiles_y) a.nxt[tx * a.tiles_y + ty] = 1u;
  }
  if (tid == 0) {
    a.cur[tile] = 0;
    atomicAdd(&a.rec[0], 1u);
    if (w >> kFrSelfBit & 1u || w >> kFrChangedBit & 1u) atomicAdd(&a.rec[1], 1u);
  }
}

// G12's sizes: one integer add per frontier cell into its cluster's root — order-free, hence exact
__global__ void nav_frontier_sizes(const unsigned* __restrict__ label, int n, unsigned* __restrict__ size) {
  const int stride = gridDim.x * blockDim.x;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const unsigned l = label[i];
    if (l != kFrNone) atomicAdd(&size[l], 1u);
  }
}

// G13: a thread per bit of seed[nx][tiles_y]; a wave's ballot is two of its words.  count[1..3] += clusters, seed clusters, seed cells.
__global__ __launch_bounds__(kFrThreads) void nav_frontier_seeds(const unsigned* __restrict__ label, const unsigned* __restrict__ size, int nx, int ny,
                                                                  int tiles_y, unsigned min_cells, unsigned* __restrict__ seed, unsigned* __restrict__ count) {
  __shared__ unsigned s_c[3];
  const int tid = threadIdx.x, lane = tid & 63;
  if (tid < 3) s_c[tid] = 0u;
  __syncthreads();
  const int gid = blockIdx.x * kFrThreads + tid, word = gid >> 5, words = nx * tiles_y;
  const int ix = word / tiles_y, iy = (word - ix * tiles_y) * kFrTile + (gid & 31);
  const bool in = word < words && iy < ny;
  const unsigned cell = (unsigned)(ix * ny + iy);
  const unsigned l = in ? label[cell] : kFrNone;
  const bool is_seed = l != kFrNone && size[l] >= min_cells, is_root = l != kFrNone && l == cell;
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
      d[i] = goal ? 0u : kFrNone;
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

bool in_grid(const tbnav_nav* h, int ix, int iy) { return ix >= 0 && ix < h->p.nx && iy >= 0 && iy < h->p.ny; }
size_t mask_words(const tbnav_nav* h) { return (size_t)h->p.nx * h->tiles_y; }
void visited_host(tbnav_nav* h) { if (h->visited.empty()) h->visited.assign(mask_words(h), 0u); }

// the device side of G10-G16, at the first call that needs it (the handle's device is current)
int ensure_buffers(tbnav_nav* h) {
  if (h->d_fcount) return TBNAV_OK;
  const size_t tiles = (size_t)h->tiles_x * h->tiles_y;
  TBNAV_HIP(hipMalloc((void**)&h->d_front, sizeof(unsigned) * mask_words(h)));
  TBNAV_HIP(hipMalloc((void**)&h->d_seed, sizeof(unsigned) * mask_words(h)));
  TBNAV_HIP(hipMalloc((void**)&h->d_visited, sizeof(unsigned) * mask_words(h)));
  TBNAV_HIP(hipMalloc((void**)&h->d_label, sizeof(unsigned) * (size_t)h->n));
  TBNAV_HIP(hipMalloc((void**)&h->d_size, sizeof(unsigned) * (size_t)h->n));
  TBNAV_HIP(hipMalloc((void**)&h->d_fflags, sizeof(unsigned) * 2 * tiles));
  TBNAV_HIP(hipMalloc((void**)&h->d_frec, sizeof(unsigned) * 2 * kMaxBatch));
  TBNAV_HIP(hipMalloc((void**)&h->d_fcount, sizeof(unsigned) * 4));
  h->visited_dirty = true;
  return TBNAV_OK;
}

// G13, with the stages' times where they are asked for (ms[4]: mark, label rounds with the host's reads, sizes, seeds)
int find(tbnav_nav* h, tbnav_rbpf* pf, int32_t particle, int32_t min_cells, tbnav_nav_frontier_info* info, float* ms) {
  if (!h || !pf || !(particle == TBNAV_NAV_BEST_PARTICLE || (particle >= 0 && particle < pf->N)) || min_cells < 1) return TBNAV_ERR_INVALID_ARG;
  if (h->p.nx != pf->xsize || h->p.ny != pf->xsize || pf->ysize != pf->xsize || h->p.xmin != pf->p.xmin || h->p.ymin != pf->p.ymin ||
      h->p.resolution != pf->p.resolution || !h->cost_set)
    return TBNAV_ERR_INVALID_ARG;
  if (h->device != pf->device) return TBNAV_ERR_UNSUPPORTED;
  tbnav::DeviceGuard guard(pf->device);
  if (!guard.ok) return TBNAV_ERR_NO_DEVICE;
  int rc = ensure_buffers(h);
  if (rc != TBNAV_OK) return rc;
  hipStream_t st = pf->stream;   // G9: behind whatever the filter has in flight
  visited_host(h);
  if (h->visited_dirty) {
    TBNAV_HIP(hipMemcpyAsync(h->d_visited, h->visited.data(), sizeof(unsigned) * mask_words(h), hipMemcpyHostToDevice, st));
    TBNAV_HIP(hipStreamSynchronize(st));   // (the host vector may change as soon as this call returns)
    h->visited_dirty = false;
  }
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  if (ms) for (auto& e : ev) TBNAV_HIP(hipEventCreate(&e));
  auto stamp = [&](int i) { return ms ? hipEventRecord(ev[i], st) : hipSuccess; };
  h->finfo.found = 0; h->label_host_valid = false;   // from here on the last find's results are being overwritten
  TBNAV_HIP(hipMemsetAsync(h->d_fcount, 0, sizeof(unsigned) * 4, st));
  if (particle == TBNAV_NAV_BEST_PARTICLE) {
    const StatePtrs sp = state_ptrs(pf->d_state[pf->cur], pf->N);
    hipLaunchKernelGGL(rbpf_argmax, dim3(1), dim3(256), 0, st, pf->N, sp.weight, sp.pose, pf->d_best, pf->d_best_pose);
    TBNAV_HIP(hipGetLastError());
  }
  TBNAV_HIP(stamp(0));
  const FrontierArgs fa{pf->pool.lo, pf->d_table[pf->cur], particle == TBNAV_NAV_BEST_PARTICLE ? pf->d_best : nullptr, particle, pf->TW, pf->TT,
                        pf->xsize, pf->cuts.half_lo, pf->cuts.half_hi, pf->cuts.free_cut, h->d_cost, h->d_visited, h->d_front, h->d_label,
                        h->d_size, h->d_fflags, h->d_fcount};
  hipLaunchKernelGGL(nav_frontier_mark, dim3(pf->TW, pf->TW), dim3(kFrThreads), 0, st, fa);
  TBNAV_HIP(hipGetLastError());
  TBNAV_HIP(stamp(1));
  int rounds = 0, launches = 0;
  long long visits = 0;
  rc = run_rounds(h, h->d_fflags, h->d_frec, st, [&](unsigned* cur, unsigned* nxt, unsigned* rec) {
    const LabelArgs la{h->d_label, cur, nxt, rec, h->p.nx, h->p.ny, h->tiles_y};
    hipLaunchKernelGGL(nav_frontier_label, dim3(h->tiles_y, h->tiles_x), dim3(kFrThreads), 0, st, la);
  }, &rounds, &launches, &visits);
  if (rc != TBNAV_OK) return rc;
  TBNAV_HIP(stamp(2));
  hipLaunchKernelGGL(nav_frontier_sizes, dim3(256), dim3(256), 0, st, h->d_label, h->n, h->d_size);
  TBNAV_HIP(hipGetLastError());
  TBNAV_HIP(stamp(3));
  const int bits = (int)mask_words(h) * kFrTile;
  hipLaunchKernelGGL(nav_frontier_seeds, dim3((bits + kFrThreads - 1) / kFrThreads), dim3(kFrThreads), 0, st, h->d_label, h->d_size, h->p.nx, h->p.ny,
                     h->tiles_y, (unsigned)min_cells, h->d_seed, h->d_fcount);
  TBNAV_HIP(hipGetLastError());
  TBNAV_HIP(stamp(4));
  unsigned cnt[4] = {0, 0, 0, 0};
  TBNAV_HIP(hipMemcpyAsync(cnt, h->d_fcount, sizeof cnt, hipMemcpyDeviceToHost, st));
  TBNAV_HIP(hipStreamSynchronize(st));
  if (ms) {
    for (int i = 0; i < 4; ++i) { ms[i] = 0.0f; (void)hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]); }
    for (auto& e : ev) (void)hipEventDestroy(e);
  }
  h->finfo = tbnav_nav_frontier_info{1, min_cells, (int32_t)cnt[0], (int32_t)cnt[1], (int32_t)cnt[2], (int32_t)cnt[3], rounds, launches, visits};
  h->found_cost_epoch = h->cost_epoch; h->found_visited_epoch = h->visited_epoch;
  if (info) *info = h->finfo;
  return TBNAV_OK;
}

int download_labels(tbnav_nav* h) {
  if (h->label_host_valid) return TBNAV_OK;
  tbnav::DeviceGuard guard(h->device);
  if (!guard.ok) return TBNAV_ERR_NO_DEVICE;
  h->label_host.resize((size_t)h->n);
  TBNAV_HIP(hipMemcpy(h->label_host.data(), h->d_label, sizeof(unsigned) * (size_t)h->n, hipMemcpyDeviceToHost));
  h->label_host_valid = true;
  return TBNAV_OK;
}

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
  return find(h, pf, particle, min_cells, info, nullptr);
}

int tbnav_nav_profile_find_frontiers(tbnav_nav* h, tbnav_rbpf* pf, int32_t particle, int32_t min_cells, tbnav_nav_frontier_info* info, float* stage_ms) {
  if (!stage_ms) return TBNAV_ERR_INVALID_ARG;
  return find(h, pf, particle, min_cells, info, stage_ms);
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
  const int rc = download_labels(h);
  if (rc != TBNAV_OK) return rc;
  std::memcpy(labels_host, h->label_host.data(), sizeof(uint32_t) * (size_t)h->n);
  return TBNAV_OK;
}

int tbnav_nav_frontier_list(tbnav_nav* h, tbnav_nav_frontier* out, int32_t cap, int32_t* n) {
  if (!h || !n || cap < 0 || (cap > 0 && !out) || !h->finfo.found) return TBNAV_ERR_INVALID_ARG;
  const int rc = download_labels(h);
  if (rc != TBNAV_OK) return rc;
  *n = h->finfo.clusters;
  if (cap < h->finfo.clusters) return TBNAV_ERR_INVALID_ARG;
  // a root is its cluster's least index, so the walk meets it before any other cell of the cluster, and the roots in ascending order
  std::vector<int32_t> slot((size_t)h->n, -1);
  const int ny = h->p.ny;
  int32_t k = 0;
  for (int i = 0; i < h->n; ++i) {
    const unsigned l = h->label_host[(size_t)i];
    if (l == kFrNone) continue;
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
  if (!h->cost_host_valid) {   // a grid set on the device: fetched to look at the goals' cells
    h->cost.resize((size_t)h->n);
    TBNAV_HIP(hipMemcpy(h->cost.data(), h->d_cost, (size_t)h->n, hipMemcpyDeviceToHost));
    h->cost_host_valid = true;
  }
  for (int i = 0; i < n; ++i) if (h->cost[(size_t)cells[2 * i] * h->p.ny + cells[2 * i + 1]] == 0) return TBNAV_ERR_INVALID_ARG;
  const int rc = ensure_buffers(h);
  if (rc != TBNAV_OK) return rc;
  if (n > h->goals_cap) {
    int* d_new = nullptr;
    TBNAV_HIP(hipMalloc((void**)&d_new, sizeof(int) * 2 * (size_t)n));
    (void)hipFree(h->d_goals);
    h->d_goals = d_new; h->goals_cap = n;
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

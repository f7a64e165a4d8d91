// nav.hip — the goal field of include/tbnav_nav.h (G1-G6): the exact integer cost-to-go to a goal cell over a cost grid, an OPTION the
// reference's controller does not have (its planner package, planner/src/planner/dstar_light.cpp:367-461, is never seen by MPPI).
// Here: the tiled label-correcting solver (nav_relax_tiles: one workgroup per ACTIVE 32 x 32 tile, relaxed in LDS to its own fixed
// point; a round is a launch, the host stops at the first round that changed nothing), the field kernel G5 (nav_field), the host
// walk G6, and the hand-over to an MPPI handle, device to device, through mppi_field.hip's setters (field_stage_device / field_commit).
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "mppi_host.hpp"
#include "nav_host.hpp"

namespace tbnav_nk {

constexpr int kTile = 32;                 // cells per tile side
constexpr int kHalo = kTile + 2;          // ... with the one-cell halo (G3: both orthogonal cells of a diagonal move out of the interior lie inside it)
constexpr int kThreads = 256;             // four waves; a wave's 64 lanes are two rows of 32 consecutive iy: no LDS bank is hit twice by a half
constexpr int kOwn = kTile * kTile / kThreads;   // cells a thread owns: rows (tid >> 5) + 8 j
constexpr int kRowStep = kThreads / kTile;
// Sweeps per visit.  A front crosses an open tile in at most kTile sweeps along an axis and kTile along the diagonal, so 4 * kTile
// leaves a tile of open space or plain walls converged in one visit; a labyrinth inside one tile (a path of up to kTile^2 cells)
// runs into the bound, writes back what it has and stays active for the next round.
constexpr int kMaxSweeps = 4 * kTile;
constexpr unsigned kInf = TBNAV_NAV_UNREACHED;
// G3's moves in the order of dstar_light.cpp:370-373 read as (dix, diy), and their w
constexpr int kDx[8] = {0, 0, -1, 1, -1, -1, 1, 1};
constexpr int kDy[8] = {-1, 1, 0, 0, -1, 1, -1, 1};
constexpr unsigned kW[8] = {10, 10, 10, 10, 14, 14, 14, 14};
// bits of a tile's wake word: 0..8 the tile at (dx + 1) * 3 + (dy + 1) — 4 is the tile itself —, 9: something in the tile changed
constexpr int kSelfBit = 4, kChangedBit = 9;

struct RelaxArgs {
  const uint8_t* cost;   // [nx][ny]
  unsigned* d;           // [nx][ny]
  unsigned* cur;         // [tiles_x][tiles_y] 1 = active this round (cleared by the workgroup that takes the tile)
  unsigned* nxt;         // ... next round (all zero when this round starts)
  unsigned* rec;         // this round's record: [0] tiles visited, [1] tiles in which something changed
  int nx, ny, tiles_y;
};

__global__ __launch_bounds__(kThreads) void nav_relax_tiles(RelaxArgs a) {
  __shared__ unsigned s_d[kHalo * kHalo];
  __shared__ uint8_t s_c[kHalo * kHalo];
  __shared__ unsigned s_wake;
  const int tile_x = blockIdx.y, tile_y = blockIdx.x, tile = tile_x * a.tiles_y + tile_y;
  if (a.cur[tile] == 0) return;   // (the whole workgroup alike)
  const int tid = threadIdx.x;
  const int x0 = tile_x * kTile - 1, y0 = tile_y * kTile - 1;   // the grid cell of LDS cell (0, 0)
  for (int i = tid; i < kHalo * kHalo; i += kThreads) {
    const int lx = i / kHalo, ly = i - lx * kHalo, gx = x0 + lx, gy = y0 + ly;
    const bool in = gx >= 0 && gx < a.nx && gy >= 0 && gy < a.ny;   // outside the grid: blocked, as G3 wants it
    const int g = gx * a.ny + gy;
    s_c[i] = in ? a.cost[g] : (uint8_t)0;
    s_d[i] = in ? a.d[g] : kInf;
  }
  if (tid == 0) s_wake = 0;
  __syncthreads();

  // a thread's cells, and for each the price of its eight moves (0: not allowed) — the costs are not read again
  const int c0 = (1 + (tid >> 5)) * kHalo + 1 + (tid & 31);
  unsigned wgt[kOwn][8], mine[kOwn], first[kOwn];
#pragma unroll
  for (int j = 0; j < kOwn; ++j) {
    const int c = c0 + j * kRowStep * kHalo;
    const unsigned ca = s_c[c];
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      const unsigned cb = s_c[c + kDx[m] * kHalo + kDy[m]];
      bool ok = ca != 0 && cb != 0;
      if (kDx[m] != 0 && kDy[m] != 0) ok = ok && s_c[c + kDy[m]] != 0 && s_c[c + kDx[m] * kHalo] != 0;
      wgt[j][m] = ok ? kW[m] * cb : 0u;
    }
    first[j] = mine[j] = s_d[c];
  }

  // Relax until a sweep lowers nothing.  A thread writes its own cells only and only lowers them, so whether a neighbour's value is
  // read before or after its owner's write of this sweep does not matter: min is monotone and the fixed point is unique.
  int more = 1;
  for (int s = 0; s < kMaxSweeps && more; ++s) {
    int changed = 0;
#pragma unroll
    for (int j = 0; j < kOwn; ++j) {
      const int c = c0 + j * kRowStep * kHalo;
      unsigned best = mine[j];
#pragma unroll
      for (int m = 0; m < 8; ++m) {
        const unsigned db = s_d[c + kDx[m] * kHalo + kDy[m]];
        const unsigned cand = db + wgt[j][m];   // (G4: no sum of a reached d and a price overflows)
        best = (db != kInf && wgt[j][m] != 0u && cand < best) ? cand : best;
      }
      if (best < mine[j]) { mine[j] = best; s_d[c] = best; changed = 1; }
    }
    more = __syncthreads_or(changed);
  }

  // the interior back (a cell outside the grid is blocked and never changes), and who has to look again
  unsigned wake = more ? 1u << kSelfBit : 0u;   // the sweep bound was hit: this tile stays active
#pragma unroll
  for (int j = 0; j < kOwn; ++j) {
    if (mine[j] != first[j]) {
      const int ix = (tid >> 5) + j * kRowStep, iy = tid & 31;   // 0 .. kTile-1
      a.d[(x0 + 1 + ix) * a.ny + (y0 + 1 + iy)] = mine[j];
      const int ex = ix == 0 ? -1 : (ix == kTile - 1 ? 1 : 0), ey = iy == 0 ? -1 : (iy == kTile - 1 ? 1 : 0);
      wake |= 1u << kChangedBit;
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
    a.cur[tile] = 0;   // (every wave has read it: two barriers ago)
    atomicAdd(&a.rec[0], 1u);
    if (w >> kSelfBit & 1u || w >> kChangedBit & 1u) atomicAdd(&a.rec[1], 1u);
  }
}

// a solve's start: d = UNREACHED but for the goal; active in round 0 is every tile that SEES the goal, in its interior or in its halo
// (a goal on its tile's rim whose neighbours inside the tile are all blocked changes nothing there, and still is news next door)
__global__ void nav_reset(unsigned* __restrict__ d, int n, int ny, int goal_ix, int goal_iy, unsigned* __restrict__ flags, int tiles, int tiles_y) {
  const int stride = gridDim.x * blockDim.x, goal = goal_ix * ny + goal_iy;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) d[i] = i == goal ? 0u : kInf;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < 2 * tiles; i += stride) {
    const int x0 = (i / tiles_y) * kTile - 1, y0 = (i % tiles_y) * kTile - 1;   // (meaningful for i < tiles: the even rounds' array)
    flags[i] = (i < tiles && goal_ix >= x0 && goal_ix < x0 + kHalo && goal_iy >= y0 && goal_iy < y0 + kHalo) ? 1u : 0u;
  }
}

// G5 (this file is compiled without contraction)
__global__ void nav_field(const unsigned* __restrict__ d, int n, double resolution, double cap, float* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned v = d[i];
  const double t = ((double)v * resolution) / 10.0;
  out[i] = (float)(v == kInf ? cap : (t < cap ? t : cap));
}

}  // namespace tbnav_nk

using namespace tbnav_nk;
using tbnav::DeviceGuard;

// the rounds of a solve (the batches and the stop rule: nav_host.hpp, run_rounds) and what a finished solve leaves in the handle
int tbnav_nk::relax_from_start(tbnav_nav* h, int goal_ix, int goal_iy) {
  int rounds = 0, launches = 0;
  long long visits = 0;
  const int rc = run_rounds(h, h->d_flags, h->d_rec, nullptr, [&](unsigned* cur, unsigned* nxt, unsigned* rec) {
    const RelaxArgs a{h->d_cost, h->d_d, cur, nxt, rec, h->p.nx, h->p.ny, h->tiles_y};
    hipLaunchKernelGGL(nav_relax_tiles, dim3(h->tiles_y, h->tiles_x), dim3(kThreads), 0, nullptr, a);
  }, &rounds, &launches, &visits);
  if (rc != TBNAV_OK) return rc;
  // what G6 walks over: the host copy where there is one, else kept on the device until a path is asked for
  if (h->cost_host_valid) h->cost_solved = h->cost;
  else TBNAV_HIP(hipMemcpy(h->d_cost_solved, h->d_cost, (size_t)h->n, hipMemcpyDeviceToDevice));
  h->cost_solved_valid = h->cost_host_valid;
  h->solved = true;
  h->info.solved = 1; h->info.goal[0] = goal_ix; h->info.goal[1] = goal_iy;
  h->info.rounds = rounds; h->info.launches = launches; h->info.tile_visits = visits;
  return TBNAV_OK;
}

namespace {
bool in_grid(const tbnav_nav* h, int ix, int iy) { return ix >= 0 && ix < h->p.nx && iy >= 0 && iy < h->p.ny; }

int download(tbnav_nav* h) {
  if (h->d_host_valid) return TBNAV_OK;
  DeviceGuard guard(h->device);
  if (!guard.ok) return TBNAV_ERR_NO_DEVICE;
  h->d_host.resize((size_t)h->n);
  TBNAV_HIP(hipMemcpy(h->d_host.data(), h->d_d, sizeof(unsigned) * (size_t)h->n, hipMemcpyDeviceToHost));
  h->d_host_valid = true;
  return TBNAV_OK;
}
int download_cost_solved(tbnav_nav* h) {
  if (h->cost_solved_valid) return TBNAV_OK;
  DeviceGuard guard(h->device);
  if (!guard.ok) return TBNAV_ERR_NO_DEVICE;
  h->cost_solved.resize((size_t)h->n);
  TBNAV_HIP(hipMemcpy(h->cost_solved.data(), h->d_cost_solved, (size_t)h->n, hipMemcpyDeviceToHost));
  h->cost_solved_valid = true;
  return TBNAV_OK;
}
bool cap_ok(double cap) { return std::isfinite(cap) && cap > 0.0; }
// G5 into d_field, finished when this returns (the nav handle's device is current)
int form_field(tbnav_nav* h, double cap) {
  hipLaunchKernelGGL(nav_field, dim3((h->n + 255) / 256), dim3(256), 0, nullptr, h->d_d, h->n, h->p.resolution, cap, h->d_field);
  TBNAV_HIP(hipGetLastError());
  TBNAV_HIP(hipDeviceSynchronize());
  return TBNAV_OK;
}
tbnav_mppi_cost_field geom_of(const tbnav_nav* h, double weight) {
  return tbnav_mppi_cost_field{h->p.nx, h->p.ny, h->p.xmin, h->p.ymin, h->p.resolution, weight};
}
}  // namespace

extern "C" {

int tbnav_nav_create(const tbnav_nav_params* params, tbnav_nav** out) {
  if (!params || !out) return TBNAV_ERR_INVALID_ARG;
  *out = nullptr;
  const tbnav_nav_params& p = *params;
  if (p.nx < 2 || p.nx > TBNAV_NAV_MAX_SIDE || p.ny < 2 || p.ny > TBNAV_NAV_MAX_SIDE || !std::isfinite(p.xmin) || !std::isfinite(p.ymin) ||
      !std::isfinite(p.resolution) || !(p.resolution > 0.0))
    return TBNAV_ERR_INVALID_ARG;
  int dev = 0;
  if (const int rc = tbnav::pick_device(p.device, &dev)) return rc;
  DeviceGuard guard(dev);
  if (!guard.ok) return TBNAV_ERR_NO_DEVICE;
  tbnav_nav* h = new (std::nothrow) tbnav_nav();
  if (!h) return TBNAV_ERR_INVALID_ARG;
  h->p = p;
  h->device = dev;
  h->n = p.nx * p.ny;
  h->inv = 1.0 / p.resolution;
  h->tiles_x = (p.nx + kTile - 1) / kTile;
  h->tiles_y = (p.ny + kTile - 1) / kTile;
  h->info.tiles[0] = h->tiles_x; h->info.tiles[1] = h->tiles_y;
  hipError_t e = hipMalloc((void**)&h->d_cost, (size_t)h->n);
  if (e == hipSuccess) e = hipMalloc((void**)&h->d_cost_solved, (size_t)h->n);
  if (e == hipSuccess) e = hipMalloc((void**)&h->d_infl, (size_t)kInflEntries);
  if (e == hipSuccess) e = hipMalloc((void**)&h->d_d, sizeof(unsigned) * (size_t)h->n);
  if (e == hipSuccess) e = hipMalloc((void**)&h->d_field, sizeof(float) * (size_t)h->n);
  if (e == hipSuccess) e = hipMalloc((void**)&h->d_flags, sizeof(unsigned) * 2 * (size_t)h->tiles_x * h->tiles_y);
  if (e == hipSuccess) e = hipMalloc((void**)&h->d_rec, sizeof(unsigned) * 2 * kMaxBatch);
  if (e != hipSuccess) { tbnav_nav_destroy(h); TBNAV_HIP(e); }
  *out = h;
  return TBNAV_OK;
}

void tbnav_nav_destroy(tbnav_nav* h) {
  if (!h) return;
  {
    DeviceGuard guard(h->device);
    (void)hipDeviceSynchronize();
    (void)hipFree(h->d_cost); (void)hipFree(h->d_cost_solved); (void)hipFree(h->d_infl); (void)hipFree(h->d_d); (void)hipFree(h->d_field); (void)hipFree(h->d_flags); (void)hipFree(h->d_rec);
    // nav_frontier.hip's (null where its calls were never made)
    (void)hipFree(h->d_front); (void)hipFree(h->d_seed); (void)hipFree(h->d_visited); (void)hipFree(h->d_label); (void)hipFree(h->d_size);
    (void)hipFree(h->d_fflags); (void)hipFree(h->d_frec); (void)hipFree(h->d_fcount); (void)hipFree(h->d_goals);
  }
  delete h;
}

int tbnav_nav_set_cost(tbnav_nav* h, const uint8_t* cost_host) {
  if (!h || !cost_host) return TBNAV_ERR_INVALID_ARG;
  for (int i = 0; i < h->n; ++i) if (cost_host[i] > TBNAV_NAV_MAX_COST) return TBNAV_ERR_INVALID_ARG;
  DeviceGuard guard(h->device);
  if (!guard.ok) return TBNAV_ERR_NO_DEVICE;
  TBNAV_HIP(hipMemcpy(h->d_cost, cost_host, (size_t)h->n, hipMemcpyHostToDevice));   // (solves are synchronous: nothing reads d_cost now)
  h->cost.assign(cost_host, cost_host + h->n);
  h->cost_set = true; h->cost_host_valid = true;
  ++h->cost_epoch;
  return TBNAV_OK;
}

int tbnav_nav_get_cost(tbnav_nav* h, uint8_t* cost_host) {
  if (!h || !cost_host || !h->cost_set) return TBNAV_ERR_INVALID_ARG;
  if (!h->cost_host_valid) {
    DeviceGuard guard(h->device);
    if (!guard.ok) return TBNAV_ERR_NO_DEVICE;
    h->cost.resize((size_t)h->n);
    TBNAV_HIP(hipMemcpy(h->cost.data(), h->d_cost, (size_t)h->n, hipMemcpyDeviceToHost));
    h->cost_host_valid = true;
  }
  std::memcpy(cost_host, h->cost.data(), (size_t)h->n);
  return TBNAV_OK;
}

int tbnav_nav_solve(tbnav_nav* h, int32_t goal_ix, int32_t goal_iy) {
  if (!h || !h->cost_set || !in_grid(h, goal_ix, goal_iy)) return TBNAV_ERR_INVALID_ARG;
  const int goal = goal_ix * h->p.ny + goal_iy;
  DeviceGuard guard(h->device);
  if (!guard.ok) return TBNAV_ERR_NO_DEVICE;
  uint8_t at_goal = 0;   // a grid set on the device has no host copy yet: the goal's cell alone is read back
  if (h->cost_host_valid) at_goal = h->cost[(size_t)goal];
  else TBNAV_HIP(hipMemcpy(&at_goal, h->d_cost + goal, 1, hipMemcpyDeviceToHost));
  if (at_goal == 0) return TBNAV_ERR_INVALID_ARG;
  h->solved = false; h->d_host_valid = false;   // from here on the last solution is being overwritten
  const int tiles = h->tiles_x * h->tiles_y;
  hipLaunchKernelGGL(nav_reset, dim3(256), dim3(256), 0, nullptr, h->d_d, h->n, h->p.ny, goal_ix, goal_iy, h->d_flags, tiles, h->tiles_y);
  TBNAV_HIP(hipGetLastError());
  return relax_from_start(h, goal_ix, goal_iy);
}

int tbnav_nav_cell_of(const tbnav_nav* h, double x, double y, int32_t* ix, int32_t* iy) {
  if (!h || !ix || !iy) return TBNAV_ERR_INVALID_ARG;
  const double gx = std::floor((x - h->p.xmin) * h->inv), gy = std::floor((y - h->p.ymin) * h->inv);
  if (!(gx >= 0.0 && gx < (double)h->p.nx && gy >= 0.0 && gy < (double)h->p.ny)) return TBNAV_ERR_OUT_OF_WORLD;   // (a NaN fails the comparisons)
  *ix = (int)gx; *iy = (int)gy;
  return TBNAV_OK;
}

int tbnav_nav_get_cost_to_go(tbnav_nav* h, uint32_t* d_host) {
  if (!h || !d_host || !h->solved) return TBNAV_ERR_INVALID_ARG;
  const int rc = download(h);
  if (rc != TBNAV_OK) return rc;
  std::memcpy(d_host, h->d_host.data(), sizeof(uint32_t) * (size_t)h->n);
  return TBNAV_OK;
}

int tbnav_nav_get_field(tbnav_nav* h, double cap, float* out) {
  if (!h || !out || !h->solved || !cap_ok(cap)) return TBNAV_ERR_INVALID_ARG;
  DeviceGuard guard(h->device);
  if (!guard.ok) return TBNAV_ERR_NO_DEVICE;
  const int rc = form_field(h, cap);
  if (rc != TBNAV_OK) return rc;
  TBNAV_HIP(hipMemcpy(out, h->d_field, sizeof(float) * (size_t)h->n, hipMemcpyDeviceToHost));
  return TBNAV_OK;
}

int tbnav_nav_path(tbnav_nav* h, int32_t start_ix, int32_t start_iy, int32_t* cells, int32_t cells_cap, int32_t* n) {
  if (!h || !n || cells_cap < 0 || (cells_cap > 0 && !cells) || !h->solved || !in_grid(h, start_ix, start_iy)) return TBNAV_ERR_INVALID_ARG;
  int rc = download(h);
  if (rc == TBNAV_OK) rc = download_cost_solved(h);
  if (rc != TBNAV_OK) return rc;
  const int ny = h->p.ny;
  const std::vector<unsigned>& d = h->d_host;
  const std::vector<uint8_t>& c = h->cost_solved;
  int ix = start_ix, iy = start_iy;
  if (c[(size_t)ix * ny + iy] == 0 || d[(size_t)ix * ny + iy] == kInf) return TBNAV_ERR_UNSUPPORTED;
  int len = 0;
  for (;;) {   // d falls strictly along the walk (G6), so it ends within n cells
    if (len < cells_cap) { cells[2 * len] = ix; cells[2 * len + 1] = iy; }
    ++len;
    if (d[(size_t)ix * ny + iy] == 0) break;
    unsigned best = kInf;
    int bm = -1;
    for (int m = 0; m < 8; ++m) {
      const int bx = ix + kDx[m], by = iy + kDy[m];
      if (!in_grid(h, bx, by) || c[(size_t)bx * ny + by] == 0 || d[(size_t)bx * ny + by] == kInf) continue;
      if (kDx[m] != 0 && kDy[m] != 0 && (c[(size_t)ix * ny + by] == 0 || c[(size_t)bx * ny + iy] == 0)) continue;
      const unsigned v = d[(size_t)bx * ny + by] + kW[m] * c[(size_t)bx * ny + by];
      if (v < best) { best = v; bm = m; }   // (strictly: ties stay with the first in G3's order)
    }
    if (bm < 0 || best != d[(size_t)ix * ny + iy] || len > h->n) return TBNAV_ERR_UNSUPPORTED;   // (not a fixed point of G4: cannot happen after a solve)
    ix += kDx[bm]; iy += kDy[bm];
  }
  *n = len;
  return len <= cells_cap ? TBNAV_OK : TBNAV_ERR_INVALID_ARG;
}

int tbnav_nav_last_solve(const tbnav_nav* h, tbnav_nav_solve_info* info, char* kernel, int32_t kernel_cap) {
  if (!h || (kernel && kernel_cap <= 0)) return TBNAV_ERR_INVALID_ARG;
  if (info) *info = h->info;
  if (kernel) std::snprintf(kernel, (size_t)kernel_cap, "%s", h->info.solved ? "nav_relax_tiles" : "");
  return TBNAV_OK;
}

int tbnav_nav_apply_to_mppi(tbnav_nav* h, tbnav_mppi* mppi, double cap, double weight) {
  if (!h || !mppi || !h->solved || !cap_ok(cap) || !std::isfinite(weight)) return TBNAV_ERR_INVALID_ARG;
  const tbnav_mppi_cost_field geom = geom_of(h, weight);
  {
    DeviceGuard guard(h->device);
    if (!guard.ok) return TBNAV_ERR_NO_DEVICE;
    const int rc = form_field(h, cap);
    if (rc != TBNAV_OK) return rc;
  }
  float* d_new = nullptr;
  const int rc = tbnav_mh::field_stage_device(mppi, geom, h->d_field, h->device, &d_new);
  return rc != TBNAV_OK ? rc : tbnav_mh::field_commit(mppi, &geom, d_new);
}

// every member or none: all copies are staged before the first member changes, as tbnav_mppi_group_set_cost_field does
int tbnav_nav_apply_to_mppi_group(tbnav_nav* h, tbnav_mppi_group* g, double cap, double weight) {
  if (!h || !g || !h->solved || !cap_ok(cap) || !std::isfinite(weight)) return TBNAV_ERR_INVALID_ARG;
  const tbnav_mppi_cost_field geom = geom_of(h, weight);
  {
    DeviceGuard guard(h->device);
    if (!guard.ok) return TBNAV_ERR_NO_DEVICE;
    const int rc = form_field(h, cap);
    if (rc != TBNAV_OK) return rc;
  }
  std::vector<float*> staged((size_t)g->n, nullptr);
  for (int r = 0; r < g->n; ++r) {
    const int rc = tbnav_mh::field_stage_device(g->m[r], geom, h->d_field, h->device, &staged[r]);
    if (rc != TBNAV_OK) {
      for (int q = 0; q < r; ++q) { DeviceGuard guard(g->m[q]->device); (void)hipFree(staged[q]); }
      return rc;
    }
  }
  int rc_all = TBNAV_OK;
  for (int r = 0; r < g->n; ++r) { const int rc = tbnav_mh::field_commit(g->m[r], &geom, staged[r]); if (rc != TBNAV_OK && rc_all == TBNAV_OK) rc_all = rc; }
  return rc_all;
}

}  // extern "C"

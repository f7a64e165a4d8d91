// nav.hip — the goal field of include/tbnav_nav.h (G1-G6): the exact integer cost-to-go to a goal cell over a cost grid, an OPTION the
// reference's controller does not have (its planner package, planner/src/planner/dstar_light.cpp:367-461, is never seen by MPPI).
// Here: the tiled label-correcting solver (nav_relax_tiles: one workgroup per ACTIVE 32 x 32 tile, relaxed in LDS to its own fixed
// point — nav_tiles.hpp's tile_fixed_point under the min-plus rule below; a round is a launch, the host stops at the first round that
// changed nothing), the field kernel G5 (nav_field), the host
// walk G6, and the hand-over to an MPPI handle, device to device, through mppi_field.hip's setters (field_stage_device / field_commit).
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "mppi_host.hpp"
#include "nav_host.hpp"

namespace tbnav_nk {

// G3's moves in the order of dstar_light.cpp:370-373 read as (dix, diy), and their w
constexpr int kDx[8] = {0, 0, -1, 1, -1, -1, 1, 1};
constexpr int kDy[8] = {-1, 1, 0, 0, -1, 1, -1, 1};
constexpr unsigned kW[8] = {10, 10, 10, 10, 14, 14, 14, 14};

struct RelaxArgs {
  const uint8_t* cost;   // [nx][ny]
  TileArgs t;            // v: the cost-to-go d
};

// tile_fixed_point's rule for G4: the costs staged beside d, and min-plus over G3's moves
struct RelaxRule {
  struct Cell { unsigned wgt[8]; };   // the price of an owned cell's eight moves (0: not allowed) — the costs are not read again
  const uint8_t* cost;
  uint8_t* s_c;                       // [kHalo * kHalo] a cell outside the grid is blocked, as G3 wants it
  __device__ __forceinline__ void stage(int i, bool in, int g) const { s_c[i] = in ? cost[g] : (uint8_t)0; }
  __device__ __forceinline__ void prepare(int c, Cell& o) const {
    const unsigned ca = s_c[c];
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      const unsigned cb = s_c[c + kDx[m] * kHalo + kDy[m]];
      bool ok = ca != 0 && cb != 0;
      if (kDx[m] != 0 && kDy[m] != 0) ok = ok && s_c[c + kDy[m]] != 0 && s_c[c + kDx[m] * kHalo] != 0;
      o.wgt[m] = ok ? kW[m] * cb : 0u;
    }
  }
  __device__ __forceinline__ bool idle(unsigned) const { return false; }
  __device__ __forceinline__ unsigned lower(const Cell& o, int c, unsigned best, const unsigned* s_d) const {
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      const unsigned db = s_d[c + kDx[m] * kHalo + kDy[m]];
      const unsigned cand = db + o.wgt[m];   // (G4: no sum of a reached d and a price overflows)
      best = (db != kInf && o.wgt[m] != 0u && cand < best) ? cand : best;
    }
    return best;
  }
};

__global__ __launch_bounds__(kThreads) void nav_relax_tiles(RelaxArgs a) {
  __shared__ unsigned s_d[kHalo * kHalo];
  __shared__ uint8_t s_c[kHalo * kHalo];
  __shared__ unsigned s_wake;
  tile_fixed_point(a.t, s_d, &s_wake, RelaxRule{a.cost, s_c});
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
    const RelaxArgs a{h->d_cost, {h->d_d, cur, nxt, rec, h->p.nx, h->p.ny, h->tiles_y}};
    hipLaunchKernelGGL(nav_relax_tiles, dim3(h->tiles_y, h->tiles_x), dim3(kThreads), 0, nullptr, a);
  }, &rounds, &launches, &visits);
  if (rc != TBNAV_OK) return rc;
  // what G6 walks over: the host copy where there is one, else kept on the device until a path is asked for
  if (h->cost_host_valid) h->cost_solved = h->cost;
  else TBNAV_HIP(hipMemcpy(h->d_cost_solved, h->d_cost, (size_t)h->n, hipMemcpyDeviceToDevice));
  h->cost_solved_valid = h->cost_host_valid;
  h->solved = true; h->ranked = false;   // (tbnav_nav_solve_frontiers_ranked sets it once this has returned)
  h->info.solved = 1; h->info.goal[0] = goal_ix; h->info.goal[1] = goal_iy;
  h->info.rounds = rounds; h->info.launches = launches; h->info.tile_visits = visits;
  return TBNAV_OK;
}

namespace {
bool cap_ok(double cap) { return std::isfinite(cap) && cap > 0.0; }
// G5 into d_field, finished when this returns (the nav handle's device is current)
int form_field(tbnav_nav* h, double cap) {
  hipLaunchKernelGGL(nav_field, dim3((h->n + 255) / 256), dim3(256), 0, nullptr, h->d_d, h->n, h->p.resolution, cap, h->d_field);
  TBNAV_HIP(hipGetLastError());
  TBNAV_HIP(hipDeviceSynchronize());
  return TBNAV_OK;
}
// the front of both hand-overs (`to`: the MPPI handle or the group): the checks, the field's geometry, and G5 in d_field
int field_for_mppi(tbnav_nav* h, const void* to, double cap, double weight, tbnav_mppi_cost_field* geom) {
  if (!h || !to || !h->solved || !cap_ok(cap) || !std::isfinite(weight)) return TBNAV_ERR_INVALID_ARG;
  *geom = tbnav_mppi_cost_field{h->p.nx, h->p.ny, h->p.xmin, h->p.ymin, h->p.resolution, weight};
  DeviceGuard guard(h->device);
  if (!guard.ok) return TBNAV_ERR_NO_DEVICE;
  return form_field(h, cap);
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
  hipError_t e = dev_alloc(h, h->d_cost, (size_t)h->n);
  if (e == hipSuccess) e = dev_alloc(h, h->d_cost_solved, (size_t)h->n);
  if (e == hipSuccess) e = dev_alloc(h, h->d_infl, (size_t)kInflEntries);
  if (e == hipSuccess) e = dev_alloc(h, h->d_d, (size_t)h->n);
  if (e == hipSuccess) e = dev_alloc(h, h->d_field, (size_t)h->n);
  if (e == hipSuccess) e = dev_alloc(h, h->d_flags, 2 * (size_t)h->tiles_x * h->tiles_y);
  if (e == hipSuccess) e = dev_alloc(h, h->d_rec, 2 * (size_t)kMaxBatch);
  if (e != hipSuccess) { tbnav_nav_destroy(h); TBNAV_HIP(e); }
  *out = h;
  return TBNAV_OK;
}

void tbnav_nav_destroy(tbnav_nav* h) {
  if (!h) return;
  {
    DeviceGuard guard(h->device);
    (void)hipDeviceSynchronize();
    for (void** b : h->buffers) (void)hipFree(*b);   // whatever dev_alloc has put into the handle, nav_frontier.hip's included
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
  const int rc = fetch_once(h, h->d_cost, h->cost, h->cost_host_valid);
  if (rc != TBNAV_OK) return rc;
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
  const int rc = fetch_once(h, h->d_d, h->d_host, h->d_host_valid);
  if (rc != TBNAV_OK) return rc;
  std::memcpy(d_host,h->d_host.data(), sizeof(uint32_t) * (size_t)h->n);
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
  int rc = fetch_once(h, h->d_d, h->d_host, h->d_host_valid);
  if (rc == TBNAV_OK) rc = fetch_once(h, h->d_cost_solved, h->cost_solved, h->cost_solved_valid);
  if (rc == TBNAV_OK && h->ranked) rc = fetch_once(h, h->d_start, h->start_host, h->start_host_valid);
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
    // G6: the goal, or the seed reached; G20: a seed that still holds its own start value (kInf off the seeds, which no walked cell holds)
    if (h->ranked ? d[(size_t)ix * ny + iy] == h->start_host[(size_t)ix * ny + iy] : d[(size_t)ix * ny + iy] == 0) break;
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
  tbnav_mppi_cost_field geom;
  int rc = field_for_mppi(h, mppi, cap, weight, &geom);
  if (rc != TBNAV_OK) return rc;
  float* d_new = nullptr;
  rc = tbnav_mh::field_stage_device(mppi, geom, h->d_field, h->device, &d_new);
  return rc != TBNAV_OK ? rc : tbnav_mh::field_commit(mppi, &geom, d_new);
}

// every member or none: all copies are staged before the first member changes, as tbnav_mppi_group_set_cost_field does
int tbnav_nav_apply_to_mppi_group(tbnav_nav* h, tbnav_mppi_group* g, double cap, double weight) {
  tbnav_mppi_cost_field geom;
  const int rc_f = field_for_mppi(h, g, cap, weight, &geom);
  if (rc_f != TBNAV_OK) return rc_f;
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

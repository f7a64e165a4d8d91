// nav_from_map.hip — the planner's cost grid taken straight from a filter particle's occupancy bits, on the device (tbnav_nav.h G7-G9).
// The host forms G7's inflation table (value by squared cell distance, fp64 without contraction: this file is compiled so); the kernel
// nav_cost_from_occ finds every cell's squared distance to the nearest occupied cell within the table's reach — integers only — and
// writes table[c] into the nav handle's cost grid (uint8_t) or into the values of an MPPI cost field (float).  Nothing of the filter's
// stored distance field is touched or allocated: the bits in the tiles (TilePool::bm) are the source.
#include <cmath>
#include <cstring>
#include <vector>

#include "rbpf_host.hpp"
#include "mppi_host.hpp"
#include "nav_host.hpp"

namespace tbnav_nk {

constexpr int kFmTile = 32;                     // cells per side of a workgroup's output tile: one tile of the filter's pool
constexpr int kFmThreads = 256;                 // four waves; a wave's 64 lanes are two rows of 32 consecutive iy
constexpr int kFmRows = 3 * kFmTile;            // staged rows: the tile's and one tile of halo either side (TBNAV_NAV_MAX_REACH)
constexpr int kFmWords = 3;                     // u32 per staged row: the tile's columns and one tile either side
constexpr int kFmOwn = kFmTile * kFmTile / kFmThreads;
constexpr int kFmRowStep = kFmThreads / kFmTile;
static_assert(TBNAV_NAV_MAX_REACH <= kFmTile, "the search never leaves the 3 x 3 tiles staged");
static_assert(kFmTile == tbnav_rk::kTS, "an output tile is a tile of the filter's pool");

struct FromMapArgs {
  const unsigned int* bm;      // TilePool::bm
  const unsigned int* table;   // [N][TT] the particles' tile tables
  const int* best;             // where the particle's index is on the device (rbpf_argmax), or null: `particle`
  int particle;
  int TW, TT;                  // tiles per side, per map
  int side;                    // cells per side of the map (and of the output grid)
  int reach;                   // R
  int n_tab;                   // R*R + 1 table entries; tab[n_tab] is the open value
};

// One workgroup per 32 x 32 output tile.  Rows are ix (the slow index), bits within a row iy — the tiles' own layout and the output's.
template <class OUT>
__global__ __launch_bounds__(kFmThreads) void nav_cost_from_occ(FromMapArgs a, const OUT* __restrict__ tab, OUT* __restrict__ out) {
  __shared__ unsigned int s_occ[kFmRows * kFmWords];
  __shared__ OUT s_tab[kInflEntries];
  const int tid = threadIdx.x, tile_x = blockIdx.y, tile_y = blockIdx.x;
  const int p = a.best ? *a.best : a.particle;
  const unsigned int* __restrict__ tab_p = a.table + (size_t)p * a.TT;
  // the occupancy rows of the 3 x 3 tiles round this one: id 0 (nobody has written the tile) and tiles outside the map read as
  // empty, and a ragged last tile is cut at the map's side
  int any = 0;
  for (int i = tid; i < kFmRows * kFmWords; i += kFmThreads) {
    const int lr = i / kFmWords, wc = i - lr * kFmWords;
    const int gx = (tile_x - 1) * kFmTile + lr, ty = tile_y - 1 + wc;
    unsigned int w = 0u;
    if (gx >= 0 && gx < a.side && ty >= 0 && ty < a.TW) {
      const unsigned int id = tab_p[(gx >> 5) * a.TW + ty];
      if (id != 0u) w = a.bm[(size_t)id * kFmTile + (gx & (kFmTile - 1))];
      const int inside = a.side - ty * kFmTile;   // columns of this tile that are cells of the map (>= 1)
      if (inside < kFmTile) w &= (1u << inside) - 1u;
    }
    s_occ[i] = w;
    any |= w != 0u;
  }
  for (int i = tid; i <= a.n_tab; i += kFmThreads) s_tab[i] = tab[i];
  any = __syncthreads_or(any);   // (also: the staging is complete)

  const int ly = tid & (kFmTile - 1), iy = tile_y * kFmTile + ly;
  const int lx0 = tid >> 5, ix0 = tile_x * kFmTile + lx0;
  if (iy >= a.side) return;
  const OUT open = s_tab[a.n_tab];
  if (!any) {   // nothing occupied within reach of any cell of this tile: in a room, most tiles
#pragma unroll
    for (int j = 0; j < kFmOwn; ++j) {
      const int ix = ix0 + j * kFmRowStep;
      if (ix < a.side) out[(size_t)ix * a.side + iy] = open;
    }
    return;
  }
  const unsigned long long low33 = (1ull << 33) - 1ull;
  const int R = a.reach, c_max = a.n_tab - 1;
  for (int j = 0; j < kFmOwn; ++j) {
    const int lx = lx0 + j * kFmRowStep, ix = ix0 + j * kFmRowStep;
    if (ix >= a.side) break;
    int best = 1 << 20;
    // rows at distance dr = 0, 1, .. R either side; in each the nearest set bit left and right of this column, out to 32 columns
    for (int dr = 0; dr <= R && dr * dr < best; ++dr) {
      for (int s = 0; s < (dr == 0 ? 1 : 2); ++s) {
        const unsigned int* row = s_occ + (kFmTile + lx + (s ? dr : -dr)) * kFmWords;   // rows 0 .. 95: dr <= 32
        const unsigned int w0 = row[0], w1 = row[1], w2 = row[2];
        // the cell is bit 32 + ly of the row's 96.  left: bit k <-> column offset k - 32; right: bit k <-> column offset k
        const unsigned long long left = ((((unsigned long long)w1 << 32) | w0) >> ly) & low33;
        const unsigned long long right = ((((unsigned long long)w2 << 32) | w1) >> ly) & low33;
        if (left) {
          const int dc = 32 - (63 - __clzll((long long)left));
          const int c = dr * dr + dc * dc;
          best = c < best ? c : best;
        }
        if (right) {
          const int dc = __ffsll((long long)right) - 1;
          const int c = dr * dr + dc * dc;
          best = c < best ? c : best;
        }
      }
    }
    out[(size_t)ix * a.side + iy] = best <= c_max ? s_tab[best] : open;
  }
}

}  // namespace tbnav_nk

using namespace tbnav_nk;

namespace {

// G7's arguments: TBNAV_OK with *reach = R, or what the header says
int infl_check(double resolution, double r_robot, double r_inflate, double k, int* reach) {
  if (!std::isfinite(resolution) || !std::isfinite(r_robot) || !std::isfinite(r_inflate) || !std::isfinite(k) || !(resolution > 0.0) ||
      !(0.0 <= r_robot && r_robot < r_inflate && r_inflate <= 10.0) || !(0.0 <= k && k <= 63.0))
    return TBNAV_ERR_INVALID_ARG;
  const double q = std::ceil(r_inflate / resolution) + 1.0;
  if (!(q <= (double)TBNAV_NAV_MAX_REACH)) return TBNAV_ERR_UNSUPPORTED;
  *reach = (int)q;
  return TBNAV_OK;
}
// the distances the tables are taken at: entry c = 0 .. R*R, then the open value's (the filter's max_occ_dist)
double infl_dist(int c, int n_tab, double resolution) { return c < n_tab ? std::sqrt((double)c) * resolution : 10.0; }
// planner::navCostFromDistance's arithmetic
uint8_t infl_cost(double d, double r_robot, double r_inflate, double k) {
  double t = (r_inflate - d) / (r_inflate - r_robot);
  t = t > 0.0 ? t : 0.0;
  t = t < 1.0 ? t : 1.0;
  return (uint8_t)(d <= r_robot ? 0.0 : 1.0 + std::rint(k * t * t));
}
// controller::costFieldFromDistance's
float infl_field(double d, double r_robot, double r_inflate) {
  const double t = (r_inflate - d) / (r_inflate - r_robot);
  return (float)(d <= r_robot ? 1.0 : (d >= r_inflate ? 0.0 : t * t));
}

FromMapArgs from_map_args(const tbnav_rbpf* pf, int32_t particle, int reach) {
  return FromMapArgs{pf->pool.bm, pf->d_table[pf->cur], particle == TBNAV_NAV_BEST_PARTICLE ? pf->d_best : nullptr, particle,
                     pf->TW, pf->TT, pf->xsize, reach, reach * reach + 1};
}
// the arg-max of the weights where the best particle is asked for, then the kernel, on the filter's stream (its device is current);
// d_tab holds n_tab + 1 values when the kernel runs (the caller has enqueued their copy on the same stream)
template <class OUT>
int from_map_enqueue(tbnav_rbpf* pf, int32_t particle, int reach, const OUT* d_tab, OUT* d_out) {
  if (particle == TBNAV_NAV_BEST_PARTICLE) {
    const StatePtrs sp = state_ptrs(pf->d_state[pf->cur], pf->N);
    hipLaunchKernelGGL(rbpf_argmax, dim3(1), dim3(256), 0, pf->stream, pf->N, sp.weight, sp.pose, pf->d_best, pf->d_best_pose);
    TBNAV_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL((nav_cost_from_occ<OUT>), dim3(pf->TW, pf->TW), dim3(kFmThreads), 0, pf->stream, from_map_args(pf, particle, reach),
                     d_tab, d_out);
  TBNAV_HIP(hipGetLastError());
  return TBNAV_OK;
}
bool particle_ok(const tbnav_rbpf* pf, int32_t particle) {
  return particle == TBNAV_NAV_BEST_PARTICLE || (particle >= 0 && particle < pf->N);
}

}  // namespace

extern "C" {

int tbnav_nav_inflation_tables(double resolution, double r_robot, double r_inflate, double k, uint8_t* cost, float* field, int32_t cap,
                               int32_t* n, int32_t* reach) {
  int R = 0;
  const int rc = infl_check(resolution, r_robot, r_inflate, k, &R);
  if (rc != TBNAV_OK) return rc;
  const int n_tab = R * R + 1;
  if (n) *n = n_tab;
  if (reach) *reach = R;
  if ((cost || field) && cap < n_tab + 1) return TBNAV_ERR_INVALID_ARG;
  for (int c = 0; c <= n_tab; ++c) {
    const double d = infl_dist(c, n_tab, resolution);
    if (cost) cost[c] = infl_cost(d, r_robot, r_inflate, k);
    if (field) field[c] = infl_field(d, r_robot, r_inflate);
  }
  return TBNAV_OK;
}

int tbnav_nav_set_cost_from_rbpf(tbnav_nav* h, tbnav_rbpf* pf, int32_t particle, double r_robot, double r_inflate, double k) {
  return tbnav_nav_profile_cost_from_rbpf(h, pf, particle, r_robot, r_inflate, k, 1, nullptr);
}

int tbnav_nav_profile_cost_from_rbpf(tbnav_nav* h, tbnav_rbpf* pf, int32_t particle, double r_robot, double r_inflate, double k, int32_t launches,
                                     float* kernel_ms) {
  if (!h || !pf || !particle_ok(pf, particle) || launches < 1) return TBNAV_ERR_INVALID_ARG;
  if (h->p.nx != pf->xsize || h->p.ny != pf->xsize || pf->ysize != pf->xsize || h->p.xmin != pf->p.xmin || h->p.ymin != pf->p.ymin ||
      h->p.resolution != pf->p.resolution)
    return TBNAV_ERR_INVALID_ARG;
  int R = 0;
  const int rc = infl_check(pf->p.resolution, r_robot, r_inflate, k, &R);
  if (rc != TBNAV_OK) return rc;
  if (h->device != pf->device) return TBNAV_ERR_UNSUPPORTED;
  const int n_tab = R * R + 1;
  tbnav::DeviceGuard guard(pf->device);
  if (!guard.ok) return TBNAV_ERR_NO_DEVICE;
  h->infl.resize((size_t)n_tab + 1);
  for (int c = 0; c <= n_tab; ++c) h->infl[(size_t)c] = infl_cost(infl_dist(c, n_tab, pf->p.resolution), r_robot, r_inflate, k);
  // G9: behind whatever the filter has in flight.  Solves are synchronous, so nothing reads d_cost now; every value the table holds
  // is at most 1 + 63 = TBNAV_NAV_MAX_COST (G2).
  TBNAV_HIP(hipMemcpyAsync(h->d_infl, h->infl.data(), (size_t)n_tab + 1, hipMemcpyHostToDevice, pf->stream));
  hipEvent_t ev[2] = {nullptr, nullptr};
  if (kernel_ms) { TBNAV_HIP(hipEventCreate(&ev[0])); TBNAV_HIP(hipEventCreate(&ev[1])); TBNAV_HIP(hipEventRecord(ev[0], pf->stream)); }
  int rc_k = TBNAV_OK;
  for (int l = 0; l < launches && rc_k == TBNAV_OK; ++l) rc_k = from_map_enqueue<uint8_t>(pf, particle, R, h->d_infl, h->d_cost);
  hipError_t e = hipSuccess;
  if (kernel_ms && rc_k == TBNAV_OK) e = hipEventRecord(ev[1], pf->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(pf->stream);
  if (kernel_ms) {
    float ms = 0.0f;
    if (e == hipSuccess && rc_k == TBNAV_OK) e = hipEventElapsedTime(&ms, ev[0], ev[1]);
    *kernel_ms = ms / (float)launches;
    (void)hipEventDestroy(ev[0]); (void)hipEventDestroy(ev[1]);
  }
  if (rc_k != TBNAV_OK) return rc_k;
  TBNAV_HIP(e);
  h->cost_set = true; h->cost_host_valid = false;   // (the host copy is fetched when somebody asks: tbnav_nav_get_cost)
  h->from_map = true;
  ++h->cost_epoch;
  return TBNAV_OK;
}

int tbnav_mppi_set_cost_field_from_rbpf(tbnav_mppi* mppi, tbnav_rbpf* pf, int32_t particle, double r_robot, double r_inflate, double weight) {
  if (!mppi || !pf || !particle_ok(pf, particle) || !std::isfinite(weight) || pf->ysize != pf->xsize || pf->xsize > TBNAV_MPPI_FIELD_MAX_SIDE)
    return TBNAV_ERR_INVALID_ARG;
  int R = 0;
  const int rc = infl_check(pf->p.resolution, r_robot, r_inflate, 0.0, &R);
  if (rc != TBNAV_OK) return rc;
  if (mppi->device != pf->device) return TBNAV_ERR_UNSUPPORTED;
  const int n_tab = R * R + 1;
  const tbnav_mppi_cost_field geom{pf->xsize, pf->xsize, pf->p.xmin, pf->p.ymin, pf->p.resolution, weight};
  std::vector<float> tab((size_t)n_tab + 1);
  for (int c = 0; c <= n_tab; ++c) tab[(size_t)c] = infl_field(infl_dist(c, n_tab, pf->p.resolution), r_robot, r_inflate);
  float* d_tmp = nullptr;   // the values, then the table
  {
    tbnav::DeviceGuard guard(pf->device);
    if (!guard.ok) return TBNAV_ERR_NO_DEVICE;
    TBNAV_HIP(hipMalloc((void**)&d_tmp, sizeof(float) * (pf->G + tab.size())));
    hipError_t e = hipMemcpyAsync(d_tmp + pf->G, tab.data(), sizeof(float) * tab.size(), hipMemcpyHostToDevice, pf->stream);
    int rc_k = TBNAV_OK;
    if (e == hipSuccess) rc_k = from_map_enqueue<float>(pf, particle, R, d_tmp + pf->G, d_tmp);
    if (e == hipSuccess && rc_k == TBNAV_OK) e = hipStreamSynchronize(pf->stream);
    if (e != hipSuccess || rc_k != TBNAV_OK) { (void)hipFree(d_tmp); TBNAV_HIP(e); return rc_k; }
  }
  // every value is 0 .. 1: tbnav_mppi.h F1's finiteness holds by construction
  float* d_new = nullptr;
  const int rc_s = tbnav_mh::field_stage_device(mppi, geom, d_tmp, pf->device, &d_new);
  { tbnav::DeviceGuard guard(pf->device); (void)hipFree(d_tmp); }
  return rc_s != TBNAV_OK ? rc_s : tbnav_mh::field_commit(mppi, &geom, d_new);
}

int tbnav_nav_last_cost_kernel(const tbnav_nav* h, char* kernel, int32_t kernel_cap) {
  if (!h || !kernel || kernel_cap <= 0) return TBNAV_ERR_INVALID_ARG;
  std::snprintf(kernel, (size_t)kernel_cap, "%s", h->from_map ? "nav_cost_from_occ<uint8_t>" : "");
  return TBNAV_OK;
}

}  // extern "C"

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

constexpr int kOccRows = 3 * kTile;             // staged rows: the output tile's (a tile of the filter's pool) and one tile of halo either side (TBNAV_NAV_MAX_REACH)
constexpr int kOccWords = 3;                    // u32 per staged row: the tile's columns and one tile either side
static_assert(TBNAV_NAV_MAX_REACH <= kTile, "the search never leaves the 3 x 3 tiles staged");

struct FromMapArgs {
  const unsigned int* bm;      // TilePool::bm
  ParticleRef p;               // side: cells per side of the map (and of the output grid)
  int reach;                   // R
  int n_tab;                   // R*R + 1 table entries; tab[n_tab] is the open value
};

// One workgroup per 32 x 32 output tile.  Rows are ix (the slow index), bits within a row iy — the tiles' own layout and the output's.
template <class OUT>
__global__ __launch_bounds__(kThreads) void nav_cost_from_occ(FromMapArgs a, const OUT* __restrict__ tab, OUT* __restrict__ out) {
  __shared__ unsigned int s_occ[kOccRows * kOccWords];
  __shared__ OUT s_tab[kInflEntries];
  const int tid = threadIdx.x, tile_x = blockIdx.y, tile_y = blockIdx.x;
  const unsigned int* __restrict__ tab_p = particle_row(a.p);
  // the occupancy rows of the 3 x 3 tiles round this one: id 0 (nobody has written the tile) and tiles outside the map read as
  // empty, and a ragged last tile is cut at the map's side
  int any = 0;
  for (int i = tid; i < kOccRows * kOccWords; i += kThreads) {
    const int lr = i / kOccWords, wc = i - lr * kOccWords;
    const int gx = (tile_x - 1) * kTile + lr, ty = tile_y - 1 + wc;
    unsigned int w = 0u;
    if (gx >= 0 && gx < a.p.side && ty >= 0 && ty < a.p.TW) {
      const unsigned int id = tab_p[(gx >> 5) * a.p.TW + ty];
      if (id != 0u) w = a.bm[(size_t)id * kTile + (gx & (kTile - 1))];
      const int inside = a.p.side - ty * kTile;   // columns of this tile that are cells of the map (>= 1)
      if (inside < kTile) w &= (1u << inside) - 1u;
    }
    s_occ[i] = w;
    any |= w != 0u;
  }
  for (int i = tid; i <= a.n_tab; i += kThreads) s_tab[i] = tab[i];
  any = __syncthreads_or(any);   // (also: the staging is complete)

  const int ly = tid & (kTile - 1), iy = tile_y * kTile + ly;
  const int lx0 = tid >> 5, ix0 = tile_x * kTile + lx0;
  if (iy >= a.p.side) return;
  const OUT open = s_tab[a.n_tab];
  if (!any) {   // nothing occupied within reach of any cell of this tile: in a room, most tiles
#pragma unroll
    for (int j = 0; j < kOwn; ++j) {
      const int ix = ix0 + j * kRowStep;
      if (ix < a.p.side) out[(size_t)ix * a.p.side + iy] = open;
    }
    return;
  }
  const unsigned long long low33 = (1ull << 33) - 1ull;
  const int R = a.reach, c_max = a.n_tab - 1;
  for (int j = 0; j < kOwn; ++j) {
    const int lx = lx0 + j * kRowStep, ix = ix0 + j * kRowStep;
    if (ix >= a.p.side) break;
    int best = 1 << 20;
    // rows at distance dr = 0, 1, .. R either side; in each the nearest set bit left and right of this column, out to 32 columns
    for (int dr = 0; dr <= R && dr * dr < best; ++dr) {
      for (int s = 0; s < (dr == 0 ? 1 : 2); ++s) {
        const unsigned int* row = s_occ + (kTile + lx + (s ? dr : -dr)) * kOccWords;   // rows 0 .. 95: dr <= 32
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
    out[(size_t)ix * a.p.side + iy] = best <= c_max ? s_tab[best] : open;
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

// the arg-max of the weights where the best particle is asked for, then the kernel, on the filter's stream (its device is current);
// d_tab holds n_tab + 1 values when the kernel runs (the caller has enqueued their copy on the same stream)
template <class OUT>
int from_map_enqueue(tbnav_rbpf* pf, int32_t particle, int reach, const OUT* d_tab, OUT* d_out) {
  const int rc = enqueue_best(pf, particle);
  if (rc != TBNAV_OK) return rc;
  const FromMapArgs a{pf->pool.bm, particle_ref(pf, particle), reach, reach * reach + 1};
  hipLaunchKernelGGL((nav_cost_from_occ<OUT>), dim3(pf->TW, pf->TW), dim3(kThreads), 0, pf->stream, a, d_tab, d_out);
  TBNAV_HIP(hipGetLastError());
  return TBNAV_OK;
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
  const int rc_grid = same_grid(h, pf);   // another grid is refused before G7's arguments are looked at, another device after
  if (rc_grid == TBNAV_ERR_INVALID_ARG) return rc_grid;
  int R = 0;
  const int rc = infl_check(pf->p.resolution, r_robot, r_inflate, k, &R);
  if (rc != TBNAV_OK) return rc;
  if (rc_grid != TBNAV_OK) return rc_grid;
  const int n_tab = R * R + 1;
  tbnav::DeviceGuard guard(pf->device);
  if (!guard.ok) return TBNAV_ERR_NO_DEVICE;
  h->infl.resize((size_t)n_tab + 1);
  for (int c = 0; c <= n_tab; ++c) h->infl[(size_t)c] = infl_cost(infl_dist(c, n_tab, pf->p.resolution), r_robot, r_inflate, k);
  // G9: behind whatever the filter has in flight.  Solves are synchronous, so nothing reads d_cost now; every value the table holds
  // is at most 1 + 63 = TBNAV_NAV_MAX_COST (G2).
  TBNAV_HIP(hipMemcpyAsync(h->d_infl, h->infl.data(), (size_t)n_tab + 1, hipMemcpyHostToDevice, pf->stream));
  StageTimer timer(kernel_ms != nullptr, 2, pf->stream);
  TBNAV_HIP(timer.create());
  TBNAV_HIP(timer.stamp(0));
  int rc_k = TBNAV_OK;
  for (int l = 0; l < launches && rc_k == TBNAV_OK; ++l) rc_k = from_map_enqueue<uint8_t>(pf, particle, R, h->d_infl, h->d_cost);
  hipError_t e = rc_k == TBNAV_OK ? timer.stamp(1) : hipSuccess;
  if (e == hipSuccess) e = hipStreamSynchronize(pf->stream);
  if (kernel_ms) {
    float ms = 0.0f;
    if (e == hipSuccess && rc_k == TBNAV_OK) e = timer.elapsed(0, &ms);
    *kernel_ms = ms / (float)launches;
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

// nav_gain.hip — the frontiers ranked by what a scan from them would reveal (tbnav_nav.h G17-G20).  On the device: the UNKNOWN and
// OCCUPIED bits of a particle's map as dense row words (nav_gain_classes), the seed cells of the last find as a list (nav_gain_list), the
// gain of every one of them — integer rays over the (2R+1)^2 window in LDS, a count of distinct unknown cells (nav_frontier_gain<RMAX>) —
// and the start of a ranked solve (nav_reset_ranked).  On the host: the ring of end points (G17), the cluster list, and the calls' checks.
// Integers and comparisons only; compiled without contraction like the rest of the planner.
#include <cstring>
#include <vector>

#include "rbpf_host.hpp"
#include "nav_host.hpp"

namespace tbnav_nk {

constexpr int kGainMaxRays = 1024;   // |E(128)| = 788 is the most
constexpr int kGainSmall = 32;       // the range up to which the small window's instantiation runs

struct GainClassArgs {
  const double* lo;            // TilePool::lo
  const unsigned int* bm;      // TilePool::bm
  ParticleRef p;
  double half_lo, half_hi;     // ExportCuts: UNKNOWN is half_lo <= l <= half_hi (G10)
  unsigned int* unk;           // [side][TW] out
  unsigned int* occ;           // [side][TW] out
};

// One workgroup per tile.  Rows are ix (the slow index), bits within a row iy — the tiles' own layout.
__global__ __launch_bounds__(kThreads) void nav_gain_classes(GainClassArgs a) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int tile_x = blockIdx.y, tile_y = blockIdx.x, tile = tile_x * a.p.TW + tile_y;
  const unsigned int id = particle_row(a.p)[tile];
  const int inside = a.p.side - tile_y * kTile;   // columns of this tile that are cells of the map (>= 1)
  const unsigned int cols = inside < kTile ? (1u << inside) - 1u : 0xFFFFFFFFu;
  if (id == 0u) {   // nobody has written this tile: unknown throughout, nothing occupied
    const int gx = tile_x * kTile + tid;
    if (tid < kTile && gx < a.p.side) { a.unk[(size_t)gx * a.p.TW + tile_y] = cols; a.occ[(size_t)gx * a.p.TW + tile_y] = ~cols; }
    return;
  }
  const double* __restrict__ t_lo = a.lo + (size_t)id * (kTile * kTile);
  const int lx0 = tid >> 5, ly = tid & (kTile - 1);
#pragma unroll
  for (int j = 0; j < kOwn; ++j) {
    const int r = lx0 + j * kRowStep;
    const double l = t_lo[r * kTile + ly];
    const unsigned long long bu = __ballot(l >= a.half_lo && l <= a.half_hi);
    if (lane == 0) {   // (lane 0's row is the even one of the wave's two)
      const int gx = tile_x * kTile + r;
      if (gx < a.p.side) a.unk[(size_t)gx * a.p.TW + tile_y] = (unsigned int)bu & cols;
      if (gx + 1 < a.p.side) a.unk[(size_t)(gx + 1) * a.p.TW + tile_y] = (unsigned int)(bu >> 32) & cols;
    }
  }
  const int gx = tile_x * kTile + tid;
  if (tid < kTile && gx < a.p.side) a.occ[(size_t)gx * a.p.TW + tile_y] = (a.bm[(size_t)id * kTile + tid] & cols) | ~cols;
}

// The set bits of seed[nx][tiles_y] as cell indices, a word per thread; *slot (zero before) is where the next word's cells go
__global__ void nav_gain_list(const unsigned* __restrict__ seed, int words, int tiles_y, int ny, unsigned* __restrict__ list, int cap, unsigned* __restrict__ slot) {
  const int stride = gridDim.x * blockDim.x;
  for (int w = blockIdx.x * blockDim.x + threadIdx.x; w < words; w += stride) {
    unsigned b = seed[w];
    if (b == 0u) continue;
    unsigned at = atomicAdd(slot, (unsigned)__popc(b));
    const int ix = w / tiles_y;
    const unsigned base = (unsigned)(ix * ny + (w - ix * tiles_y) * kTile);
    for (int k = 0; k < kTile && b != 0u; ++k) {
      if (at < (unsigned)cap) list[at] = base + (unsigned)(__ffs(b) - 1);   // (the find counted these bits: cap is their number)
      ++at;
      b &= b - 1u;
    }
  }
}

struct GainArgs {
  const unsigned* unk;         // [side][TW]
  const unsigned* occ;         // [side][TW]
  const unsigned* list;        // [viewpoints] cell indices
  const short* rays;           // [n_rays][2] E(R)
  int n_rays, R, side, TW;
  unsigned* gain;              // [side][side] out, at the viewpoints
  unsigned long long* stat;    // [0] max= gain << 32 | ~cell, [1] max= ~gain
};

// One workgroup per viewpoint.  LDS bitmaps of the window: row r is ix = vx - R + r, bit c of the row iy = vy - R + c.
template <int RMAX>
__global__ __launch_bounds__(kThreads) void nav_frontier_gain(GainArgs a) {
  constexpr int W = (2 * RMAX + 1 + 31) / 32, ROWS = 2 * RMAX + 1;
  __shared__ unsigned s_unk[ROWS * W], s_occ[ROWS * W], s_seen[ROWS * W];
  __shared__ unsigned s_total;
  const int tid = threadIdx.x;
  const unsigned cell = a.list[blockIdx.x];
  const int R = a.R < RMAX ? a.R : RMAX;
  if (cell >= (unsigned)(a.side * a.side)) return;   // (the whole workgroup alike; cannot happen after nav_gain_list)
  const int vx = (int)cell / a.side, vy = (int)cell - vx * a.side;
  const int rows = 2 * R + 1, words = (rows + 31) >> 5, x0 = vx - R, y0 = vy - R;
  for (int i = tid; i < rows * words; i += kThreads) {
    const int r = i / words, w = i - r * words, gx = x0 + r, c0 = y0 + w * 32;
    unsigned u = 0u, o = 0xFFFFFFFFu;   // outside the grid: nothing unknown, and a ray ends as at an occupied cell
    if (gx >= 0 && gx < a.side) {
      const int g0 = c0 >> 5, sh = c0 & 31;   // (an arithmetic shift: c0 may be negative)
      const bool in0 = g0 >= 0 && g0 < a.TW, in1 = g0 + 1 >= 0 && g0 + 1 < a.TW;
      const unsigned u0 = in0 ? a.unk[(size_t)gx * a.TW + g0] : 0u, u1 = in1 ? a.unk[(size_t)gx * a.TW + g0 + 1] : 0u;
      const unsigned o0 = in0 ? a.occ[(size_t)gx * a.TW + g0] : 0xFFFFFFFFu, o1 = in1 ? a.occ[(size_t)gx * a.TW + g0 + 1] : 0xFFFFFFFFu;
      u = sh ? (u0 >> sh) | (u1 << (32 - sh)) : u0;
      o = sh ? (o0 >> sh) | (o1 << (32 - sh)) : o0;
    }
    s_unk[r * W + w] = u; s_occ[r * W + w] = o; s_seen[r * W + w] = 0u;
  }
  if (tid == 0) s_total = 0u;
  __syncthreads();

  for (int k = tid; k < a.n_rays; k += kThreads) {
    const int ex = a.rays[2 * k], ey = a.rays[2 * k + 1];
    const int ax = ex < 0 ? -ex : ex, ay = ey < 0 ? -ey : ey, sx = ex < 0 ? -1 : 1, sy = ey < 0 ? -1 : 1;
    const int n = ax > ay ? ax : ay;
    if (n > R) continue;   // (E(R) holds no such end point)
    // G17's quotients with the remainder carried: 2*s*|e| + n = q * 2n + rem, 0 <= rem < 2n — the same integers as the closed form
    int qx = 0, remx = n, qy = 0, remy = n;
    int px = R, py = R;
    for (int s = 1; s <= n; ++s) {
      remx += 2 * ax; if (remx >= 2 * n) { remx -= 2 * n; ++qx; }
      remy += 2 * ay; if (remy >= 2 * n) { remy -= 2 * n; ++qy; }
      const int cx = R + sx * qx, cy = R + sy * qy;
      const unsigned m = 1u << (cy & 31), pm = 1u << (py & 31);
      if (s_occ[cx * W + (cy >> 5)] & m) break;
      if (cx != px && cy != py && (s_occ[px * W + (cy >> 5)] & m) && (s_occ[cx * W + (py >> 5)] & pm)) break;   // G18: a diagonal wall does not leak
      if ((s_unk[cx * W + (cy >> 5)] & m) && !(s_seen[cx * W + (cy >> 5)] & m)) atomicOr(&s_seen[cx * W + (cy >> 5)], m);
      px = cx; py = cy;
    }
  }
  __syncthreads();
  unsigned mine = 0u;
  for (int i = tid; i < rows * words; i += kThreads) mine += (unsigned)__popc(s_seen[(i / words) * W + (i - (i / words) * words)]);
  if (mine) atomicAdd(&s_total, mine);
  __syncthreads();
  if (tid == 0) {
    const unsigned total = s_total;
    a.gain[cell] = total;
    atomicMax(&a.stat[0], ((unsigned long long)total << 32) | (unsigned long long)(0xFFFFFFFFu - cell));   // the most, and among those the least cell
    atomicMax(&a.stat[1], (unsigned long long)(0xFFFFFFFFu - total));
  }
}

// G20's start: d = start = weight * (gain_max - gain) at the seeds and UNREACHED elsewhere; active in round 0 every tile that sees a seed
// (nav_reset_goals' rule).  The host has zeroed `flags` before.
__global__ void nav_reset_ranked(unsigned* __restrict__ d, unsigned* __restrict__ start, int nx, int ny, int tiles_y, const unsigned* __restrict__ seed,
                                 const unsigned* __restrict__ gain, const unsigned long long* __restrict__ stat, unsigned weight, unsigned* __restrict__ flags) {
  const int stride = gridDim.x * blockDim.x, total = nx * ny;
  const unsigned gain_max = (unsigned)(stat[0] >> 32);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int gx = i / ny, gy = i - gx * ny;
    const bool goal = (seed[gx * tiles_y + (gy >> 5)] >> (gy & 31)) & 1u;
    const unsigned v = goal ? weight * (gain_max - gain[i]) : kInf;   // (G20: at most 4096 * 66048)
    d[i] = v; start[i] = v;
    if (!goal) continue;
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

bool range_ok(int32_t r) { return r >= 1 && r <= TBNAV_NAV_MAX_GAIN_RANGE; }

// G17's ring in ascending (ex, ey)
void ring(int R, std::vector<short>& out) {
  out.clear();
  for (int ex = -R; ex <= R; ++ex)
    for (int ey = -R; ey <= R; ++ey) {
      const int q = ex * ex + ey * ey;
      if (q > R * R - R && q <= R * R + R) { out.push_back((short)ex); out.push_back((short)ey); }
    }
}


// the device side of G17-G20, at the first call that needs it (the handle's device is current)
int ensure_gain_buffers(tbnav_nav* h) {
  if (h->d_gstat) return TBNAV_OK;
  TBNAV_HIP(dev_alloc(h, h->d_gunk, mask_words(h)));
  TBNAV_HIP(dev_alloc(h, h->d_gocc, mask_words(h)));
  TBNAV_HIP(dev_alloc(h, h->d_grays, 2 * (size_t)kGainMaxRays));
  TBNAV_HIP(dev_alloc(h, h->d_gain, (size_t)h->n));
  TBNAV_HIP(dev_alloc(h, h->d_start, (size_t)h->n));
  TBNAV_HIP(dev_alloc(h, h->d_gstat, 3));   // (the last: what it holds says that all of them stand)
  return TBNAV_OK;
}

// G19: the find, then the gain of its seeds; ms[5] where times are asked for (the find's four stages, then the gain's kernels together)
int find_gain(tbnav_nav* h, tbnav_rbpf* pf, int32_t particle, int32_t min_cells, int32_t range, tbnav_nav_frontier_info* info, tbnav_nav_gain_info* ginfo,
              float* ms) {
  if (!range_ok(range)) return TBNAV_ERR_INVALID_ARG;
  int rc = find_frontiers(h, pf, particle, min_cells, info, ms);
  if (rc != TBNAV_OK) return rc;
  if (ms) ms[4] = 0.0f;
  tbnav::DeviceGuard guard(pf->device);
  if (!guard.ok) return TBNAV_ERR_NO_DEVICE;
  rc = ensure_gain_buffers(h);
  if (rc != TBNAV_OK) return rc;
  hipStream_t st = pf->stream;
  std::vector<short> rays;
  ring(range, rays);
  const int n_rays = (int)rays.size() / 2, views = h->finfo.seed_cells;
  if (n_rays > kGainMaxRays) return TBNAV_ERR_UNSUPPORTED;   // (cannot happen: |E(128)| = 788)
  tbnav_nav_gain_info gi{1, range, n_rays, views, 0, 0, {-1, -1}};
  if (views > 0) {
    if (views > h->glist_cap) {
      TBNAV_HIP(dev_alloc(h, h->d_glist, (size_t)views));
      h->glist_cap = views;
    }
    if (h->grays_range != range) {
      h->grays_range = 0;
      TBNAV_HIP(hipMemcpyAsync(h->d_grays, rays.data(), sizeof(short) * rays.size(), hipMemcpyHostToDevice, st));
      TBNAV_HIP(hipStreamSynchronize(st));   // (`rays` goes out of scope with this call)
      h->grays_range = range;
    }
    StageTimer timer(ms != nullptr, 2, st);
    TBNAV_HIP(timer.create());
    TBNAV_HIP(hipMemsetAsync(h->d_gain, 0, sizeof(unsigned) * (size_t)h->n, st));
    TBNAV_HIP(hipMemsetAsync(h->d_gstat, 0, sizeof(unsigned long long) * 3, st));
    TBNAV_HIP(timer.stamp(0));
    // the particle is the find's: where the best one was asked for, rbpf_argmax's index is still in place — nothing of the filter's has run since
    const GainClassArgs ca{pf->pool.lo, pf->pool.bm, particle_ref(pf, particle), pf->cuts.half_lo, pf->cuts.half_hi, h->d_gunk, h->d_gocc};
    hipLaunchKernelGGL(nav_gain_classes, dim3(pf->TW, pf->TW), dim3(kThreads), 0, st, ca);
    TBNAV_HIP(hipGetLastError());
    hipLaunchKernelGGL(nav_gain_list, dim3(64), dim3(256), 0, st, h->d_seed, (int)mask_words(h), h->tiles_y, h->p.ny, h->d_glist, views,
                       reinterpret_cast<unsigned*>(h->d_gstat + 2));
    TBNAV_HIP(hipGetLastError());
    const GainArgs ga{h->d_gunk, h->d_gocc, h->d_glist, h->d_grays, n_rays, range, h->p.nx, h->tiles_y, h->d_gain, h->d_gstat};
    if (range <= kGainSmall) hipLaunchKernelGGL((nav_frontier_gain<kGainSmall>), dim3(views), dim3(kThreads), 0, st, ga);
    else hipLaunchKernelGGL((nav_frontier_gain<TBNAV_NAV_MAX_GAIN_RANGE>), dim3(views), dim3(kThreads), 0, st, ga);
    TBNAV_HIP(hipGetLastError());
    TBNAV_HIP(timer.stamp(1));
    unsigned long long stat[2] = {0, 0};
    TBNAV_HIP(hipMemcpyAsync(stat, h->d_gstat, sizeof stat, hipMemcpyDeviceToHost, st));
    TBNAV_HIP(hipStreamSynchronize(st));
    if (ms) (void)timer.elapsed(0, &ms[4]);
    const unsigned best = 0xFFFFFFFFu - (unsigned)(stat[0] & 0xFFFFFFFFull);
    gi.gain_max = (int32_t)(stat[0] >> 32);
    gi.gain_min = (int32_t)(0xFFFFFFFFu - (unsigned)stat[1]);
    gi.best[0] = (int32_t)(best / (unsigned)h->p.ny); gi.best[1] = (int32_t)(best % (unsigned)h->p.ny);
    h->gain_rmax = range <= kGainSmall ? kGainSmall : TBNAV_NAV_MAX_GAIN_RANGE;
  }
  h->ginfo = gi;
  if (ginfo) *ginfo = gi;
  return TBNAV_OK;
}

// the gain array on the host: zeros where the find left no viewpoint (d_gain was not touched then)
int fetch_gain(tbnav_nav* h) {
  if (h->gain_host_valid) return TBNAV_OK;
  if (h->ginfo.viewpoints == 0) { h->gain_host.assign((size_t)h->n, 0u); h->gain_host_valid = true; return TBNAV_OK; }
  return fetch_once(h, h->d_gain, h->gain_host, h->gain_host_valid);
}

}  // namespace

extern "C" {

int tbnav_nav_gain_rays(int32_t range_cells, int32_t* ends, int32_t cap, int32_t* n) {
  if (!range_ok(range_cells)) return TBNAV_ERR_INVALID_ARG;
  std::vector<short> rays;
  ring(range_cells, rays);
  const int32_t count = (int32_t)(rays.size() / 2);
  if (n) *n = count;
  if (ends && cap < count) return TBNAV_ERR_INVALID_ARG;
  for (size_t i = 0; ends && i < rays.size(); ++i) ends[i] = rays[i];
  return TBNAV_OK;
}

int tbnav_nav_find_frontiers_gain(tbnav_nav* h, tbnav_rbpf* pf, int32_t particle, int32_t min_cells, int32_t range_cells,
                                  tbnav_nav_frontier_info* info, tbnav_nav_gain_info* ginfo) {
  return find_gain(h, pf, particle, min_cells, range_cells, info, ginfo, nullptr);
}

int tbnav_nav_profile_find_frontiers_gain(tbnav_nav* h, tbnav_rbpf* pf, int32_t particle, int32_t min_cells, int32_t range_cells,
                                          tbnav_nav_frontier_info* info, tbnav_nav_gain_info* ginfo, float* stage_ms) {
  if (!stage_ms) return TBNAV_ERR_INVALID_ARG;
  return find_gain(h, pf, particle, min_cells, range_cells, info, ginfo, stage_ms);
}

int tbnav_nav_last_gain(const tbnav_nav* h, tbnav_nav_gain_info* ginfo) {
  if (!h || !ginfo) return TBNAV_ERR_INVALID_ARG;
  *ginfo = h->ginfo;
  return TBNAV_OK;
}

int tbnav_nav_last_gain_kernels(const tbnav_nav* h, char* kernels, int32_t kernels_cap) {
  if (!h || !kernels || kernels_cap <= 0) return TBNAV_ERR_INVALID_ARG;
  if (h->gain_rmax) std::snprintf(kernels, (size_t)kernels_cap, "nav_gain_classes;nav_gain_list;nav_frontier_gain<%d>", h->gain_rmax);
  else kernels[0] = '\0';
  return TBNAV_OK;
}

int tbnav_nav_get_frontier_gain(tbnav_nav* h, uint32_t* gain_host) {
  if (!h || !gain_host || !h->ginfo.computed) return TBNAV_ERR_INVALID_ARG;
  const int rc = fetch_gain(h);
  if (rc != TBNAV_OK) return rc;
  std::memcpy(gain_host, h->gain_host.data(), sizeof(uint32_t) * (size_t)h->n);
  return TBNAV_OK;
}

int tbnav_nav_frontier_gain_list(tbnav_nav* h, tbnav_nav_frontier_gain* out, int32_t cap, int32_t* n) {
  if (!h || !n || cap < 0 || (cap > 0 && !out) || !h->ginfo.computed || !h->finfo.found) return TBNAV_ERR_INVALID_ARG;
  int rc = fetch_once(h, h->d_label, h->label_host, h->label_host_valid);
  if (rc == TBNAV_OK) rc = fetch_gain(h);
  if (rc != TBNAV_OK) return rc;
  *n = h->finfo.clusters;
  if (cap < h->finfo.clusters) return TBNAV_ERR_INVALID_ARG;
  // tbnav_nav_frontier_list's walk: a root is met before any other cell of its cluster, and the roots in ascending order; so is, among
  // the cells with the cluster's most gain, the least
  std::vector<int32_t> slot((size_t)h->n, -1), size;
  const int ny = h->p.ny;
  int32_t k = 0;
  for (int i = 0; i < h->n; ++i) {
    const unsigned l = h->label_host[(size_t)i];
    if (l == kInf) continue;
    if (l == (unsigned)i) {
      if (k >= cap) return TBNAV_ERR_UNSUPPORTED;   // (more roots than the device counted: cannot happen after a find)
      slot[(size_t)i] = k;
      out[k++] = tbnav_nav_frontier_gain{{i / ny, i - (i / ny) * ny}, -1, {-1, -1}};
      size.push_back(0);
    }
    const int32_t s = slot[(size_t)l];
    if (s < 0) return TBNAV_ERR_UNSUPPORTED;        // (a label that is no root: not a fixed point of G12)
    ++size[(size_t)s];
    const int32_t g = (int32_t)h->gain_host[(size_t)i];
    if (g > out[s].gain_max) { out[s].gain_max = g; out[s].best[0] = i / ny; out[s].best[1] = i - (i / ny) * ny; }
  }
  for (int32_t s = 0; s < k; ++s)
    if (size[(size_t)s] < h->finfo.min_cells) out[s] = tbnav_nav_frontier_gain{{out[s].root[0], out[s].root[1]}, 0, {-1, -1}};
  return TBNAV_OK;
}

int tbnav_nav_solve_frontiers_ranked(tbnav_nav* h, int32_t gain_weight) {
  if (!h || !h->finfo.found || !h->ginfo.computed || h->found_cost_epoch != h->cost_epoch || h->found_visited_epoch != h->visited_epoch ||
      gain_weight < 0 || gain_weight > TBNAV_NAV_MAX_GAIN_WEIGHT)
    return TBNAV_ERR_INVALID_ARG;
  if (h->finfo.seed_cells == 0) return TBNAV_ERR_UNSUPPORTED;   // nothing left to explore
  tbnav::DeviceGuard guard(h->device);
  if (!guard.ok) return TBNAV_ERR_NO_DEVICE;
  h->solved = false; h->d_host_valid = false; h->start_host_valid = false;   // from here on the last solution is being overwritten
  const size_t tiles = (size_t)h->tiles_x * h->tiles_y;
  TBNAV_HIP(hipMemsetAsync(h->d_flags, 0, sizeof(unsigned) * 2 * tiles, nullptr));
  hipLaunchKernelGGL(nav_reset_ranked, dim3(256), dim3(256), 0, nullptr, h->d_d, h->d_start, h->p.nx, h->p.ny, h->tiles_y, h->d_seed, h->d_gain, h->d_gstat,
                     (unsigned)gain_weight, h->d_flags);
  TBNAV_HIP(hipGetLastError());
  const int rc = relax_from_start(h, -1, -1);
  if (rc == TBNAV_OK) h->ranked = true;
  return rc;
}

}  // extern "C"

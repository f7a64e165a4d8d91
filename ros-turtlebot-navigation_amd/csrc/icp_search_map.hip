// icp_search_map.hip — the correlative search against a filter particle's MAP instead of a target scan (include/tbnav_icp.h, MAP
// SEARCH, items M1-M9; an addition with no counterpart in the reference).  One kernel forms the likelihood table from the occupancy
// bits in the particle's tiles (TilePool::bm, read through the tile table as nav_cost_from_occ reads them); everything behind the
// table — icp_search_score, icp_search_select, icp_search_shape, the wide stage, search_finish — is icp_search.hip's search_pairs,
// unchanged, on a table that has launch_table's padded layout.  Integers only; restated in tests/icp_search_map_restatement.py.
//   icp_search_table_from_occ  one workgroup of 256 threads per (32 x 32 tile of the table, pair).  S3's stamp depends on
//                              d2 = ox^2 + oy^2 alone and never rises with it (the host checks that while it forms the value-by-d2
//                              table), so M4's maximum over the occupied cells of the (2k+1)^2 square is the stamp AT THE LEAST d2
//                              among them: a nearest-cell search, no atomic maximum.  The workgroup stages the 48 map rows
//                              (ix: the tile's 32 and kHalo = 8 either side) as 48-bit windows of iy, funnel-shifted out of up to
//                              three words each, since the table's origin cx - h2 is aligned to nothing.  Tile id 0, tiles outside
//                              the map and the columns of a ragged last tile read as empty.  A wave's 64 lanes are two map rows of
//                              32 consecutive iy: every staged row is a broadcast read.  A thread walks rows dr = 0 .. k either
//                              side of its cell and takes the nearest set bit left and right within k columns (clz / ffs on the
//                              masked window), stopping at the first dr with dr^2 >= the best so far; then one look into the
//                              value table.  The map's rows are ix with bits along iy and the table is [iy][ix]: the tile is
//                              transposed through LDS, and the workgroup writes ITS part of the padded table — the tile, plus the
//                              border of wl zero cells where the tile touches the table's side, plus the bytes up to tab_stride
//                              behind the last tile — in whole dwords along ix wherever a dword lies wholly inside that part and in
//                              bytes at its ragged ends: no two workgroups write the same byte.  tgt_points is the popcount of the
//                              window's own cells, one atomicAdd per tile that holds any.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "icp_device.hpp"
#include "icp_search_device.hpp"
#include "nav_host.hpp"
#include "tbnav_icp.h"

namespace {

using namespace tbnav_icpdev;

constexpr int kTile = kOccTile;                            // 32: a table tile is as large as a tile of the filter's pool, and a word of it
constexpr int kHalo = kOccHalo;                            // rows and bits staged either side of the tile, whatever k is
constexpr int kRows = kOccRows;                            // 48 staged rows of 48 bits
constexpr int kOutStride = kTile + 4;                      // bytes per transposed row in LDS: 9 dwords, odd, so 32 iy hit 32 banks
constexpr int kOwn = kTile * kTile / kThreads;             // cells per thread
constexpr int kRowStep = kThreads / kTile;
static_assert(kTile == tbnav_rk::kTS && kTile == 32, "a table tile is a tile of the filter's pool");

struct OccArgs {
  const unsigned int* bm;      // TilePool::bm
  const unsigned int* table;   // [N][TT] the particles' tile tables
  const int* best;             // the filter's arg-max on the device (rbpf_argmax), read where a pair asks for it
  int TW, TT, side;            // tiles per side and per map, cells per side
  int n, wl, pside, tab_stride, k;   // the table: side, border, padded side, bytes per pair, stamp half width
  int tiles;                   // table tiles per axis
};

// blockIdx.x: the table tile, ty * tiles + tx (tx along ix); blockIdx.y: the pair of this chunk
__global__ __launch_bounds__(kThreads) void icp_search_table_from_occ(OccArgs a, const MapPair* __restrict__ pairs,
                                                                      const uint8_t* __restrict__ value, uint8_t* __restrict__ tables,
                                                                      uint32_t* __restrict__ tgt_points) {
  __shared__ unsigned long long s_occ[kRows];      // row r: map row X0 - kHalo + r; bit b: map column Y0 - kHalo + b
  __shared__ uint8_t s_val[kMapValues];
  __shared__ uint8_t s_out[kTile * kOutStride];    // [iy][ix] of the tile
  const int tid = threadIdx.x, pair = blockIdx.y;
  const int ty = (int)blockIdx.x / a.tiles, tx = (int)blockIdx.x - ty * a.tiles;
  const MapPair mp = pairs[pair];
  const unsigned int* __restrict__ ids = a.table + (size_t)(mp.particle < 0 ? *a.best : mp.particle) * a.TT;
  const int X0 = mp.ox + tx * kTile, Y0 = mp.oy + ty * kTile;   // the map cell of the tile's cell (0, 0)
  int any = 0;
  if (tid < tbnav_icpdev::kWave) {
    unsigned long long win = 0ull;
    if (tid < kRows) {
      win = occ_row_window(a.bm, ids, a.TW, a.side, X0 - kHalo + tid, Y0 - kHalo);
      s_occ[tid] = win;
      any = win != 0ull;
    }
    // the occupied cells of the window itself: the tile's rows and columns that are cells of the table
    uint32_t cnt = 0u;
    const int ix = tx * kTile + tid - kHalo;
    if (tid >= kHalo && tid < kHalo + kTile && ix < a.n) {
      const int cols = a.n - ty * kTile < kTile ? a.n - ty * kTile : kTile;
      cnt = (uint32_t)__popcll(win & (((1ull << cols) - 1ull) << kHalo));
    }
    cnt = wave_sum_u32(cnt);
    if (tid == 0 && cnt) atomicAdd(&tgt_points[pair], cnt);
  }
  if (tid < kMapValues) s_val[tid] = value[tid];
  any = __syncthreads_or(any);   // (also: the staging is complete)

  if (any) {
    const int k = a.k, c_max = 2 * k * k;
    const int ly = tid & (kTile - 1), c = ly + kHalo;          // this thread's bit in a staged row
#pragma unroll
    for (int j = 0; j < kOwn; ++j) {
      const int lx = (tid >> 5) + j * kRowStep;
      if (tx * kTile + lx >= a.n || ty * kTile + ly >= a.n) continue;   // a ragged table tile: not a cell of the table, never stored
      const int best = nearest_occ_d2(s_occ, lx, c, k);
      s_out[ly * kOutStride + lx] = best <= c_max ? s_val[best] : (uint8_t)0;
    }
  }
  __syncthreads();

  // this workgroup's part of the padded table: rows [ry0, ry1) x columns [rx0, rx1) in padded coordinates
  const int last = a.tiles - 1;
  const int rx0 = tx == 0 ? 0 : a.wl + tx * kTile, rx1 = tx == last ? a.pside : a.wl + (tx + 1) * kTile;
  const int ry0 = ty == 0 ? 0 : a.wl + ty * kTile, ry1 = ty == last ? a.pside : a.wl + (ty + 1) * kTile;
  uint8_t* __restrict__ out = tables + (size_t)pair * (size_t)a.tab_stride;   // (16-byte aligned: tab_stride is a multiple of 16)
  const int cx0 = a.wl + tx * kTile, cy0 = a.wl + ty * kTile;                 // padded coordinates of the tile's cell (0, 0)
  const int lane = tid & 15;
  for (int ry = ry0 + (tid >> 4); ry < ry1; ry += kThreads / 16) {
    const int iy = ry - cy0;
    const bool row_in = any && iy >= 0 && iy < kTile && ty * kTile + iy < a.n;
    const int p0 = ry * a.pside + rx0, p1 = ry * a.pside + rx1;
    for (int d = (p0 >> 2) + lane; d < ((p1 + 3) >> 2); d += 16) {
      uint32_t v = 0u;
      if (row_in) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int ix = 4 * d + q - ry * a.pside - cx0;
          if (ix >= 0 && ix < kTile && tx * kTile + ix < a.n) v |= (uint32_t)s_out[iy * kOutStride + ix] << (8 * q);
        }
      }
      if (4 * d >= p0 && 4 * d + 4 <= p1) {
        *reinterpret_cast<uint32_t*>(out + 4 * d) = v;
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (4 * d + q >= p0 && 4 * d + q < p1) out[4 * d + q] = (uint8_t)(v >> (8 * q));
      }
    }
  }
  if (tx == last && ty == last && tid < a.tab_stride - a.pside * a.pside) out[a.pside * a.pside + tid] = (uint8_t)0;
}

// M1: the handles, the parameters and the particle; M3: the guess.  Nothing is changed.  -> the pairs' frames in `map`
int map_prepare(const tbnav_icp* h, const tbnav_rbpf* pf, const float* scan, int32_t n_beams, int32_t n, const int32_t* particles,
                const double* T_init, MapSource& map) {
  if (!h || !pf || !scan || !particles || !T_init || n < 1 || n_beams <= 0 || n_beams > TBNAV_ICP_MAX_BEAMS) return TBNAV_ERR_INVALID_ARG;
  const tbnav_icp_search_params& sp = h->search.p;
  if (!search_params_ok(sp) || sp.resolution != pf->p.resolution) return TBNAV_ERR_INVALID_ARG;
  for (int i = 0; i < n; ++i)
    if (!tbnav_nk::particle_ok(pf, particles[i])) return TBNAV_ERR_INVALID_ARG;
  if (h->device != pf->device || pf->comm) return TBNAV_ERR_UNSUPPORTED;
  const SearchConst sc = search_const(sp);
  const int h2 = sc.n / 2;
  map.pf = pf;
  map.E = (double)h2 * sp.resolution;
  map.pairs.resize((size_t)n);
  map.local.resize((size_t)n);
  for (int i = 0; i < n; ++i) {
    const double* T = T_init + 3 * (size_t)i;
    if (!std::isfinite(T[0]) || !std::isfinite(T[1]) || !std::isfinite(T[2])) return TBNAV_ERR_OUT_OF_WORLD;
    const double fx = std::floor((T[1] - pf->p.xmin) * sc.inv), fy = std::floor((T[2] - pf->p.ymin) * sc.inv);
    if (!(fx >= 0.0 && fx < (double)pf->xsize && fy >= 0.0 && fy < (double)pf->xsize)) return TBNAV_ERR_OUT_OF_WORLD;
    const int cx = (int)fx, cy = (int)fy;
    map.pairs[(size_t)i] = MapPair{particles[i], cx - h2, cy - h2, 0};
    map.local[(size_t)i] = make_double2(T[1] - (pf->p.xmin + (double)cx * sp.resolution), T[2] - (pf->p.ymin + (double)cy * sp.resolution));
  }
  if (int rc = map_value_table(sp, map.value)) return rc;
  return TBNAV_OK;
}

// what a map search does before its tables: the beam table, the scan as scan 0, every pair reading it, the world guesses, and the
// ICP handle's stream behind whatever the filter's has in flight (M8), the arg-max of its weights included where a pair asks for it
int map_begin(tbnav_icp* h, tbnav_rbpf* pf, const float* scan, int32_t n_beams, int32_t n, const double* T_init, const MapSource& map) {
  IcpSearch& S = h->search;
  if (int rc = ensure_table(h, n_beams)) return rc;
  if (int rc = h->d_scans.reserve(sizeof(float) * (size_t)n_beams)) return rc;
  TBNAV_HIP(hipMemcpyAsync(h->d_scans.ptr, scan, sizeof(float) * (size_t)n_beams, hipMemcpyHostToDevice, h->stream));
  IcpPair pr{};
  pr.tgt = 0; pr.src = 0;
  h->h_pairs.assign((size_t)n, pr);
  h->h_init.resize((size_t)n);
  for (int i = 0; i < n; ++i) h->h_init[(size_t)i] = {T_init[3 * i], T_init[3 * i + 1], T_init[3 * i + 2]};
  bool best = false;
  for (const MapPair& p : map.pairs) best = best || p.particle == TBNAV_ICP_MAP_BEST_PARTICLE;
  if (best)
    if (int rc = tbnav_nk::enqueue_best(pf, TBNAV_NAV_BEST_PARTICLE)) return rc;
  if (!S.map_ev) TBNAV_HIP(hipEventCreateWithFlags(&S.map_ev, hipEventDisableTiming));
  TBNAV_HIP(hipEventRecord(S.map_ev, pf->stream));
  TBNAV_HIP(hipStreamWaitEvent(h->stream, S.map_ev, 0));
  return TBNAV_OK;
}

}  // namespace

namespace tbnav_icpdev {

int map_value_table(const tbnav_icp_search_params& sp, uint8_t* value) {
  const int k = sp.stamp_cells;
  std::memset(value, 0, (size_t)kMapValues);
  for (int c = 0; c <= 2 * k * k; ++c) {
    const double d2 = (double)c * (sp.resolution * sp.resolution);
    value[c] = (uint8_t)std::floor(255.0 * std::exp(-(d2 / (2.0 * (sp.sigma * sp.sigma)))) + 0.5);
    if (c > 0 && value[c] > value[c - 1]) return TBNAV_ERR_UNSUPPORTED;
  }
  return TBNAV_OK;
}

int launch_table_from_occ(tbnav_icp* h, int first, int n, const SearchConst& sc, const MapSource& map) {
  IcpSearch& S = h->search;
  const tbnav_rbpf* pf = map.pf;
  S.h_map.resize((size_t)kMapValues + sizeof(MapPair) * (size_t)n);
  std::memcpy(S.h_map.data(), map.value, (size_t)kMapValues);
  std::memcpy(S.h_map.data() + kMapValues, map.pairs.data() + first, sizeof(MapPair) * (size_t)n);
  if (int rc = S.d_map_in.reserve(S.h_map.size())) return rc;
  TBNAV_HIP(hipMemcpyAsync(S.d_map_in.ptr, S.h_map.data(), S.h_map.size(), hipMemcpyHostToDevice, h->stream));
  TBNAV_HIP(hipMemsetAsync(S.d_tgt_points.ptr, 0, sizeof(uint32_t) * (size_t)n, h->stream));
  const int tiles = (sc.n + kTile - 1) / kTile;
  const OccArgs a{pf->pool.bm, pf->d_table[pf->cur], pf->d_best, pf->TW, pf->TT, pf->xsize, sc.n, sc.wl, sc.side, sc.tab_stride, sc.k, tiles};
  hipLaunchKernelGGL(icp_search_table_from_occ, dim3(tiles * tiles, n), dim3(kThreads), 0, h->stream, a,
                     reinterpret_cast<const MapPair*>(S.d_map_in.as<unsigned char>() + kMapValues), S.d_map_in.as<uint8_t>(),
                     S.d_tables.as<uint8_t>(), S.d_tgt_points.as<uint32_t>());
  TBNAV_HIP(hipGetLastError());
  S.map_ran = true;
  return TBNAV_OK;
}

}  // namespace tbnav_icpdev

namespace {

// the entries' common body.  scores / wide_scores: the test hooks' volumes (n == 1), as search_one's
int map_search(tbnav_icp* h, tbnav_rbpf* pf, const float* scan, int32_t n_beams, int32_t n, const int32_t* particles, const double* T_init,
               tbnav_icp_search_info* infos, uint32_t* scores, bool wide_hook, uint32_t* wide_scores) {
  if (!infos) return TBNAV_ERR_INVALID_ARG;
  MapSource map;
  if (int rc = map_prepare(h, pf, scan, n_beams, n, particles, T_init, map)) return rc;
  IcpSearch& S = h->search;
  tbnav_icp_search_wide_params wp = S.wide_p;
  if (wide_hook) wp.when = TBNAV_ICP_WIDE_ALWAYS;
  const bool wide = wide_hook || (S.wide_on && !scores);
  if (wide && !wide_params_ok(wp, S.p)) return TBNAV_ERR_INVALID_ARG;
  DeviceGuard guard(h->device);
  if (!guard.ok) return TBNAV_ERR_NO_DEVICE;
  if (int rc = map_begin(h, pf, scan, n_beams, n, T_init, map)) return rc;
  if (int rc = search_pairs(h, n, n_beams, S.p, scores, S.shape_on ? &S.shape_p : nullptr, wide ? &wp : nullptr, wide_scores, &map)) return rc;
  for (int i = 0; i < n; ++i) infos[i] = h->h_sinfo[(size_t)i];
  S.last = h->h_sinfo[(size_t)n - 1];
  S.last_shape = h->h_sshape[(size_t)n - 1];
  S.last_wide = h->h_swide[(size_t)n - 1];
  return TBNAV_OK;
}

}  // namespace

extern "C" {

int tbnav_icp_search_map(tbnav_icp* h, tbnav_rbpf* pf, int32_t particle, const float* scan, int32_t n_beams, const double T_init[3],
                         tbnav_icp_search_info* info) {
  return map_search(h, pf, scan, n_beams, 1, &particle, T_init, info, nullptr, false, nullptr);
}

int tbnav_icp_search_map_batch(tbnav_icp* h, tbnav_rbpf* pf, const float* scan, int32_t n_beams, int32_t n, const int32_t* particles,
                               const double* T_init, tbnav_icp_search_info* infos) {
  return map_search(h, pf, scan, n_beams, n, particles, T_init, infos, nullptr, false, nullptr);
}

int tbnav_icp_search_map_scores(tbnav_icp* h, tbnav_rbpf* pf, int32_t particle, const float* scan, int32_t n_beams, const double T_init[3],
                                tbnav_icp_search_info* info, uint32_t* scores) {
  if (!scores) return TBNAV_ERR_INVALID_ARG;
  return map_search(h, pf, scan, n_beams, 1, &particle, T_init, info, scores, false, nullptr);
}

int tbnav_icp_search_map_wide_scores(tbnav_icp* h, tbnav_rbpf* pf, int32_t particle, const float* scan, int32_t n_beams,
                                     const double T_init[3], tbnav_icp_search_info* info, uint32_t* scores) {
  return map_search(h, pf, scan, n_beams, 1, &particle, T_init, info, nullptr, true, scores);
}

int tbnav_icp_search_map_table(tbnav_icp* h, tbnav_rbpf* pf, int32_t particle, const double T_init[3], uint8_t* table, uint32_t* tgt_points) {
  if (!table || !tgt_points) return TBNAV_ERR_INVALID_ARG;
  MapSource map;
  const float none = 0.0f;   // (no scan takes part: M4 is the map's alone)
  if (int rc = map_prepare(h, pf, &none, 1, 1, &particle, T_init, map)) return rc;
  DeviceGuard guard(h->device);
  if (!guard.ok) return TBNAV_ERR_NO_DEVICE;
  IcpSearch& S = h->search;
  SearchConst sc = search_const(S.p);
  sc.E = map.E;
  if (int rc = S.d_tables.reserve((size_t)sc.tab_stride)) return rc;
  if (int rc = S.d_tgt_points.reserve(sizeof(uint32_t))) return rc;
  if (particle == TBNAV_ICP_MAP_BEST_PARTICLE)
    if (int rc = tbnav_nk::enqueue_best(pf, TBNAV_NAV_BEST_PARTICLE)) return rc;
  if (!S.map_ev) TBNAV_HIP(hipEventCreateWithFlags(&S.map_ev, hipEventDisableTiming));
  TBNAV_HIP(hipEventRecord(S.map_ev, pf->stream));
  TBNAV_HIP(hipStreamWaitEvent(h->stream, S.map_ev, 0));
  TBNAV_HIP(hipMemsetAsync(S.d_tables.ptr, 0xff, (size_t)sc.tab_stride, h->stream));   // every byte is the kernel's to write
  if (int rc = launch_table_from_occ(h, 0, 1, sc, map)) return rc;
  std::vector<uint8_t> padded((size_t)sc.tab_stride);
  TBNAV_HIP(hipMemcpyAsync(padded.data(), S.d_tables.ptr, padded.size(), hipMemcpyDeviceToHost, h->stream));
  TBNAV_HIP(hipMemcpyAsync(tgt_points, S.d_tgt_points.ptr, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  TBNAV_HIP(hipStreamSynchronize(h->stream));
  // the border and the bytes behind the table are part of what the kernel owes the scoring kernels: all zero
  for (int i = 0; i < sc.tab_stride; ++i) {
    const int ry = i / sc.side, rx = i - ry * sc.side;
    const bool in = ry >= sc.wl && ry < sc.wl + sc.n && rx >= sc.wl && rx < sc.wl + sc.n;
    if (!in && padded[(size_t)i] != 0) return TBNAV_ERR_HIP;
  }
  for (int iy = 0; iy < sc.n; ++iy)
    std::memcpy(table + (size_t)iy * sc.n, padded.data() + (size_t)(iy + sc.wl) * sc.side + sc.wl, (size_t)sc.n);
  return TBNAV_OK;
}

int tbnav_icp_last_map_kernel(const tbnav_icp* h, char* kernel, int32_t kernel_cap) {
  if (!h || !kernel || kernel_cap <= 0) return TBNAV_ERR_INVALID_ARG;
  std::snprintf(kernel, (size_t)kernel_cap, "%s", h->search.map_ran ? "icp_search_table_from_occ" : "");
  return TBNAV_OK;
}

}  // extern "C"

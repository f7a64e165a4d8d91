// icp_search_device.hpp — what the correlative search's kernels (icp_search.hip) and the kernel that measures the shape of
// its score volume (icp_search_shape.hip) share: the by-value constants, the per-pair input and result, the cell of a
// coordinate, the names of the wave reductions they use (wave.hpp) and the scoring front (load_table, base_cells, slow_read: what icp_search_score and
// icp_search_shape do before they score, and how either reads a table byte for a point of the slow list), and what the search against
// a filter's map (icp_search_map.hip) hands to search_pairs in place of target scans (MapPair, MapSource), and the nearest occupied
// cell of a filter's map (occ_row_window, nearest_occ_d2), which that file's table kernel and the global search's field kernel
// (icp_global.hip) both call.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <vector>

#include "icp_device.hpp"
#include "tbnav_icp.h"

namespace tbnav_icpdev {

struct SearchConst {
  double E, inv;
  int n, side, wl, wa, k, nl, na;   // side = n + 2*wl
  int tab_stride;                   // bytes of one padded table, a multiple of 16
  unsigned slack;
};

struct SearchPair {
  int32_t tgt, src;
  double x0, y0;
};

// what the host reads per pair
struct SearchSel {
  uint32_t score, lin, count, points, tgt_points, thr;
};

// floor((v + E) * inv) as an int; false: not a number, or so far out that neither a stamp nor a window reaches the table
__device__ __forceinline__ bool cell_of(double v, double E, double inv, int& c) {
  const double f = floor((v + E) * inv);
  if (!(f >= -65536.0 && f <= 65536.0)) return false;
  c = (int)f;
  return true;
}

using tbnav::wave_max_u64; using tbnav::wave_sum_u32; using tbnav::wave_sum_i64;   // (wave.hpp)

// ---- the scoring front.  Dynamic LDS of a scoring kernel: the padded table, then uint16 cells[n_beams], the fast list
// growing up from 0 and the slow list down from n_beams - 1 (compacted by atomics: a sum of integers has no order) ----
inline size_t score_lds_bytes(const SearchConst& sc, int n_beams) {
  return (size_t)sc.tab_stride + ((sizeof(uint16_t) * (size_t)n_beams + 15) & ~(size_t)15);
}

// the pair's padded table into LDS in whole uint4s; the caller synchronises
__device__ __forceinline__ void load_table(uint4* lds_tab, const uint8_t* __restrict__ tables, int pair, const SearchConst& sc, int t) {
  const uint4* src = reinterpret_cast<const uint4*>(tables + (size_t)pair * (size_t)sc.tab_stride);
  for (int i = t; i < sc.tab_stride / 16; i += kThreads) lds_tab[i] = src[i];
}

// the base cells of source scan ss rotated by cs = (cos, sin) and moved by (pr.x0, pr.y0), this thread's beams t, t + B, ...
// A base cell inside the table goes to the fast list as the first cell of its window in the padded table (rows by .. by + 2*wl,
// columns bx .. bx + 2*wl, all inside it); one outside it whose window reaches in goes to the slow list as its padded
// coordinates (0 .. side - 1 <= 207 each), to be read with slow_read.  *n_fast and *n_slow are LDS counters the caller zeroed
// before a barrier; the caller synchronises.  Returns this thread's count of valid points.
__device__ __forceinline__ uint32_t base_cells(const float* __restrict__ ss, const float2* __restrict__ beams, int n_beams,
                                               const IcpConst& k, const SearchConst& sc, double2 cs, const SearchPair& pr,
                                               uint16_t* cells, uint32_t* n_fast, uint32_t* n_slow, int t) {
  uint32_t valid = 0u;
  for (int i = t; i < n_beams; i += kThreads) {
    float2 p;
    if (!cloud_point(ss[i], beams[i], k, p)) continue;
    ++valid;
    const double sx = (double)p.x, sy = (double)p.y;
    const double ax = (((cs.x * sx) - (cs.y * sy)) + pr.x0);
    const double ay = (((cs.y * sx) + (cs.x * sy)) + pr.y0);
    int bx, by;
    if (!cell_of(ax, sc.E, sc.inv, bx) || !cell_of(ay, sc.E, sc.inv, by)) continue;
    if (bx >= 0 && bx < sc.n && by >= 0 && by < sc.n) {
      cells[atomicAdd(n_fast, 1u)] = (uint16_t)(by * sc.side + bx);
    } else if (bx >= -sc.wl && bx < sc.n + sc.wl && by >= -sc.wl && by < sc.n + sc.wl) {
      cells[n_beams - 1 - (int)atomicAdd(n_slow, 1u)] = (uint16_t)(((by + sc.wl) << 8) | (bx + sc.wl));
    }
  }
  return valid;
}

// what the slow-list point v adds to the candidate at (iy, ix) of the window: the table byte its cell holds, 0 outside the table
__device__ __forceinline__ uint32_t slow_read(const uint8_t* tab, const SearchConst& sc, int v, int iy, int ix) {
  const int ry = (v >> 8) + iy - sc.wl, rx = (v & 0xff) + ix - sc.wl;   // padded coordinates of the cell this candidate reads
  if (ry >= sc.wl && ry < sc.n + sc.wl && rx >= sc.wl && rx < sc.n + sc.wl) return tab[ry * sc.side + rx];
  return 0u;
}

// the seven integers of F3 for one pair, 64 bytes
struct ShapeRec {
  long long S0, Sx, Sy, Sxx, Sxy, Syy;
  uint32_t cells, pad0;
  long long pad1;
};
static_assert(sizeof(ShapeRec) == 64, "one 64-byte record per pair");

// icp_search_shape.hip: icp_search_shape over the n pairs of a chunk, after the final icp_search_select on h->stream
// (d_sel holds the choice) -> h->search.d_shape[0, n), which the caller reserved
int launch_shape(tbnav_icp* h, int n, int n_beams, const SearchConst& sc, const SearchPair* d_pairs, const double2* d_rot,
                 const tbnav_icp_search_shape_params& shp);
// F4, F5, F6 on the host: the record of one pair from its integers; info->T becomes the shaped T
void shape_finish(const ShapeRec& r, const tbnav_icp_search_params& sp, const tbnav_icp_search_shape_params& shp,
                  const double T_init[3], tbnav_icp_search_info* info, tbnav_icp_search_shape* out);
bool shape_params_ok(const tbnav_icp_search_shape_params& p);

// icp_search.hip: S7 on the host, the record of one pair from its selection (sc and sp name the window: the wide stage calls it
// with wl := W, wa := A)
void search_finish(const SearchSel& s, const SearchConst& sc, const tbnav_icp_search_params& sp, const double T_init[3],
                   tbnav_icp_search_info* info);

// icp_search_wide.hip (WIDE WINDOW, W1-W8).  wide_params_ok: W1's limits against the search parameters sp.  wide_stage: the wide
// stage for the pairs esc (places in the chunk that starts at pair `first`, whose tables d_tables and target counts are still
// on the device, d_pairs its SearchPairs) -> h->h_sinfo / h->h_sshape of those pairs; it synchronises h->stream once.
// scores (one pair only): the wide score volume, or null.  shp: the shape over the wide window, or null.
bool wide_params_ok(const tbnav_icp_search_wide_params& wp, const tbnav_icp_search_params& sp);
int wide_stage(tbnav_icp* h, int first, const std::vector<int>& esc, int n_beams, const tbnav_icp_search_params& sp,
               const SearchConst& sc, const SearchPair* d_pairs, const tbnav_icp_search_wide_params& wp, uint32_t* scores,
               const tbnav_icp_search_shape_params* shp);

// icp_search_map.hip (MAP SEARCH, M1-M9): a particle's map in place of a target scan.  One MapPair per pair goes to the device;
// MapSource is what search_pairs needs to know of the route: E' (M3) for SearchConst::E, the local guesses for SearchPair::x0 / y0
// (h->h_init keeps the WORLD T_init for search_finish, shape_finish and the wide stage's angles), and the table's source.
constexpr int kMapValues = (2 * TBNAV_ICP_SEARCH_MAX_STAMP * TBNAV_ICP_SEARCH_MAX_STAMP + 1 + 15) & ~15;   // 144 bytes: whole uint4s
struct MapPair {
  int32_t particle;   // a slot, or TBNAV_ICP_MAP_BEST_PARTICLE: the filter's arg-max, on the device
  int32_t ox, oy;     // the map cell of table cell [0][0]: (cx - h2, cy - h2), anywhere relative to the map
  int32_t pad;
};
struct MapSource {
  const tbnav_rbpf* pf;
  double E;                        // E' = (double)h2 * resolution
  std::vector<MapPair> pairs;      // [n_pairs]
  std::vector<double2> local;      // [n_pairs] (x0 - o.x, y0 - o.y)
  uint8_t value[kMapValues];       // S3's stamp by d2 = ox^2 + oy^2, 0 .. 2k^2 (M4)
};
// ---- the nearest occupied cell of a filter's map, what icp_search_table_from_occ (icp_search_map.hip) and icp_global_field
// (icp_global.hip) both stand on.  A workgroup stages kOccRows map rows (a tile's 32 and kOccHalo either side) as kOccRows-bit
// windows of the map's columns; a cell then looks at rows dr = 0 .. k either side of its own. ----
constexpr int kOccTile = 32;                               // a tile of the filter's pool, and a word of it
constexpr int kOccHalo = TBNAV_ICP_SEARCH_MAX_STAMP;       // rows and bits staged either side of the tile, whatever k is
constexpr int kOccRows = kOccTile + 2 * kOccHalo;          // 48 staged rows of 48 bits
static_assert(kOccRows <= 64 && kOccRows <= kWave, "a staged row is one 64-bit window, and one wave stages them all");

// bits g0 .. g0 + kOccRows - 1 of map row mx (bit b: map column g0 + b), funnel-shifted out of up to three words read through the
// particle's tile table ids ([TW][TW]; tile id 0, tiles outside the map, rows outside it and the columns of a ragged last tile read as
// empty).  g0 may be anywhere relative to the map.
__device__ __forceinline__ unsigned long long occ_row_window(const unsigned int* __restrict__ bm, const unsigned int* __restrict__ ids,
                                                             int TW, int side, int mx, int g0) {
  const int w0 = g0 >> 5, o = g0 & 31;                      // (an arithmetic shift: floor for a window that starts left of the map)
  unsigned int w[3] = {0u, 0u, 0u};
  if (mx >= 0 && mx < side) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int wy = w0 + j;
      if (wy < 0 || wy >= TW) continue;
      const unsigned int id = ids[(mx >> 5) * TW + wy];
      if (id != 0u) w[j] = bm[(size_t)id * kOccTile + (mx & (kOccTile - 1))];
      const int inside = side - wy * kOccTile;                // columns of this tile that are cells of the map (>= 1)
      if (inside < kOccTile) w[j] &= (1u << inside) - 1u;
    }
  }
  unsigned long long win = (((unsigned long long)w[1] << 32) | w[0]) >> o;
  if (o > 64 - kOccRows) win |= (unsigned long long)w[2] << (64 - o);
  return win & ((1ull << kOccRows) - 1ull);
}

// the least dr^2 + dc^2 over the set bits within k rows and k columns of bit c (kOccHalo .. kOccHalo + 31) of staged row
// kOccHalo + lx, or 1 << 20 where there is none: rows outwards, the nearest set bit left and right of c in each (clz / ffs on the
// masked window), stopping at the first dr with dr^2 >= the best so far
__device__ __forceinline__ int nearest_occ_d2(const unsigned long long* s_occ, int lx, int c, int k) {
  const unsigned int m = (1u << (k + 1)) - 1u;
  int best = 1 << 20;
  for (int dr = 0; dr <= k && dr * dr < best; ++dr) {
    for (int s = 0; s < (dr == 0 ? 1 : 2); ++s) {
      const unsigned long long row = s_occ[kOccHalo + lx + (s ? dr : -dr)];   // rows 0 .. 47: dr <= k <= kOccHalo
      const unsigned int left = (unsigned int)(row >> (c - k)) & m;           // bit q: column offset q - k
      const unsigned int right = (unsigned int)(row >> c) & m;                // bit q: column offset q
      if (left) {
        const int dc = k - (31 - __clz((int)left));
        const int d2 = dr * dr + dc * dc;
        best = d2 < best ? d2 : best;
      }
      if (right) {
        const int dc = __ffs((int)right) - 1;
        const int d2 = dr * dr + dc * dc;
        best = d2 < best ? d2 : best;
      }
    }
  }
  return best;
}

// icp_search_map.hip: S3's stamp by d2 = ox^2 + oy^2, 0 .. 2k^2, into value[kMapValues]; TBNAV_ERR_UNSUPPORTED should it ever rise
// with d2 (M4's nearest-cell form stands on its never rising)
int map_value_table(const tbnav_icp_search_params& sp, uint8_t* value);

// icp_search.hip: S1's limits, and the constants of parameters that keep them
bool search_params_ok(const tbnav_icp_search_params& p);
SearchConst search_const(const tbnav_icp_search_params& p);
// icp_search_table_from_occ over the pairs [first, first + n) of map -> d_tables, d_tgt_points (launch_table's layout), on h->stream
int launch_table_from_occ(tbnav_icp* h, int first, int n, const SearchConst& sc, const MapSource& map);

}  // namespace tbnav_icpdev

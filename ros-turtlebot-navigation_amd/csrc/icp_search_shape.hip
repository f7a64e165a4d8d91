// icp_search_shape.hip — the shape of the correlative search's score volume (include/tbnav_icp.h, CORRELATIVE SEARCH, items F1-F6;
// an addition with no counterpart in the reference).  A corridor's high scores form a ridge along it and a room's a compact blob:
// the second moments of the chosen angle's slice tell the two apart, and the guess is kept along a direction the scan cannot see.
//   icp_search_shape   one workgroup of 256 threads per pair, behind the final icp_search_select: it reads the choice
//                      (sel[pair]: lin -> ia, score = best), scores that one angle again exactly as icp_search_score does,
//                      through the same scoring front (icp_search_device.hpp: load_table, base_cells, slow_read; the padded
//                      table and the base cells in LDS, a fast list and a bounds-tested slow list), with its own loop: up to 5
//                      translations per thread in one instantiation, a runtime loop over them, the points innermost.  It forms
//                      w = score - floor of F2 and the seven integers of F3, and reduces them with wave shuffles and one LDS
//                      stage: integers have no order.  One 64-byte record per pair.
// F4 / F5 are the host's (shape_finish below, fp64 without contraction: -ffp-contract=off, csrc/Makefile), where S7 runs; the
// record comes back in the synchronisation that brings the selection back (icp_search.hip).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "common.hpp"
#include "icp_device.hpp"
#include "icp_search_device.hpp"
#include "tbnav_icp.h"

namespace {

using namespace tbnav_icpdev;

constexpr int kSlots = 5;      // translations per thread: nl^2 <= 33^2 = 1089 <= 5 * 256
constexpr int kSums = 7;       // S0, Sx, Sy, Sxx, Sxy, Syy, cells
static_assert((2 * TBNAV_ICP_SEARCH_MAX_LIN + 1) * (2 * TBNAV_ICP_SEARCH_MAX_LIN + 1) <= kSlots * kThreads, "the slots do not hold the window");

// blockIdx.x: the pair.  The scoring is icp_search_score's for the one angle sel[pair] names, behind the same front.
__global__ __launch_bounds__(kThreads) void icp_search_shape(const float* __restrict__ scans, const float* __restrict__ stored,
                                                             const float2* __restrict__ beams, int n_beams,
                                                             const SearchPair* __restrict__ pairs, const double2* __restrict__ rot,
                                                             const uint8_t* __restrict__ tables, const SearchSel* __restrict__ sel,
                                                             ShapeRec* __restrict__ out, IcpConst k, SearchConst sc, unsigned drop) {
  extern __shared__ uint4 lds_tab[];                                    // the padded table, then the cells
  const uint8_t* tab = reinterpret_cast<const uint8_t*>(lds_tab);
  uint16_t* cells = reinterpret_cast<uint16_t*>(lds_tab + sc.tab_stride / 16);  // [n_beams]: fast list up from 0, slow list down from the end
  __shared__ uint32_t n_fast, n_slow;
  __shared__ long long red[kThreads / kWave][kSums + 1];
  const int t = threadIdx.x;
  const int pair = blockIdx.x;
  load_table(lds_tab, tables, pair, sc, t);
  if (t == 0) { n_fast = 0u; n_slow = 0u; }
  __syncthreads();
  const int n_cand = sc.nl * sc.nl;
  const SearchSel choice = sel[pair];
  int ia = (int)(choice.lin / (uint32_t)n_cand);
  ia = ia < sc.na ? ia : sc.na - 1;                                     // lin < na * nl^2 by construction; never index past rot
  const uint32_t best = choice.score;
  const uint32_t floor_ = best - (uint32_t)(((unsigned long long)best * drop) >> 10);
  const SearchPair pr = pairs[pair];
  const double2 cs = rot[(size_t)pair * sc.na + ia];
  const float* ss = pr.src < 0 ? stored : scans + (size_t)pr.src * n_beams;
  (void)base_cells(ss, beams, n_beams, k, sc, cs, pr, cells, &n_fast, &n_slow, t);
  __syncthreads();
  const int nf = (int)n_fast, ns = (int)n_slow;
  const int per = (n_cand + kThreads - 1) / kThreads;                   // 1 .. kSlots, the same for every thread
  long long s[kSums] = {0, 0, 0, 0, 0, 0, 0};
  // one translation at a time, the points innermost: the inner loops hold no branch, so their LDS reads are issued in
  // batches (with the translations innermost behind a runtime count every read waited for the one before it: 37-99 us a
  // launch where icp_search_score takes 12-22)
  for (int j = 0; j < per; ++j) {
    const int q = t + j * kThreads;
    const bool in = q < n_cand;
    const int iy = in ? q / sc.nl : 0;
    const int ix = in ? q - iy * sc.nl : 0;
    const int off = iy * sc.side + ix;                                  // a slot past the window reads candidate 0's cells and is dropped
    uint32_t acc = 0u;
#pragma unroll 8
    for (int p = 0; p < nf; ++p) acc += tab[(int)cells[p] + off];
    for (int p = 0; p < ns; ++p) acc += slow_read(tab, sc, cells[n_beams - 1 - p], iy, ix);
    if (!in || acc <= floor_) continue;
    const long long w = (long long)(acc - floor_);
    const long long dx = ix - sc.wl, dy = iy - sc.wl;
    s[0] += w;
    s[1] += w * dx;
    s[2] += w * dy;
    s[3] += w * dx * dx;
    s[4] += w * dx * dy;
    s[5] += w * dy * dy;
    s[6] += 1;
  }
#pragma unroll
  for (int i = 0; i < kSums; ++i) {
    s[i] = wave_sum_i64(s[i]);
    if ((t & (kWave - 1)) == 0) red[t / kWave][i] = s[i];
  }
  __syncthreads();
  if (t == 0) {
#pragma unroll
    for (int i = 0; i < kSums; ++i) {
      s[i] = red[0][i];
#pragma unroll
      for (int w = 1; w < kThreads / kWave; ++w) s[i] += red[w][i];
    }
    ShapeRec r;
    r.S0 = s[0]; r.Sx = s[1]; r.Sy = s[2]; r.Sxx = s[3]; r.Sxy = s[4]; r.Syy = s[5];
    r.cells = (uint32_t)s[6];
    r.pad0 = 0u;
    r.pad1 = 0;
    out[pair] = r;
  }
}

}  // namespace

namespace tbnav_icpdev {

bool shape_params_ok(const tbnav_icp_search_shape_params& p) {
  return p.drop_q10 >= 0 && p.drop_q10 <= 1023 && std::isfinite(p.flat_cells2) && p.flat_cells2 > 0.0;
}

int launch_shape(tbnav_icp* h, int n, int n_beams, const SearchConst& sc, const SearchPair* d_pairs, const double2* d_rot,
                 const tbnav_icp_search_shape_params& shp) {
  IcpSearch& S = h->search;
  hipLaunchKernelGGL(icp_search_shape, dim3(n), dim3(kThreads), score_lds_bytes(sc, n_beams), h->stream, h->d_scans.as<float>(),
                     h->d_stored.as<float>(), h->d_table, n_beams, d_pairs, d_rot, S.d_tables.as<uint8_t>(), S.d_sel.as<SearchSel>(),
                     S.d_shape.as<ShapeRec>(), h->k, sc, (unsigned)shp.drop_q10);
  TBNAV_HIP(hipGetLastError());
  return TBNAV_OK;
}

void shape_finish(const ShapeRec& r, const tbnav_icp_search_params& sp, const tbnav_icp_search_shape_params& shp,
                  const double T_init[3], tbnav_icp_search_info* info, tbnav_icp_search_shape* out) {
  tbnav_icp_search_shape o{};
  o.S0 = r.S0; o.Sx = r.Sx; o.Sy = r.Sy; o.Sxx = r.Sxx; o.Sxy = r.Sxy; o.Syy = r.Syy;
  o.cells = (int32_t)r.cells;
  o.T_raw[0] = info->T[0]; o.T_raw[1] = info->T[1]; o.T_raw[2] = info->T[2];
  o.computed = 1;
  if (r.S0 > 0) {
    // F4
    const double S0 = (double)r.S0;
    const double mx = (double)r.Sx / S0, my = (double)r.Sy / S0;
    const double a = ((double)r.Sxx / S0) - (mx * mx);
    const double b = ((double)r.Sxy / S0) - (mx * my);
    const double c = ((double)r.Syy / S0) - (my * my);
    const double hd = 0.5 * (a - c);
    const double hh = std::sqrt((hd * hd) + (b * b));
    o.l1 = (0.5 * (a + c)) + hh;
    o.l2 = (0.5 * (a + c)) - hh;
    const double vx = hd >= 0.0 ? hd + hh : b;
    const double vy = hd >= 0.0 ? b : hh - hd;
    const double n = std::sqrt((vx * vx) + (vy * vy));
    o.ex = n > 0.0 ? vx / n : 1.0;
    o.ey = n > 0.0 ? vy / n : 0.0;
    // F5
    if (o.l1 > shp.flat_cells2) {
      double dx = 0.0, dy = 0.0;
      if (o.l2 > shp.flat_cells2) {
        o.kind = 2;
      } else {
        o.kind = 1;
        const double d0 = (double)(info->ix - sp.lin_cells), d1 = (double)(info->iy - sp.lin_cells);
        const double p = (d0 * o.ex) + (d1 * o.ey);
        dx = d0 - (p * o.ex);
        dy = d1 - (p * o.ey);
      }
      info->T[1] = T_init[1] + (dx * sp.resolution);
      info->T[2] = T_init[2] + (dy * sp.resolution);
    }
  }
  *out = o;
}

}  // namespace tbnav_icpdev

extern "C" {

void tbnav_icp_default_search_shape_params(tbnav_icp_search_shape_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof *p);
  p->drop_q10 = 256;
  p->flat_cells2 = 2.0;
}

int tbnav_icp_set_search_shape(tbnav_icp* h, const tbnav_icp_search_shape_params* params) {
  if (!h) return TBNAV_ERR_INVALID_ARG;
  if (!params) {
    h->search.shape_on = false;
    tbnav_icp_default_search_shape_params(&h->search.shape_p);
    return TBNAV_OK;
  }
  if (!shape_params_ok(*params)) return TBNAV_ERR_INVALID_ARG;
  h->search.shape_p = *params;
  h->search.shape_p.reserved = 0;
  h->search.shape_on = true;
  return TBNAV_OK;
}

int tbnav_icp_get_search_shape(const tbnav_icp* h, int32_t* on, tbnav_icp_search_shape_params* params) {
  if (!h) return TBNAV_ERR_INVALID_ARG;
  if (on) *on = h->search.shape_on ? 1 : 0;
  if (params) *params = h->search.shape_p;
  return TBNAV_OK;
}

int tbnav_icp_last_search_shape(const tbnav_icp* h, tbnav_icp_search_shape* shape) {
  if (!h || !shape) return TBNAV_ERR_INVALID_ARG;
  *shape = h->search.last_shape;
  return TBNAV_OK;
}

}  // extern "C"

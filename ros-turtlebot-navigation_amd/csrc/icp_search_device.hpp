// icp_search_device.hpp — what the correlative search's kernels (icp_search.hip) and the kernel that measures the shape of
// its score volume (icp_search_shape.hip) share: the by-value constants, the per-pair input and result, the cell of a
// coordinate and the wave reductions.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

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

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(v, off, kWave);
    v = o > v ? o : v;
  }
  return v;
}

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off, kWave);
  return v;
}

// the seven integers of F3 for one pair, 64 bytes
struct ShapeRec {
  long long S0, Sx, Sy, Sxx, Sxy, Syy;
  uint32_t cells, pad0;
  long long pad1;
};
static_assert(sizeof(ShapeRec) == 64, "one 64-byte record per pair");

// icp_search_shape.hip: icp_search_shape over the n pairs of a chunk, after the final icp_search_select on h->stream
// (d_sel holds the choice) -> h->search.d_shape[0, n)
int launch_shape(tbnav_icp* h, int n, int n_beams, const SearchConst& sc, const SearchPair* d_pairs, const double2* d_rot,
                 const tbnav_icp_search_shape_params& shp);
// F4, F5, F6 on the host: the record of one pair from its integers; info->T becomes the shaped T
void shape_finish(const ShapeRec& r, const tbnav_icp_search_params& sp, const tbnav_icp_search_shape_params& shp,
                  const double T_init[3], tbnav_icp_search_info* info, tbnav_icp_search_shape* out);
bool shape_params_ok(const tbnav_icp_search_shape_params& p);

}  // namespace tbnav_icpdev

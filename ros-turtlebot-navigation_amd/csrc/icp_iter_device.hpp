// icp_iter_device.hpp — what the alignment kernels share inside an iteration: icp_align (icp.hip, scan against scan) and
// icp_align_map (icp_align_map.hip, scan against a filter particle's map; include/tbnav_icp.h, MAP ALIGNMENT).  The line
// metric's sums (L3) and Gauss-Newton step (L4), the header's fixed summation tree (item 3), and the composition with the
// stopping rules (items 3 and 4).  One definition each: both kernels are held to their restatements bit for bit, and both files
// are compiled with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

#include "icp_device.hpp"
#include "tbnav_icp.h"

namespace tbnav_icpdev {

constexpr int kLineSums = 10;   // H00, H01, H02, H11, H12, H22, g0, g1, g2, Sr

// L3: what a kept pair adds: a the transformed source point, b the point of the line, n its normal, all in doubles
__device__ __forceinline__ void line_add(double (&sum)[kLineSums], double ax, double ay, double bx, double by, double nx, double ny) {
  const double ex = ax - bx, ey = ay - by;
  const double r = (nx * ex) + (ny * ey);
  const double jj = (ax * ny) - (ay * nx);
  sum[0] += jj * jj; sum[1] += jj * nx; sum[2] += jj * ny;
  sum[3] += nx * nx; sum[4] += nx * ny; sum[5] += ny * ny;
  sum[6] += jj * r; sum[7] += nx * r; sum[8] += ny * r;
  sum[9] += r * r;
}

// L4: the increment from the totals of n >= 3 pairs (theta eliminated last); mse is assigned first; false: degenerate
__device__ __forceinline__ bool line_step(const double* tot, int n, double min_cond, double& c, double& s, double& tix, double& tiy,
                                          double& mse) {
  const double H00 = tot[0], H01 = tot[1], H02 = tot[2], H11 = tot[3], H12 = tot[4], H22 = tot[5];
  const double g0 = tot[6], g1 = tot[7], g2 = tot[8];
  mse = tot[9] / (double)n;
  const double tr = H11 + H22;
  const double det = (H11 * H22) - (H12 * H12);
  if (!(det > min_cond * (tr * tr))) return false;
  const double v1 = ((H22 * H01) - (H12 * H02)) / det;
  const double v2 = ((H11 * H02) - (H12 * H01)) / det;
  const double dth = H00 - ((H01 * v1) + (H02 * v2));
  if (!(dth > min_cond * H00)) return false;
  const double th = -(g0 - ((v1 * g1) + (v2 * g2))) / dth;
  const double w1 = g1 + (H01 * th), w2 = g2 + (H02 * th);
  tix = -((H22 * w1) - (H12 * w2)) / det;
  tiy = -((H11 * w2) - (H12 * w1)) / det;
  const double u = 0.5 * th;
  const double q = 1.0 + (u * u);
  c = (1.0 - (u * u)) / q; s = th / q;
  return true;
}

// the LDS of item 3's tree over kThreads threads with NS fp64 sums and the pair count
template <int NS>
struct TreeLds {
  double red_a[NS][kThreads / 2];   // s = 128 partials
  double red_b[NS][kThreads / 4];   // s = 64 partials
  int cnt_a[kThreads / 2], cnt_b[kThreads / 4];
  double tot[NS];
  int tot_n;
};

// item 3's tree: t += t + s for s = 128, 64 (LDS), 32 .. 1 (wave 0, shuffles); the totals are in L.tot / L.tot_n for every thread
// behind the last of its three barriers.  The next writes of red_a / red_b / tot come after the next call's first / second
// barrier, which every thread reaches only after it has read the totals.
template <int NS>
__device__ __forceinline__ void tree_totals(TreeLds<NS>& L, double (&sum)[NS], int cnt, int t) {
  if (t >= kThreads / 2) {
#pragma unroll
    for (int q = 0; q < NS; ++q) L.red_a[q][t - kThreads / 2] = sum[q];
    L.cnt_a[t - kThreads / 2] = cnt;
  }
  __syncthreads();
  if (t < kThreads / 2) {
#pragma unroll
    for (int q = 0; q < NS; ++q) sum[q] = sum[q] + L.red_a[q][t];
    cnt += L.cnt_a[t];
    if (t >= kThreads / 4) {
#pragma unroll
      for (int q = 0; q < NS; ++q) L.red_b[q][t - kThreads / 4] = sum[q];
      L.cnt_b[t - kThreads / 4] = cnt;
    }
  }
  __syncthreads();
  if (t < kWave) {
#pragma unroll
    for (int q = 0; q < NS; ++q) sum[q] = sum[q] + L.red_b[q][t];
    cnt += L.cnt_b[t];
#pragma unroll
    for (int s = kWave / 2; s > 0; s >>= 1) {
#pragma unroll
      for (int q = 0; q < NS; ++q) sum[q] = sum[q] + __shfl_down(sum[q], s, kWave);
      cnt += __shfl_down(cnt, s, kWave);
    }
    if (t == 0) {
#pragma unroll
      for (int q = 0; q < NS; ++q) L.tot[q] = sum[q];
      L.tot_n = cnt;
    }
  }
  __syncthreads();
}

// the accumulated transform and the last mse the REL / ABS rules compare with
struct IcpState {
  double R00, R01, R10, R11, tx, ty;
  double prev;   // starts at DBL_MAX
};

// R <- R_inc * R, t <- R_inc * t + t_inc (item 3), then item 4's rules in their order: the criterion that stops the loop after
// iteration `iter`, or TBNAV_ICP_NOT_RUN to go on (prev = mse then)
__device__ __forceinline__ int advance(IcpState& S, double c, double s, double tix, double tiy, double mse, int iter, const IcpConst& k) {
  const double n00 = (c * S.R00) - (s * S.R10), n01 = (c * S.R01) - (s * S.R11);
  const double n10 = (s * S.R00) + (c * S.R10), n11 = (s * S.R01) + (c * S.R11);
  const double ntx = ((c * S.tx) - (s * S.ty)) + tix, nty = ((s * S.tx) + (c * S.ty)) + tiy;
  S.R00 = n00; S.R01 = n01; S.R10 = n10; S.R11 = n11; S.tx = ntx; S.ty = nty;
  if (iter >= k.max_iter) return TBNAV_ICP_ITERATIONS;
  if (c >= k.rot_thresh && ((tix * tix) + (tiy * tiy)) <= k.trans_thresh) return TBNAV_ICP_TRANSFORM;
  const double dm = fabs(mse - S.prev);
  if (dm < 1e-12) return TBNAV_ICP_ABS_MSE;
  if (dm / S.prev < k.fitness_eps) return TBNAV_ICP_REL_MSE;
  S.prev = mse;
  return TBNAV_ICP_NOT_RUN;
}

}  // namespace tbnav_icpdev

// icp.hip — ICP between laser scans, point-to-point and (as an option) point-to-line (include/tbnav_icp.h): the reference's
// ScanAlignment::pclICP / pclICPWrapper (bmapping/src/bmapping/cloud_alignment.cpp:37-223) restated on the device.
//
// One kernel, icp_align<Metric, P, C>, and two metrics.  One workgroup of kThreads threads aligns one (target, source) pair;
// the whole iteration loop runs inside the launch.
//   - the target cloud lives in LDS as float2, one slot per BEAM (an invalid beam holds NaN, which never wins the strict
//     '<' of the nearest-neighbour scan, so the scan order over the valid points is the compacted cloud's order); the
//     scan runs as C independent chains per point (latency: one wave per SIMD), merged in (distance, index) order;
//   - thread t keeps the source beams t, t + B, ... (P of them, a template parameter) in registers, untransformed;
//   - per iteration: transform, nearest neighbour against every target, the metric's fp64 sums in the header's fixed order
//     (per thread in increasing beam, then the tree t += t + s: s = 128 and 64 through LDS, 32..1 by shuffles in wave 0),
//     and wave 0 leaves the totals in LDS; after ONE barrier every thread computes R_inc and the stopping criteria from
//     them redundantly (wave-uniform), so the loop needs no further barrier and no global memory.
// A metric (PointMetric, LineMetric) supplies what differs: how many sums there are, what a kept pair adds to them, and how
// the increment (c, s, tix, tiy) and mse come out of the totals.  PointMetric is the reference's: nine sums and a closed-form
// rotation.  LineMetric is the header's POINT-TO-LINE METRIC (an addition; the reference has no such metric): the target's
// normals as a second float2 array in LDS beside the cloud, computed by the workgroup before the loop, ten sums, and a 3x3
// Gauss-Newton step solved by every thread from the totals.
// The line metric's sums and step, the tree and the composition with the stopping rules are icp_iter_device.hpp's, which
// icp_align_map (icp_align_map.hip, the alignment to a filter's map) calls too.
// Compiled with -ffp-contract=off (csrc/Makefile): every fp64 / fp32 expression keeps the restatement's rounding.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstring>
#include <map>
#include <new>
#include <vector>

#include "common.hpp"
#include "icp_device.hpp"
#include "icp_iter_device.hpp"
#include "tbnav_icp.h"

namespace {

using namespace tbnav_icpdev;   // the handle, the kernel constants and cloud_point (icp_device.hpp)

// the target cloud of scan ts into LDS, one slot per beam, padded to whole float4 pairs of points; NaN for what is not a point
__device__ __forceinline__ void load_target(float2* tgt, const float* __restrict__ ts, const float2* __restrict__ table, int n_beams,
                                            int n4, const IcpConst& k, int t) {
  const float qnan = __builtin_nanf("");
  for (int i = t; i < n4; i += kThreads) {
    float2 p = make_float2(qnan, qnan);
    if (i < n_beams && !cloud_point(ts[i], table[i], k, p)) p = make_float2(qnan, qnan);
    tgt[i] = p;
  }
}

// the normal of target beam i from the LDS cloud (one slot per beam, NaN where there is no point: a NaN distance fails the
// gap test, so invalid beams inside the window are skipped); false: no normal
__device__ __forceinline__ bool target_normal(const float2* tgt, int i, int n_beams, const IcpLine& ln, float2& nrm) {
  const float2 p = tgt[i];
  if (!(p.x == p.x)) return false;
  int lo = i, hi = i;
  const int first = i - ln.window > 0 ? i - ln.window : 0;
  const int last = i + ln.window < n_beams - 1 ? i + ln.window : n_beams - 1;
  for (int j = first; j < i; ++j) {
    const float2 q = tgt[j];
    const float dx = q.x - p.x, dy = q.y - p.y;
    const float d = dx * dx + dy * dy;
    if ((double)d <= ln.gap2) { lo = j; break; }
  }
  for (int j = last; j > i; --j) {
    const float2 q = tgt[j];
    const float dx = q.x - p.x, dy = q.y - p.y;
    const float d = dx * dx + dy * dy;
    if ((double)d <= ln.gap2) { hi = j; break; }
  }
  if (lo == hi) return false;
  const float2 a = tgt[lo], b = tgt[hi];
  const double tx = (double)b.x - (double)a.x, ty = (double)b.y - (double)a.y;
  const double l = sqrt((tx * tx) + (ty * ty));
  if (l == 0.0) return false;
  nrm.x = (float)(-ty / l);
  nrm.y = (float)(tx / l);
  return true;
}

// ---- the two metrics: what icp_align does not share ----
// kSums: the fp64 sums of the header (the pair count n is counted apart, as an int).  kNormals: the kernel keeps the target's
// normals in LDS beside the cloud and hands add() the nearest target's.  kMaxBeams: what fits in LDS.  Params: the metric's
// by-value kernel parameters.
//   add(sum, a, b, nf, d): a kept pair (transformed source a, nearest target b with normal nf at fp32 squared distance d)
//     into the thread's sums; false: the pair does not count.
//   step(tot, n, mp, c, s, tix, tiy, mse): the increment from the totals of n >= 3 pairs; mse is assigned first; false: degenerate.

// the reference's point-to-point metric: Sax, Say, Sbx, Sby, Sxx, Syy, Sxy, Syx, Sd and the closed-form 2-D rotation
struct PointMetric {
  static constexpr int kSums = 9;
  static constexpr bool kNormals = false;
  static constexpr int kMaxBeams = TBNAV_ICP_MAX_BEAMS;
  struct Params {};
  static __device__ __forceinline__ bool add(double (&sum)[kSums], float2 a, float2 b, float2, float d) {
    const double ax = a.x, ay = a.y, bx = b.x, by = b.y;
    sum[0] += ax; sum[1] += ay; sum[2] += bx; sum[3] += by;
    sum[4] += ax * bx; sum[5] += ay * by; sum[6] += ax * by; sum[7] += ay * bx;
    sum[8] += (double)d;
    return true;
  }
  static __device__ __forceinline__ bool step(const double* tot, int n, const Params&, double& c, double& s, double& tix,
                                              double& tiy, double& mse) {
    const double dn = (double)n;
    const double Sax = tot[0], Say = tot[1], Sbx = tot[2], Sby = tot[3];
    const double A = (tot[4] + tot[5]) - ((Sax * Sbx) + (Say * Sby)) / dn;
    const double S = (tot[6] - tot[7]) - ((Sax * Sby) - (Say * Sbx)) / dn;
    const double r = sqrt((A * A) + (S * S));
    mse = tot[8] / dn;
    if (r == 0.0) return false;
    c = A / r; s = S / r;
    const double amx = Sax / dn, amy = Say / dn, bmx = Sbx / dn, bmy = Sby / dn;
    tix = bmx - ((c * amx) - (s * amy));
    tiy = bmy - ((s * amx) + (c * amy));
    return true;
  }
};

// the point-to-line metric (tbnav_icp.h, POINT-TO-LINE METRIC; no counterpart in the reference): H00, H01, H02, H11, H12,
// H22, g0, g1, g2, Sr and the 3x3 Gauss-Newton step (theta eliminated last)
struct LineMetric {
  static constexpr int kSums = kLineSums;
  static constexpr bool kNormals = true;
  static constexpr int kMaxBeams = TBNAV_ICP_LINE_MAX_BEAMS;
  using Params = IcpLine;
  static __device__ __forceinline__ bool add(double (&sum)[kSums], float2 a, float2 b, float2 nf, float) {
    if (!(nf.x == nf.x)) return false;  // the nearest target has no normal
    line_add(sum, (double)a.x, (double)a.y, (double)b.x, (double)b.y, (double)nf.x, (double)nf.y);   // (icp_iter_device.hpp)
    return true;
  }
  static __device__ __forceinline__ bool step(const double* tot, int n, const Params& ln, double& c, double& s, double& tix,
                                              double& tiy, double& mse) {
    return line_step(tot, n, ln.min_cond, c, s, tix, tiy, mse);
  }
};

template <class M, int P, int C = (P <= 2 ? 4 : P <= 4 ? 2 : 1)>
__global__ __launch_bounds__(kThreads) void icp_align(const float* __restrict__ scans, const float* __restrict__ stored,
                                                        const float2* __restrict__ table, int n_beams,
                                                        const IcpPair* __restrict__ pairs, IcpOut* __restrict__ out, IcpConst k,
                                                        typename M::Params mp) {
  constexpr int NS = M::kSums;
  extern __shared__ float4 lds_dyn[];          // 16-byte aligned: the nearest-neighbour scan reads it as float4
  const int n4 = (n_beams + 3) & ~3;           // the LDS cloud is padded to whole float4 pairs of points with NaN
  float2* tgt = reinterpret_cast<float2*>(lds_dyn);  // [n4]
  float2* nrm = tgt + n4;                            // [n4], M::kNormals only (NaN: no normal)
  __shared__ TreeLds<NS> tree;                // the partials of s = 128 and 64, and the totals (icp_iter_device.hpp)

  const int t = threadIdx.x;
  const IcpPair pr = pairs[blockIdx.x];
  const float* ts = pr.tgt < 0 ? stored : scans + (size_t)pr.tgt * n_beams;
  const float* ss = pr.src < 0 ? stored : scans + (size_t)pr.src * n_beams;
  load_target(tgt, ts, table, n_beams, n4, k, t);
  float2 src[P];
  bool valid[P];
#pragma unroll
  for (int j = 0; j < P; ++j) {
    const int i = t + j * kThreads;
    valid[j] = i < n_beams && cloud_point(ss[i], table[i], k, src[j]);
    if (!valid[j]) src[j] = make_float2(0.0f, 0.0f);
  }
  __syncthreads();
  if constexpr (M::kNormals) {
    for (int i = t; i < n4; i += kThreads) {
      float2 v;
      if (!(i < n_beams && target_normal(tgt, i, n_beams, mp, v))) v = make_float2(__builtin_nanf(""), __builtin_nanf(""));
      nrm[i] = v;
    }
    __syncthreads();
  }

  IcpState st{pr.c, -pr.s, pr.s, pr.c, pr.x, pr.y, DBL_MAX};
  double mse = 0.0;
  int iter = 0, n = 0, crit = TBNAV_ICP_NOT_RUN;
  while (true) {
    ++iter;
    double sum[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) sum[q] = 0.0;
    int cnt = 0;
    float2 a[P];
    float best[P][C];
    int bi[P][C];
#pragma unroll
    for (int j = 0; j < P; ++j) {
      a[j].x = (float)(((st.R00 * (double)src[j].x) + (st.R01 * (double)src[j].y)) + st.tx);
      a[j].y = (float)(((st.R10 * (double)src[j].x) + (st.R11 * (double)src[j].y)) + st.ty);
#pragma unroll
      for (int c = 0; c < C; ++c) { best[j][c] = __builtin_huge_valf(); bi[j][c] = 0x7fffffff; }
    }
    // nearest neighbour: C independent chains per point (chain c: targets m = c mod C, in increasing m, strict '<'), four
    // targets per two 16-byte LDS reads (a broadcast: every lane reads the same address).  The loop stays in the kernel's
    // body, not in a helper, and compares by selects, not branches: so its body is one basic block in every instantiation.
    for (int m = 0; m < n4; m += 4) {
      const float4 t01 = *reinterpret_cast<const float4*>(&tgt[m]);
      const float4 t23 = *reinterpret_cast<const float4*>(&tgt[m + 2]);
      const float bx[4] = {t01.x, t01.z, t23.x, t23.z}, by[4] = {t01.y, t01.w, t23.y, t23.w};
#pragma unroll
      for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int j = 0; j < P; ++j) {
          const float dx = a[j].x - bx[r], dy = a[j].y - by[r];
          const float d = dx * dx + dy * dy;
          const bool lt = d < best[j][r % C];
          best[j][r % C] = lt ? d : best[j][r % C];
          bi[j][r % C] = lt ? m + r : bi[j][r % C];
        }
      }
    }
    // the chains' minima in (distance, index) order: the lowest index among equal distances, as one scan in beam order
#pragma unroll
    for (int j = 0; j < P; ++j) {
#pragma unroll
      for (int c = 1; c < C; ++c) {
        if (best[j][c] < best[j][0] || (best[j][c] == best[j][0] && bi[j][c] < bi[j][0])) { best[j][0] = best[j][c]; bi[j][0] = bi[j][c]; }
      }
    }
    // the gate, and what the metric makes of a pair inside it
#pragma unroll
    for (int j = 0; j < P; ++j) {
      if (valid[j] && (double)best[j][0] <= k.max_corr2) {
        const float2 b = tgt[bi[j][0]];
        float2 nf = make_float2(0.0f, 0.0f);
        if constexpr (M::kNormals) nf = nrm[bi[j][0]];
        if (M::add(sum, a[j], b, nf, best[j][0])) ++cnt;
      }
    }
    // the tree; then every thread: R_inc and the criteria from the totals (wave-uniform from here to the loop's end)
    tree_totals(tree, sum, cnt, t);
    n = tree.tot_n;
    if (n < 3) { crit = TBNAV_ICP_NO_CORRESPONDENCES; mse = 0.0; break; }
    // step() assigns all four or returns false.  The zeros are never read, but left undefined on the degenerate path they
    // cost most instantiations registers (8-10 VGPRs at P = 2, which is a workgroup per CU in a batch of the line metric)
    double c = 0.0, s = 0.0, tix = 0.0, tiy = 0.0;
    if (!M::step(tree.tot, n, mp, c, s, tix, tiy, mse)) { crit = TBNAV_ICP_DEGENERATE; break; }
    crit = advance(st, c, s, tix, tiy, mse, iter, k);
    if (crit != TBNAV_ICP_NOT_RUN) break;
  }
  if (t == 0) {
    IcpOut o;
    o.R00 = st.R00; o.R10 = st.R10; o.tx = st.tx; o.ty = st.ty; o.mse = mse;
    o.iterations = iter; o.correspondences = n; o.criterion = crit; o.pad = 0;
    out[blockIdx.x] = o;
  }
}

// the normals of one scan taken as a target, per beam (test hook): one workgroup, the same cloud_point / target_normal as the
// alignment; a beam without a normal gets (0, 0) and has = 0
__global__ __launch_bounds__(kThreads) void icp_normals(const float* __restrict__ scan, const float2* __restrict__ table, int n_beams,
                                                        float2* __restrict__ nxy, int* __restrict__ has, IcpConst k, IcpLine ln) {
  extern __shared__ float4 lds_dyn[];
  float2* tgt = reinterpret_cast<float2*>(lds_dyn);
  const int t = threadIdx.x;
  const int n4 = (n_beams + 3) & ~3;
  load_target(tgt, scan, table, n_beams, n4, k, t);
  __syncthreads();
  for (int i = t; i < n_beams; i += kThreads) {
    float2 v = make_float2(0.0f, 0.0f);
    const bool ok = target_normal(tgt, i, n_beams, ln, v);
    nxy[i] = ok ? v : make_float2(0.0f, 0.0f);
    has[i] = ok ? 1 : 0;
  }
}

// the cloud of one scan, per beam (test hook; the same cloud_point as the alignment)
__global__ __launch_bounds__(kThreads) void icp_cloud(const float* __restrict__ scan, const float2* __restrict__ table, int n_beams,
                                                      float2* __restrict__ xy, int* __restrict__ valid, IcpConst k) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n_beams) return;
  float2 p = make_float2(0.0f, 0.0f);
  valid[i] = cloud_point(scan[i], table[i], k, p) ? 1 : 0;
  xy[i] = p;
}

bool converged(int crit) { return crit >= TBNAV_ICP_ITERATIONS && crit <= TBNAV_ICP_REL_MSE; }

}  // namespace

namespace tbnav_icpdev {

int ensure_table(tbnav_icp* h, int n_beams) {
  if (h->table_beams == n_beams) return TBNAV_OK;
  // createPointCloud's beam angles (cloud_alignment.cpp:120-154): float angle, std::cos(float) = glibc cosf
  std::vector<float2> tab((size_t)n_beams);
  const float bmin = h->p.beam_min, bmax = h->p.beam_max, bd = h->p.beam_delta;
  float ang = bmin;
  for (int i = 0; i < n_beams; ++i) {
    tab[(size_t)i] = make_float2(std::cos(ang), std::sin(ang));
    ang += bd;
    if (bmax < 0.0 && ang <= bmax) ang = bmin;
    else if (bmax >= 0.0 && ang >= bmax) ang = bmin;
  }
  if (h->d_table) TBNAV_HIP(hipFree(h->d_table));
  h->d_table = nullptr;
  h->table_beams = 0;
  TBNAV_HIP(hipMalloc(&h->d_table, sizeof(float2) * (size_t)n_beams));
  TBNAV_HIP(hipMemcpyAsync(h->d_table, tab.data(), sizeof(float2) * (size_t)n_beams, hipMemcpyHostToDevice, h->stream));
  TBNAV_HIP(hipStreamSynchronize(h->stream));  // tab is about to go out of scope
  h->table_beams = n_beams;
  return TBNAV_OK;
}

}  // namespace tbnav_icpdev

namespace {

IcpPair make_pair(int tgt, int src, const double T[3]) {
  // pclICP's guess (cloud_alignment.cpp:171-183): float cos / sin / x / y
  IcpPair p;
  p.tgt = tgt; p.src = src;
  p.c = (double)(float)std::cos(T[0]);
  p.s = (double)(float)std::sin(T[0]);
  p.x = (double)(float)T[1];
  p.y = (double)(float)T[2];
  return p;
}

// one more alignment for run_pairs: the pair, and its guess as given (the correlative search starts from the doubles)
void add_pair(tbnav_icp* h, int tgt, int src, const double T[3]) {
  h->h_pairs.push_back(make_pair(tgt, src, T));
  h->h_init.push_back({T[0], T[1], T[2]});
}

void clear_pairs(tbnav_icp* h) {
  h->h_pairs.clear();
  h->h_init.clear();
}

// one launch of icp_align<M, P> over h->d_pairs.  Dynamic LDS: the cloud, 8 bytes per beam rounded up to 4 beams, and as much
// again for the normals of a metric that keeps them
template <class M, int P>
int launch(tbnav_icp* h, int n_pairs, int n_beams) {
  const size_t lds = (M::kNormals ? 2 : 1) * sizeof(float2) * (size_t)((n_beams + 3) & ~3);
  typename M::Params mp{};
  if constexpr (M::kNormals) mp = h->line;
  hipLaunchKernelGGL((icp_align<M, P>), dim3(n_pairs), dim3(kThreads), lds, h->stream, h->d_scans.as<float>(), h->d_stored.as<float>(),
                     h->d_table, n_beams, h->d_pairs.as<IcpPair>(), h->d_out.as<IcpOut>(), h->k, mp);
  TBNAV_HIP(hipGetLastError());
  return TBNAV_OK;
}

// source beams per thread -> P; the ladder ends at the P that holds the metric's kMaxBeams (n_beams <= kMaxBeams: beams_ok)
template <class M>
int dispatch(tbnav_icp* h, int n_pairs, int n_beams) {
  static_assert(M::kMaxBeams <= 16 * kThreads, "no instantiation holds kMaxBeams");
  const int per = (n_beams + kThreads - 1) / kThreads;
  if (per <= 1) return launch<M, 1>(h, n_pairs, n_beams);
  if (per <= 2) return launch<M, 2>(h, n_pairs, n_beams);
  if (per <= 3) return launch<M, 3>(h, n_pairs, n_beams);
  if (per <= 4) return launch<M, 4>(h, n_pairs, n_beams);
  if (per <= 6) return launch<M, 6>(h, n_pairs, n_beams);
  if constexpr (M::kMaxBeams <= 8 * kThreads) {
    return launch<M, 8>(h, n_pairs, n_beams);
  } else {
    if (per <= 8) return launch<M, 8>(h, n_pairs, n_beams);
    if (per <= 12) return launch<M, 12>(h, n_pairs, n_beams);
    return launch<M, 16>(h, n_pairs, n_beams);
  }
}

// the beam counts the handle's metric can align
bool beams_ok(const tbnav_icp* h, int n_beams) {
  return n_beams > 0 && n_beams <= (h->metric == TBNAV_ICP_METRIC_LINE ? LineMetric::kMaxBeams : PointMetric::kMaxBeams);
}

// aligns h->h_pairs[0, n_pairs) (scans already in d_scans / d_stored) -> h->h_out, with the handle's metric.  With the
// correlative search on (tbnav_icp_set_search) every pair is searched first -> h->h_sinfo, and an accepted search's pose
// replaces the pair's guess: one host round trip between the search and the alignment (the guess is formed here, with glibc).
int run_pairs(tbnav_icp* h, int n_pairs, int n_beams) {
  if (int rc = h->d_pairs.reserve(sizeof(IcpPair) * (size_t)n_pairs)) return rc;
  if (int rc = h->d_out.reserve(sizeof(IcpOut) * (size_t)n_pairs)) return rc;
  if (h->search.on) {
    if (int rc = search_pairs(h, n_pairs, n_beams, h->search.p, nullptr, h->search.shape_on ? &h->search.shape_p : nullptr,
                              h->search.wide_on ? &h->search.wide_p : nullptr)) return rc;
    for (int i = 0; i < n_pairs; ++i) {
      const tbnav_icp_search_info& si = h->h_sinfo[(size_t)i];
      if (si.accepted) h->h_pairs[(size_t)i] = make_pair(h->h_pairs[(size_t)i].tgt, h->h_pairs[(size_t)i].src, si.T);
    }
  } else {
    h->h_sinfo.assign((size_t)n_pairs, tbnav_icp_search_info{});
    h->h_sshape.assign((size_t)n_pairs, tbnav_icp_search_shape{});
    h->h_swide.assign((size_t)n_pairs, tbnav_icp_search_wide_info{});
  }
  TBNAV_HIP(hipMemcpyAsync(h->d_pairs.ptr, h->h_pairs.data(), sizeof(IcpPair) * (size_t)n_pairs, hipMemcpyHostToDevice, h->stream));
  const bool line = h->metric == TBNAV_ICP_METRIC_LINE;
  if (int rc = line ? dispatch<LineMetric>(h, n_pairs, n_beams) : dispatch<PointMetric>(h, n_pairs, n_beams)) return rc;
  h->h_out.resize((size_t)n_pairs);
  TBNAV_HIP(hipMemcpyAsync(h->h_out.data(), h->d_out.ptr, sizeof(IcpOut) * (size_t)n_pairs, hipMemcpyDeviceToHost, h->stream));
  TBNAV_HIP(hipStreamSynchronize(h->stream));
  ++h->last_launches;
  return TBNAV_OK;
}

// the test hooks' scratch in d_scans, 4 floats per beam: the uploaded scan at its start, then the flags [n_beams] int and the
// values [n_beams] float2 that the hook's kernel writes
int hook_scratch(tbnav_icp* h, const float* scan, int n_beams, int*& flags, float2*& xy) {
  if (int rc = h->d_scans.reserve(sizeof(float) * 4 * (size_t)n_beams)) return rc;
  flags = reinterpret_cast<int*>(h->d_scans.as<float>() + n_beams);
  xy = reinterpret_cast<float2*>(h->d_scans.as<float>() + 2 * (size_t)n_beams);  // 8-byte aligned
  TBNAV_HIP(hipMemcpyAsync(h->d_scans.ptr, scan, sizeof(float) * (size_t)n_beams, hipMemcpyHostToDevice, h->stream));
  return TBNAV_OK;
}

void result(const IcpOut& o, double T_out[3], tbnav_icp_info* info) {
  if (converged(o.criterion)) {
    T_out[0] = std::atan2(o.R10, o.R00);  // pclICP :209 (on the fp64 state, header note)
    T_out[1] = o.tx;
    T_out[2] = o.ty;
  } else {
    T_out[0] = T_out[1] = T_out[2] = 0.0;
  }
  if (info) {
    info->iterations = o.iterations;
    info->correspondences = o.correspondences;
    info->mse = o.mse;
    info->criterion = o.criterion;
    info->reserved = 0;
  }
}

void first_call(double T_out[3], int32_t* ok, tbnav_icp_info* info) {
  T_out[0] = T_out[1] = T_out[2] = 0.0;
  if (ok) *ok = 1;
  if (info) *info = tbnav_icp_info{0, 0, 0.0, TBNAV_ICP_NOT_RUN, 0};
}

int store_scan(tbnav_icp* h, const float* dev_src, const float* host_src, int n_beams) {
  if (int rc = h->d_stored.reserve(sizeof(float) * (size_t)n_beams)) return rc;
  if (dev_src) TBNAV_HIP(hipMemcpyAsync(h->d_stored.ptr, dev_src, sizeof(float) * (size_t)n_beams, hipMemcpyDeviceToDevice, h->stream));
  else TBNAV_HIP(hipMemcpyAsync(h->d_stored.ptr, host_src, sizeof(float) * (size_t)n_beams, hipMemcpyHostToDevice, h->stream));
  TBNAV_HIP(hipStreamSynchronize(h->stream));
  h->stored_beams = n_beams;
  h->have_stored = true;
  return TBNAV_OK;
}

}  // namespace

extern "C" {

void tbnav_icp_default_params(tbnav_icp_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof *p);
  p->max_iter = 100;
  p->max_corr_dist = 0.5;
  p->transform_eps = 1e-8;
  p->fitness_eps = 1e-6;
  p->device = -1;
}

int tbnav_icp_create(const tbnav_icp_params* params, tbnav_icp** out) {
  if (!params || !out) return TBNAV_ERR_INVALID_ARG;
  *out = nullptr;
  // max_corr_dist^2 must be finite: a point with no nearest target (an empty target cloud, a guess that is not a number) is
  // left at distance +inf with no index, and only a finite gate keeps it from being taken for a pair
  if (params->max_iter < 1 || params->max_iter > TBNAV_ICP_MAX_ITER || !(params->max_corr_dist > 0.0) ||
      !std::isfinite(params->max_corr_dist * params->max_corr_dist) || !(params->transform_eps >= 0.0) ||
      !(params->fitness_eps >= 0.0))
    return TBNAV_ERR_INVALID_ARG;
  int dev = 0;
  if (const int rc = tbnav::pick_device(params->device, &dev)) return rc;
  DeviceGuard guard(dev);
  if (!guard.ok) return TBNAV_ERR_NO_DEVICE;
  tbnav_icp* h = new (std::nothrow) tbnav_icp();
  if (!h) return TBNAV_ERR_INVALID_ARG;
  h->p = *params;
  h->device = dev;
  tbnav_icp_default_search_params(&h->search.p);
  tbnav_icp_default_search_shape_params(&h->search.shape_p);
  tbnav_icp_default_search_wide_params(&h->search.wide_p);
  IcpConst& k = h->k;
  k.range_min = params->range_min;
  k.range_max = params->range_max;
  k.trs_c = std::cos(params->Trs[0]);  // Transform2D(Vector2D, theta) (rigid2d.hpp)
  k.trs_s = std::sin(params->Trs[0]);
  k.trs_x = params->Trs[1];
  k.trs_y = params->Trs[2];
  k.max_corr2 = params->max_corr_dist * params->max_corr_dist;
  k.rot_thresh = 1.0 - params->transform_eps;
  k.trans_thresh = params->transform_eps;
  k.fitness_eps = params->fitness_eps;
  k.max_iter = params->max_iter;
  const hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    delete h;
    return tbnav::hip_fail(e, "hipStreamCreateWithFlags", __FILE__, __LINE__);
  }
  *out = h;
  return TBNAV_OK;
}

void tbnav_icp_destroy(tbnav_icp* h) {
  if (!h) return;
  {
    DeviceGuard guard(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    (void)hipFree(h->d_table);
    for (DevBuf* b : {&h->d_stored, &h->d_scans, &h->d_pairs, &h->d_out, &h->d_align_in, &h->d_align_rec, &h->d_verify_in, &h->d_verify_out, &h->d_verify_rec}) b->release();
    search_free(h);
    global_free(h);
    if (h->stream) (void)hipStreamDestroy(h->stream);
  }
  delete h;
}

int tbnav_icp_reset(tbnav_icp* h) {
  if (!h) return TBNAV_ERR_INVALID_ARG;
  h->have_stored = false;
  h->stored_beams = 0;
  return TBNAV_OK;
}

int tbnav_icp_last_batch_launches(const tbnav_icp* h) { return h ? h->last_launches : 0; }

int tbnav_icp_set_metric(tbnav_icp* h, int32_t metric, int32_t normal_window, double normal_max_gap) {
  if (!h || (metric != TBNAV_ICP_METRIC_POINT && metric != TBNAV_ICP_METRIC_LINE) || normal_window > TBNAV_ICP_LINE_MAX_WINDOW)
    return TBNAV_ERR_INVALID_ARG;
  // a stored scan the line metric has no LDS for cannot be kept
  if (metric == TBNAV_ICP_METRIC_LINE && h->have_stored && h->stored_beams > TBNAV_ICP_LINE_MAX_BEAMS) return TBNAV_ERR_INVALID_ARG;
  h->metric = metric;
  h->line.window = normal_window > 0 ? normal_window : TBNAV_ICP_LINE_NORMAL_WINDOW;
  h->line_gap = normal_max_gap > 0.0 ? normal_max_gap : TBNAV_ICP_LINE_NORMAL_MAX_GAP;  // NaN selects the default too
  h->line.gap2 = h->line_gap * h->line_gap;
  return TBNAV_OK;
}

int tbnav_icp_get_metric(const tbnav_icp* h, int32_t* metric, int32_t* normal_window, double* normal_max_gap) {
  if (!h) return TBNAV_ERR_INVALID_ARG;
  if (metric) *metric = h->metric;
  if (normal_window) *normal_window = h->line.window;
  if (normal_max_gap) *normal_max_gap = h->line_gap;
  return TBNAV_OK;
}

int tbnav_icp_normals(tbnav_icp* h, const float* scan, int32_t n_beams, float* nxy, int32_t* has) {
  if (!h || !scan || !nxy || !has || n_beams <= 0 || n_beams > TBNAV_ICP_LINE_MAX_BEAMS) return TBNAV_ERR_INVALID_ARG;
  DeviceGuard guard(h->device);
  if (!guard.ok) return TBNAV_ERR_NO_DEVICE;
  if (int rc = ensure_table(h, n_beams)) return rc;
  int* d_has;
  float2* d_nxy;
  if (int rc = hook_scratch(h, scan, n_beams, d_has, d_nxy)) return rc;
  hipLaunchKernelGGL(icp_normals, dim3(1), dim3(kThreads), sizeof(float2) * (size_t)((n_beams + 3) & ~3), h->stream,
                     h->d_scans.as<float>(), h->d_table, (int)n_beams, d_nxy, d_has, h->k, h->line);
  TBNAV_HIP(hipGetLastError());
  TBNAV_HIP(hipMemcpyAsync(nxy, d_nxy, sizeof(float2) * (size_t)n_beams, hipMemcpyDeviceToHost, h->stream));
  TBNAV_HIP(hipMemcpyAsync(has, d_has, sizeof(int32_t) * (size_t)n_beams, hipMemcpyDeviceToHost, h->stream));
  TBNAV_HIP(hipStreamSynchronize(h->stream));
  return TBNAV_OK;
}

int tbnav_icp_cloud(tbnav_icp* h, const float* scan, int32_t n_beams, float* xy, int32_t* n_points) {
  if (!h || !scan || !xy || !n_points || n_beams <= 0 || n_beams > TBNAV_ICP_MAX_BEAMS) return TBNAV_ERR_INVALID_ARG;
  DeviceGuard guard(h->device);
  if (!guard.ok) return TBNAV_ERR_NO_DEVICE;
  if (int rc = ensure_table(h, n_beams)) return rc;
  int* d_valid;
  float2* d_xy;
  if (int rc = hook_scratch(h, scan, n_beams, d_valid, d_xy)) return rc;
  hipLaunchKernelGGL(icp_cloud, dim3((n_beams + kThreads - 1) / kThreads), dim3(kThreads), 0, h->stream, h->d_scans.as<float>(),
                     h->d_table, (int)n_beams, d_xy, d_valid, h->k);
  TBNAV_HIP(hipGetLastError());
  std::vector<float2> pts((size_t)n_beams);
  std::vector<int> valid((size_t)n_beams);
  TBNAV_HIP(hipMemcpyAsync(pts.data(), d_xy, sizeof(float2) * (size_t)n_beams, hipMemcpyDeviceToHost, h->stream));
  TBNAV_HIP(hipMemcpyAsync(valid.data(), d_valid, sizeof(int) * (size_t)n_beams, hipMemcpyDeviceToHost, h->stream));
  TBNAV_HIP(hipStreamSynchronize(h->stream));
  int m = 0;
  for (int i = 0; i < n_beams; ++i)
    if (valid[(size_t)i]) { xy[2 * m] = pts[(size_t)i].x; xy[2 * m + 1] = pts[(size_t)i].y; ++m; }
  *n_points = m;
  return TBNAV_OK;
}

int tbnav_icp_match(tbnav_icp* h, const float* target_scan, const float* source_scan, int32_t n_beams, const double T_init[3],
                    double T_out[3], tbnav_icp_info* info) {
  if (!h || !target_scan || !source_scan || !T_init || !T_out || !info || !beams_ok(h, n_beams))
    return TBNAV_ERR_INVALID_ARG;
  DeviceGuard guard(h->device);
  if (!guard.ok) return TBNAV_ERR_NO_DEVICE;
  if (int rc = ensure_table(h, n_beams)) return rc;
  if (int rc = h->d_scans.reserve(sizeof(float) * 2 * (size_t)n_beams)) return rc;
  TBNAV_HIP(hipMemcpyAsync(h->d_scans.ptr, target_scan, sizeof(float) * (size_t)n_beams, hipMemcpyHostToDevice, h->stream));
  TBNAV_HIP(hipMemcpyAsync(h->d_scans.as<float>() + n_beams, source_scan, sizeof(float) * (size_t)n_beams, hipMemcpyHostToDevice, h->stream));
  clear_pairs(h);
  add_pair(h, 0, 1, T_init);
  h->last_launches = 0;
  if (int rc = run_pairs(h, 1, n_beams)) return rc;
  h->search.last = h->h_sinfo[0];
  h->search.last_shape = h->h_sshape[0];
  h->search.last_wide = h->h_swide[0];
  result(h->h_out[0], T_out, info);
  return TBNAV_OK;
}

int tbnav_icp_step(tbnav_icp* h, const float* scan, int32_t n_beams, const double T_init[3], double T_out[3], int32_t* ok,
                   tbnav_icp_info* info) {
  if (!h || !scan || !T_init || !T_out || !ok || !beams_ok(h, n_beams)) return TBNAV_ERR_INVALID_ARG;
  if (h->have_stored && n_beams != h->stored_beams) return TBNAV_ERR_INVALID_ARG;
  DeviceGuard guard(h->device);
  if (!guard.ok) return TBNAV_ERR_NO_DEVICE;
  if (!h->have_stored) {  // cloud_alignment.cpp:64-68
    if (int rc = store_scan(h, nullptr, scan, n_beams)) return rc;
    first_call(T_out, ok, info);
    h->search.last = tbnav_icp_search_info{};
    h->search.last_shape = tbnav_icp_search_shape{};
    h->search.last_wide = tbnav_icp_search_wide_info{};
    return TBNAV_OK;
  }
  if (int rc = ensure_table(h, n_beams)) return rc;
  if (int rc = h->d_scans.reserve(sizeof(float) * (size_t)n_beams)) return rc;
  TBNAV_HIP(hipMemcpyAsync(h->d_scans.ptr, scan, sizeof(float) * (size_t)n_beams, hipMemcpyHostToDevice, h->stream));
  clear_pairs(h);
  add_pair(h, -1, 0, T_init);
  h->last_launches = 0;
  if (int rc = run_pairs(h, 1, n_beams)) return rc;
  h->search.last = h->h_sinfo[0];
  h->search.last_shape = h->h_sshape[0];
  h->search.last_wide = h->h_swide[0];
  const IcpOut o = h->h_out[0];
  result(o, T_out, info);
  *ok = converged(o.criterion) ? 1 : 0;
  if (*ok) return store_scan(h, h->d_scans.as<float>(), nullptr, n_beams);  // :59 — a failure keeps the old scan (:53-56)
  return TBNAV_OK;
}

int tbnav_icp_step_batch(tbnav_icp* h, const float* scans, int32_t n_beams, int32_t n_scans, const double* T_init, int32_t* ok,
                         double* T_out, tbnav_icp_info* info) {
  if (!h || !scans || !T_init || !ok || !T_out || !beams_ok(h, n_beams) || n_scans <= 0)
    return TBNAV_ERR_INVALID_ARG;
  if (h->have_stored && n_beams != h->stored_beams) return TBNAV_ERR_INVALID_ARG;
  DeviceGuard guard(h->device);
  if (!guard.ok) return TBNAV_ERR_NO_DEVICE;
  if (int rc = ensure_table(h, n_beams)) return rc;
  if (int rc = h->d_scans.reserve(sizeof(float) * (size_t)n_beams * (size_t)n_scans)) return rc;
  TBNAV_HIP(hipMemcpyAsync(h->d_scans.ptr, scans, sizeof(float) * (size_t)n_beams * (size_t)n_scans, hipMemcpyHostToDevice, h->stream));
  h->last_launches = 0;
  int s = 0;
  int target = -1;  // -1: the stored scan
  if (!h->have_stored) {
    first_call(T_out, ok, info);
    target = 0;
    s = 1;
  }
  // launch 1: every scan against its predecessor (the stored scan for the first), speculatively.  Then walk in order: the
  // result for (actual target, scan) is taken from what has been aligned so far; when it is missing (a scan before
  // failed, so the target stayed an earlier scan), the scans from there are aligned against the actual target in another
  // launch — through the first one whose speculative alignment converged (the scans before it will probably fail against
  // any target, and the walk would need each of them next).
  struct Done { IcpOut out; tbnav_icp_search_info search; tbnav_icp_search_shape shape; tbnav_icp_search_wide_info wide; };
  std::map<std::pair<int, int>, Done> done;  // (target, source) -> result, and the search in front of it
  h->search.last = tbnav_icp_search_info{};
  h->search.last_shape = tbnav_icp_search_shape{};
  h->search.last_wide = tbnav_icp_search_wide_info{};
  if (s < n_scans) {
    clear_pairs(h);
    for (int q = s; q < n_scans; ++q) add_pair(h, q - 1, q, T_init + 3 * (size_t)q);
    if (int rc = run_pairs(h, (int)h->h_pairs.size(), n_beams)) return rc;
    for (size_t j = 0; j < h->h_pairs.size(); ++j) done[{h->h_pairs[j].tgt, h->h_pairs[j].src}] = Done{h->h_out[j], h->h_sinfo[j], h->h_sshape[j], h->h_swide[j]};
  }
  for (; s < n_scans; ++s) {
    auto it = done.find({target, s});
    if (it == done.end()) {
      clear_pairs(h);
      for (int q = s; q < n_scans; ++q) {
        add_pair(h, target, q, T_init + 3 * (size_t)q);
        const auto spec = done.find({q - 1, q});
        if (spec != done.end() && converged(spec->second.out.criterion)) break;
      }
      if (int rc = run_pairs(h, (int)h->h_pairs.size(), n_beams)) return rc;
      for (size_t j = 0; j < h->h_pairs.size(); ++j) done[{h->h_pairs[j].tgt, h->h_pairs[j].src}] = Done{h->h_out[j], h->h_sinfo[j], h->h_sshape[j], h->h_swide[j]};
      it = done.find({target, s});
    }
    const IcpOut& o = it->second.out;
    h->search.last = it->second.search;
    h->search.last_shape = it->second.shape;
    h->search.last_wide = it->second.wide;
    result(o, T_out + 3 * (size_t)s, info ? info + s : nullptr);
    ok[s] = converged(o.criterion) ? 1 : 0;
    if (ok[s]) target = s;
  }
  if (target >= 0) return store_scan(h, h->d_scans.as<float>() + (size_t)target * n_beams, nullptr, n_beams);
  return TBNAV_OK;
}

}  // extern "C"

/* tbnav_icp.h — point-to-point ICP between two laser scans on the GPU: the scan matcher that the reference's
 * bmapping::ScanAlignment::pclICPWrapper (bmapping/src/bmapping/cloud_alignment.cpp:37-223) runs once per scan through
 * pcl::IterativeClosestPoint<PointXYZ, PointXYZ>.  PCL is a third-party library that is not part of this project, so
 * what is implemented here is a RESTATEMENT of PCL 1.8's algorithm with the reference's settings (max_iter 100,
 * max_correspondence_dist 0.5, transformation_epsilon 1e-8, euclidean_fitness_epsilon 1e-6; cloud_alignment.cpp:21-34,
 * 186-190).  Its arithmetic is fixed below tightly enough that a numpy restatement (tests/icp_restatement.py) reproduces
 * the kernel bit for bit.  Parity with PCL itself is UNPINNED: no PCL build has been compared against it.
 *
 * CONTRACT
 *  1. Cloud (createPointCloud, cloud_alignment.cpp:76-157).  float beam_angle starts at beam_min; beam i is kept when
 *     r >= range_min && r < range_max (float compares: NaN and inf fall out); its point is (double)r * (double)cosf(angle),
 *     (double)r * (double)sinf(angle), mapped by Trs as rigid2d::Transform2D::operator() does ((c*x - s*y) + tx,
 *     (s*x + c*y) + ty in fp64, c = cos(Trs theta), s = sin(Trs theta)) and rounded to float; then beam_angle +=
 *     beam_delta (float) and the wrap of :140-154 (beam_max < 0: angle <= beam_max -> beam_min; else angle >= beam_max ->
 *     beam_min).  The cosf/sinf table is built on the host with glibc once per beam count; the points on the device.
 *  2. Initial guess (pclICP, :171-183): R = [[c, -s], [s, c]], t = (x, y) with c = float(cos theta), s = float(sin theta),
 *     x = float(x), y = float(y) of T_init, held in fp64 from then on.
 *  3. Iteration k = 1, 2, ...:
 *     - every source point a0 goes to a = float(((R00*a0x) + (R01*a0y)) + tx), likewise y with R10, R11, ty (fp64, no
 *       contraction);
 *     - its nearest target point b: the fp32 d = dx*dx + dy*dy, targets scanned in beam order with a strict '<' (the lowest
 *       index wins a tie); the pair is kept when (double)d <= max_corr_dist * max_corr_dist (PCL drops d > max^2);
 *     - fewer than 3 pairs: FAILED (TBNAV_ICP_NO_CORRESPONDENCES);
 *     - fp64 sums n, Sax, Say, Sbx, Sby, Sax*bx, Say*by, Sax*by, Say*bx, Sd in this FIXED order: thread t of B = 256 adds the
 *       kept pairs of the source beams i = t, t + B, t + 2B, ... in increasing i (i is the BEAM index, invalid beams add
 *       nothing), then a tree adds t and t + s for s = B/2, ..., 1;
 *     - A = (Sax*bx + Say*by) - ((Sax*Sbx) + (Say*Sby)) / n,  S = (Sax*by - Say*bx) - ((Sax*Sby) - (Say*Sbx)) / n,
 *       r = sqrt((A*A) + (S*S)); r == 0: FAILED (TBNAV_ICP_DEGENERATE); else c = A/r, s = S/r,
 *       t_inc = b_mean - R_inc * a_mean (means = sums / n);
 *     - R <- R_inc * R, t <- R_inc * t + t_inc.  No transcendental inside the loop: in exact arithmetic this is the 2-D
 *       solution PCL's Umeyama SVD finds for points of constant z.
 *  4. Stopping, checked after the update in PCL's DefaultConvergenceCriteria order:
 *     k >= max_iter -> TBNAV_ICP_ITERATIONS (PCL counts this as converged);
 *     c >= 1 - transform_eps && |t_inc|^2 <= transform_eps -> TBNAV_ICP_TRANSFORM;
 *     mse = Sd / n of this iteration: |mse - prev| < 1e-12 -> TBNAV_ICP_ABS_MSE; |mse - prev| / prev < fitness_eps ->
 *     TBNAV_ICP_REL_MSE; otherwise prev = mse (prev starts at DBL_MAX).
 *  5. Result (host): theta = atan2(R10, R00), x = t0, y = t1.  On a failure T_out is (0, 0, 0).
 *
 * KNOWN DIVERGENCES FROM PCL
 *  - PCL applies each increment to the float cloud in place and evaluates its criteria in float; here the source points
 *    are transformed from the original cloud by the accumulated fp64 transform.
 *  - PCL's kd-tree breaks distance ties in its own order.
 *  - PCL solves a 3x3 float Jacobi SVD (Umeyama); here the closed 2-D form above in fp64.
 *  - PCL's behaviour when the cross-covariance vanishes (r == 0) is not restated.
 *  - The RANSAC threshold cloud_alignment.cpp:190 sets is taken to have no effect on an IterativeClosestPoint with no
 *    correspondence rejector installed (an assumption: PCL's text is not part of this project).
 *  - The reference's result is read from a float matrix; here from the fp64 state.
 *
 * KERNEL: one workgroup of 256 threads per pair, the whole iteration loop in one launch; target cloud as float2 in LDS,
 * source points in registers, no global traffic inside the loop (csrc/icp.hip).  Limits: n_beams <= 4096 (32 KB of LDS),
 * max_iter <= 1000; anything larger is TBNAV_ERR_INVALID_ARG.
 */
#ifndef TBNAV_ICP_H
#define TBNAV_ICP_H

#include <stdint.h>

#include "tbnav_status.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TBNAV_ICP_MAX_BEAMS 4096
#define TBNAV_ICP_MAX_ITER 1000

typedef struct tbnav_icp_params {
  float beam_min, beam_max, beam_delta, range_min, range_max;  /* LaserProperties (sensor_model.hpp) */
  int32_t max_iter;                                              /* 100 in the reference */
  double Trs[3];                                                 /* robot <- laser: theta, x, y */
  double max_corr_dist;                                          /* 0.5 */
  double transform_eps;                                          /* 1e-8 */
  double fitness_eps;                                            /* 1e-6 */
  int32_t device;                                                /* -1: the current device */
  int32_t reserved;
} tbnav_icp_params;

/* why an alignment stopped; ITERATIONS, TRANSFORM, ABS_MSE and REL_MSE are converged (PCL's hasConverged()) */
typedef enum tbnav_icp_criterion {
  TBNAV_ICP_NOT_RUN = 0,             /* tbnav_icp_step's first call: the scan was stored, T = identity, ok = 1 */
  TBNAV_ICP_ITERATIONS = 1,
  TBNAV_ICP_TRANSFORM = 2,
  TBNAV_ICP_ABS_MSE = 3,
  TBNAV_ICP_REL_MSE = 4,
  TBNAV_ICP_NO_CORRESPONDENCES = 5,  /* failed: fewer than 3 pairs within max_corr_dist */
  TBNAV_ICP_DEGENERATE = 6           /* failed: r == 0 */
} tbnav_icp_criterion;

typedef struct tbnav_icp_info {
  int32_t iterations;       /* iterations run (the failing one included) */
  int32_t correspondences;  /* pairs kept in the last iteration */
  double mse;               /* Sd / n of the last iteration (0 when it had fewer than 3 pairs) */
  int32_t criterion;        /* tbnav_icp_criterion */
  int32_t reserved;
} tbnav_icp_info;

typedef struct tbnav_icp tbnav_icp;

/* The defaults above are the reference's (cloud_alignment.cpp:21-34): callers set the laser fields and Trs. */
void tbnav_icp_default_params(tbnav_icp_params* p);
int tbnav_icp_create(const tbnav_icp_params* params, tbnav_icp** out);
void tbnav_icp_destroy(tbnav_icp* h);
/* forget the stored scan: the next tbnav_icp_step is a first call again */
int tbnav_icp_reset(tbnav_icp* h);

/* pclICP (cloud_alignment.cpp:160-223), stateless: clouds of target_scan and source_scan (n_beams ranges each) aligned
 * from T_init = (theta, x, y).  info is required (info->criterion says whether it converged). */
int tbnav_icp_match(tbnav_icp* h, const float* target_scan, const float* source_scan, int32_t n_beams, const double T_init[3],
                    double T_out[3], tbnav_icp_info* info);

/* pclICPWrapper (cloud_alignment.cpp:37-72) with the stored scan in the handle: the first call stores the scan and returns
 * ok = 1, T = identity; a converged match replaces the stored scan; a failed one keeps it (ok = 0).  n_beams must equal the
 * stored scan's.  info is optional.  (The "ICP FAILED TO CONVERGED!" line is printed by the C++ shim, not here.) */
int tbnav_icp_step(tbnav_icp* h, const float* scan, int32_t n_beams, const double T_init[3], double T_out[3], int32_t* ok,
                   tbnav_icp_info* info);

/* n_scans successive tbnav_icp_step calls, bit for bit: scans [n_scans][n_beams], T_init [n_scans][3]; ok [n_scans],
 * T_out [n_scans][3] (exactly tbnav_rbpf_slam_batch's icp_ok / T_icp), info [n_scans] optional.  Every consecutive pair is
 * aligned speculatively in one launch; the results are then walked in order, and the pairs whose target changed because
 * a scan before them failed (the target stays the last converged scan) are aligned again in further launches. */
int tbnav_icp_step_batch(tbnav_icp* h, const float* scans, int32_t n_beams, int32_t n_scans, const double* T_init,
                         int32_t* ok, double* T_out, tbnav_icp_info* info);

/* test hook: the cloud the kernel builds from one scan (contract item 1), compacted in beam order: xy [n_beams][2],
 * *n_points valid points. */
int tbnav_icp_cloud(tbnav_icp* h, const float* scan, int32_t n_beams, float* xy, int32_t* n_points);

/* number of kernel launches the last tbnav_icp_step_batch made (1 when no scan failed) */
int tbnav_icp_last_batch_launches(const tbnav_icp* h);

#ifdef __cplusplus
}
#endif
#endif /* TBNAV_ICP_H */

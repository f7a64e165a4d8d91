// icp_test_hooks.cpp — extern "C" access for tests/: bmapping::ScanAlignment with useDeviceICP() driving a
// bmapping::ParticleFilter the way turtle_mapping_node.cpp does (:400-410, :474), the same conventions as test_hooks.cpp.
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "bmapping/cloud_alignment.hpp"
#include "bmapping/grid_mapper.hpp"
#include "bmapping/particle_filter.hpp"
#include "rigid2d/rigid2d.hpp"

using rigid2d::Transform2D;
using rigid2d::Twist2D;
using rigid2d::Vector2D;

namespace {

thread_local std::string g_icp_err;

const double kD2R = rigid2d::PI / 180.0;

bmapping::LaserProperties hook_laser() {
  return bmapping::LaserProperties((float)(0.0 * kD2R), (float)(360.0 * kD2R), (float)(1.0 * kD2R), 0.12f, 3.5f, 0.95, 0.0, 0.04, 0.01, 0.5);
}

bmapping::ICPMetric hook_metric(int metric, const char* who) {
  if (metric != 0 && metric != 1) throw std::invalid_argument(std::string(who) + ": metric must be 0 or 1");
  return metric == 1 ? bmapping::ICPMetric::PointToLine : bmapping::ICPMetric::PointToPoint;
}

// The shipped filter (slam.launch; as hst_pf_run) around aligner, which the caller has put on the device (useDeviceICP):
// ParticleFilter copies it and the copy shares the device handle.  n_scans of SLAM() on scans [n_scans][n_beams],
// odom [n_scans + 1][3] (theta, x, y; odom[s] = prev, odom[s + 1] = cur), u [n_scans][3] (w, vx, vy).  What the filter's copy
// of the matcher returns is observed through a second copy of the same aligner, fed what SLAM feeds its own (icpInitGuess,
// particle_filter.cpp:602-612): out_ok [n_scans], out_T [n_scans][3] (theta, x, y).  out_pose [n_scans][3] = getRobotState,
// out_neff [n_scans].
void run_filter(bmapping::ScanAlignment& aligner, int N, int k, double map_half, uint64_t seed, const float* scans, int n_beams,
                int n_scans, const double* odom, const double* u, int32_t* out_ok, double* out_T, double* out_pose, int32_t* out_neff) {
  Transform2D Trs;
  bmapping::GridMapper grid(0.05, -map_half, map_half, -map_half, map_half, hook_laser(), Trs);
  bmapping::ScanAlignment observer = aligner;  // shares the handle; keeps its own stored scan
  Transform2D start(Vector2D(odom[1], odom[2]), odom[0]);
  bmapping::ParticleFilter pf(N, k, 0.1, 0.2, 0.1, 0.2, 1e-10, 1e-10, 1e-10, 1e-10, 1e-8, 1e-8, 1.0, 20.0, 1.0, 10.0, aligner, start, grid);
  bmapping::getTwister().seed(seed);
  for (int s = 0; s < n_scans; ++s) {
    std::vector<float> scan(scans + (size_t)s * n_beams, scans + (size_t)(s + 1) * n_beams);
    rigid2d::Pose prev, cur;
    prev.theta = odom[3 * s]; prev.x = odom[3 * s + 1]; prev.y = odom[3 * s + 2];
    cur.theta = odom[3 * (s + 1)]; cur.x = odom[3 * (s + 1) + 1]; cur.y = odom[3 * (s + 1) + 2];
    Twist2D tw; tw.w = u[3 * s]; tw.vx = u[3 * s + 1]; tw.vy = u[3 * s + 2];
    const double dth = rigid2d::normalize_angle_PI(rigid2d::normalize_angle_PI(cur.theta) - rigid2d::normalize_angle_PI(prev.theta));
    const Transform2D Tinit(Vector2D(cur.x - prev.x, cur.y - prev.y), dth);
    Transform2D T;
    out_ok[s] = observer.pclICPWrapper(T, Tinit, scan) ? 1 : 0;
    const auto d = T.displacement();
    out_T[3 * s] = d.theta; out_T[3 * s + 1] = d.x; out_T[3 * s + 2] = d.y;
    pf.SLAM(scan, tw, cur, prev);
    const auto p = pf.getRobotState().displacement();
    out_pose[3 * s] = p.theta; out_pose[3 * s + 1] = p.x; out_pose[3 * s + 2] = p.y;
    out_neff[s] = pf.effectiveParticles();
  }
}

}  // namespace

extern "C" {

const char* hst_icp_last_error() { return g_icp_err.c_str(); }

// The hst_icp_pf_run* put a ScanAlignment(props, Trs) on the device their own way and hand it to run_filter (whose
// comment has the arguments).  Each returns 0, or -1 (message in hst_icp_last_error).
// hst_icp_pf_run: the point metric, no search.  hst_icp_pf_run_metric: the metric named (0: point-to-point, 1: point-to-line).
// hst_icp_pf_run_search: the same with the correlative search in front of the ICP (search != 0; lin_cells as given, all else
// the defaults).
int hst_icp_pf_run_search(int metric, int search, int lin_cells, int N, int k, double map_half, uint64_t seed, const float* scans, int n_beams, int n_scans,
                          const double* odom, const double* u, int32_t* out_ok, double* out_T, double* out_pose, int32_t* out_neff) {
  try {
    const bmapping::ICPMetric m = hook_metric(metric, "hst_icp_pf_run_search");
    bmapping::ScanAlignment aligner(hook_laser(), Transform2D());
    if (search) {
      bmapping::ICPSearch sp;
      sp.lin_cells = lin_cells;
      aligner.useDeviceICP(-1, m, sp);
    } else if (metric == 1) aligner.useDeviceICP(-1, m);
    else aligner.useDeviceICP();
    run_filter(aligner, N, k, map_half, seed, scans, n_beams, n_scans, odom, u, out_ok, out_T, out_pose, out_neff);
    return 0;
  } catch (const std::exception& e) { g_icp_err = e.what(); return -1; }
}

// hst_icp_pf_run_search_shape: the filter with the search (lin_cells as given, all else the defaults) and, shape != 0, the shape
// of its score volume (drop_q10 and flat_cells2 as given) in front of the ICP; everything else as hst_icp_pf_run_search.
int hst_icp_pf_run_search_shape(int metric, int shape, int drop_q10, double flat_cells2, int lin_cells, int N, int k, double map_half, uint64_t seed,
                                const float* scans, int n_beams, int n_scans, const double* odom, const double* u, int32_t* out_ok, double* out_T,
                                double* out_pose, int32_t* out_neff) {
  try {
    const bmapping::ICPMetric m = hook_metric(metric, "hst_icp_pf_run_search_shape");
    bmapping::ScanAlignment aligner(hook_laser(), Transform2D());
    bmapping::ICPSearch sp;
    sp.lin_cells = lin_cells;
    sp.shape = shape != 0;
    sp.shape_drop_q10 = drop_q10;
    sp.shape_flat_cells2 = flat_cells2;
    aligner.useDeviceICP(-1, m, sp);
    run_filter(aligner, N, k, map_half, seed, scans, n_beams, n_scans, odom, u, out_ok, out_T, out_pose, out_neff);
    return 0;
  } catch (const std::exception& e) { g_icp_err = e.what(); return -1; }
}

// hst_icp_pf_run_search_wide: the filter with the search (its defaults) and, wide != 0, its wide second stage (wide_lin_cells,
// wide_ang_steps and when as given) in front of the ICP; everything else as hst_icp_pf_run_search.
int hst_icp_pf_run_search_wide(int metric, int wide, int wide_lin_cells, int wide_ang_steps, int when, int N, int k, double map_half, uint64_t seed,
                               const float* scans, int n_beams, int n_scans, const double* odom, const double* u, int32_t* out_ok, double* out_T,
                               double* out_pose, int32_t* out_neff) {
  try {
    const bmapping::ICPMetric m = hook_metric(metric, "hst_icp_pf_run_search_wide");
    bmapping::ScanAlignment aligner(hook_laser(), Transform2D());
    bmapping::ICPSearch sp;
    sp.wide = wide != 0;
    sp.wide_lin_cells = wide_lin_cells;
    sp.wide_ang_steps = wide_ang_steps;
    sp.wide_when = static_cast<bmapping::ICPWideWhen>(when);
    aligner.useDeviceICP(-1, m, sp);
    run_filter(aligner, N, k, map_half, seed, scans, n_beams, n_scans, odom, u, out_ok, out_T, out_pose, out_neff);
    return 0;
  } catch (const std::exception& e) { g_icp_err = e.what(); return -1; }
}

int hst_icp_pf_run_metric(int metric, int N, int k, double map_half, uint64_t seed, const float* scans, int n_beams, int n_scans,
                          const double* odom, const double* u, int32_t* out_ok, double* out_T, double* out_pose, int32_t* out_neff) {
  return hst_icp_pf_run_search(metric, 0, 0, N, k, map_half, seed, scans, n_beams, n_scans, odom, u, out_ok, out_T, out_pose, out_neff);
}

int hst_icp_pf_run(int N, int k, double map_half, uint64_t seed, const float* scans, int n_beams, int n_scans, const double* odom,
                   const double* u, int32_t* out_ok, double* out_T, double* out_pose, int32_t* out_neff) {
  return hst_icp_pf_run_metric(0, N, k, map_half, seed, scans, n_beams, n_scans, odom, u, out_ok, out_T, out_pose, out_neff);
}

}  // extern "C"

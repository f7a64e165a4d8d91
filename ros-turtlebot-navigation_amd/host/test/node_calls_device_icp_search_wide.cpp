// node_calls_device_icp_search_wide.cpp — COMPILE-ONLY: turtle_mapping_node.cpp's construction of the scan matcher and the filter
// (:389-410), compiled with -DTBNAV_SCAN_ALIGNMENT_DEVICE_ICP -DTBNAV_SCAN_ALIGNMENT_SEARCH -DTBNAV_SCAN_ALIGNMENT_SEARCH_WIDE
// (host/Makefile).  With the three defines the unchanged node's ScanAlignment aligns every scan with the device ICP, the
// correlative search in front of it and the search's wide second stage behind a rejected first stage (include/tbnav_icp.h, items
// W1-W8; additions, the reference has none of them).  The second function names the new ICPSearch members as a node that sets
// them itself would.  Nothing here runs.
#if !defined(TBNAV_SCAN_ALIGNMENT_DEVICE_ICP) || !defined(TBNAV_SCAN_ALIGNMENT_SEARCH) || !defined(TBNAV_SCAN_ALIGNMENT_SEARCH_WIDE)
#error "built with -DTBNAV_SCAN_ALIGNMENT_DEVICE_ICP -DTBNAV_SCAN_ALIGNMENT_SEARCH -DTBNAV_SCAN_ALIGNMENT_SEARCH_WIDE"
#endif
#include <cstdint>
#include <vector>

#include "bmapping/cloud_alignment.hpp"
#include "bmapping/grid_mapper.hpp"
#include "bmapping/particle_filter.hpp"
#include "bmapping/sensor_model.hpp"
#include "rigid2d/rigid2d.hpp"

using bmapping::GridMapper;
using bmapping::LaserProperties;
using bmapping::ParticleFilter;
using bmapping::ScanAlignment;
using rigid2d::Transform2D;

// what the constructor's default arguments are in this translation unit
static_assert(TBNAV_SCAN_ALIGNMENT_DEVICE_ICP_DEFAULT, "the device ICP is the default here");
static_assert(TBNAV_SCAN_ALIGNMENT_METRIC_DEFAULT == bmapping::ICPMetric::PointToPoint, "the point metric stays the default here");
static_assert(TBNAV_SCAN_ALIGNMENT_SEARCH_DEFAULT, "the search is on by default here");
static_assert(!TBNAV_SCAN_ALIGNMENT_SEARCH_SHAPE_DEFAULT, "the shape is not");
static_assert(TBNAV_SCAN_ALIGNMENT_SEARCH_WIDE_DEFAULT, "and the wide second stage is");

void turtle_mapping_node_calls_with_device_icp_search_wide() {
  float beam_min = 0, beam_max = 6.28f, beam_delta = 0.0174f, range_min = 0.12f, range_max = 3.5f;
  double z_hit = 0.95, z_short = 0.0, z_max = 0.04, z_rand = 0.01, sigma_hit = 0.5;
  Transform2D Trs, robot_pose;
  LaserProperties props(beam_min, beam_max, beam_delta, range_min, range_max, z_hit, z_short, z_max, z_rand, sigma_hit);
  GridMapper grid(0.05, -2.0, 2.0, -2.0, 2.0, props, Trs);
  ScanAlignment aligner(props, Trs);  // :400 — the search and its wide second stage, by the three defines
  ParticleFilter pf(40, 50, 0.1, 0.2, 0.1, 0.2, 1e-10, 1e-10, 1e-10, 1e-10, 1e-8, 1e-8, 1, 20, 1, 10, aligner, robot_pose, grid);
  Transform2D T;
  aligner.pclICPWrapper(T, Transform2D(), std::vector<float>(360, 1.0f));
}

void a_node_that_sets_the_wide_members_itself() {
  LaserProperties props(0, 6.28f, 0.0174f, 0.12f, 3.5f, 0.95, 0.0, 0.04, 0.01, 0.5);
  ScanAlignment aligner(props, Transform2D(), false);
  bmapping::ICPSearch s;
  static_assert(sizeof(s.wide) == sizeof(bool), "wide is a flag");
  s.wide = true;
  s.wide_lin_cells = 64;
  s.wide_ang_steps = 90;
  s.wide_when = bmapping::ICPWideWhen::OnRejectOrEdge;
  aligner.useDeviceICP(-1, bmapping::ICPMetric::PointToLine, s);
}

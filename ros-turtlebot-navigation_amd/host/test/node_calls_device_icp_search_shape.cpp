// node_calls_device_icp_search_shape.cpp — COMPILE-ONLY: turtle_mapping_node.cpp's construction of the scan matcher and the filter
// (:389-410), compiled with -DTBNAV_SCAN_ALIGNMENT_DEVICE_ICP -DTBNAV_SCAN_ALIGNMENT_POINT_TO_LINE
// -DTBNAV_SCAN_ALIGNMENT_SEARCH -DTBNAV_SCAN_ALIGNMENT_SEARCH_SHAPE (host/Makefile).  With the four defines the unchanged node's
// ScanAlignment aligns every scan with the device ICP's point-to-line metric, the correlative search in front of it and the
// shape of the search's score volume keeping the guess along a corridor (include/tbnav_icp.h; all three are additions, the
// reference has none of them).  Nothing here runs.
#if !defined(TBNAV_SCAN_ALIGNMENT_DEVICE_ICP) || !defined(TBNAV_SCAN_ALIGNMENT_POINT_TO_LINE) || !defined(TBNAV_SCAN_ALIGNMENT_SEARCH) || \
    !defined(TBNAV_SCAN_ALIGNMENT_SEARCH_SHAPE)
#error "built with -DTBNAV_SCAN_ALIGNMENT_DEVICE_ICP -DTBNAV_SCAN_ALIGNMENT_POINT_TO_LINE -DTBNAV_SCAN_ALIGNMENT_SEARCH -DTBNAV_SCAN_ALIGNMENT_SEARCH_SHAPE"
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
static_assert(TBNAV_SCAN_ALIGNMENT_METRIC_DEFAULT == bmapping::ICPMetric::PointToLine, "the line metric is the default here");
static_assert(TBNAV_SCAN_ALIGNMENT_SEARCH_DEFAULT, "the search is on by default here");
static_assert(TBNAV_SCAN_ALIGNMENT_SEARCH_SHAPE_DEFAULT, "and so is the shape of its score volume");

void turtle_mapping_node_calls_with_device_icp_search_shape() {
  float beam_min = 0, beam_max = 6.28f, beam_delta = 0.0174f, range_min = 0.12f, range_max = 3.5f;
  double z_hit = 0.95, z_short = 0.0, z_max = 0.04, z_rand = 0.01, sigma_hit = 0.5;
  Transform2D Trs, robot_pose;
  LaserProperties props(beam_min, beam_max, beam_delta, range_min, range_max, z_hit, z_short, z_max, z_rand, sigma_hit);
  GridMapper grid(0.05, -2.0, 2.0, -2.0, 2.0, props, Trs);
  ScanAlignment aligner(props, Trs);  // :400 — the line metric, the search and its shape, by the four defines
  ParticleFilter pf(40, 50, 0.1, 0.2, 0.1, 0.2, 1e-10, 1e-10, 1e-10, 1e-10, 1e-8, 1e-8, 1, 20, 1, 10, aligner, robot_pose, grid);
  Transform2D T;
  aligner.pclICPWrapper(T, Transform2D(), std::vector<float>(360, 1.0f));
}

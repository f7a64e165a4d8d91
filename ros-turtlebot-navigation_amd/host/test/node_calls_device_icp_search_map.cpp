// node_calls_device_icp_search_map.cpp — COMPILE-ONLY: a mapping node that relocalises against its own map.  It builds the scan
// matcher and the filter as turtle_mapping_node.cpp does (:389-410), with -DTBNAV_SCAN_ALIGNMENT_DEVICE_ICP
// -DTBNAV_SCAN_ALIGNMENT_SEARCH (host/Makefile), and calls ScanAlignment::searchMap (include/tbnav_icp.h, MAP SEARCH M1-M9; an
// addition, the reference has nothing like it) with a guess in the world, reading every member of its result.  Nothing here runs.
#if !defined(TBNAV_SCAN_ALIGNMENT_DEVICE_ICP) || !defined(TBNAV_SCAN_ALIGNMENT_SEARCH)
#error "built with -DTBNAV_SCAN_ALIGNMENT_DEVICE_ICP -DTBNAV_SCAN_ALIGNMENT_SEARCH"
#endif
#include <type_traits>
#include <vector>

#include "bmapping/cloud_alignment.hpp"
#include "bmapping/grid_mapper.hpp"
#include "bmapping/particle_filter.hpp"
#include "bmapping/sensor_model.hpp"
#include "rigid2d/rigid2d.hpp"

using bmapping::GridMapper;
using bmapping::LaserProperties;
using bmapping::MapSearchResult;
using bmapping::ParticleFilter;
using bmapping::ScanAlignment;
using rigid2d::Transform2D;

static_assert(std::is_same<decltype(MapSearchResult::T), Transform2D>::value, "T is a pose in the world");
static_assert(std::is_same<decltype(MapSearchResult::quality), double>::value, "quality is a double");
static_assert(std::is_same<decltype(MapSearchResult::accepted), bool>::value && std::is_same<decltype(MapSearchResult::at_edge), bool>::value,
              "accepted and at_edge are flags");

bool a_node_that_relocalises_against_its_map(const std::vector<float>& scan, const Transform2D& lost_guess, Transform2D& found) {
  LaserProperties props(0, 6.28f, 0.0174f, 0.12f, 3.5f, 0.95, 0.0, 0.04, 0.01, 0.5);
  Transform2D Trs, robot_pose;
  GridMapper grid(0.05, -10.0, 10.0, -10.0, 10.0, props, Trs);
  ScanAlignment aligner(props, Trs);   // the device ICP and its search with the default parameters, by the two defines
  ParticleFilter pf(40, 50, 0.1, 0.2, 0.1, 0.2, 1e-10, 1e-10, 1e-10, 1e-10, 1e-8, 1e-8, 1, 20, 1, 10, aligner, robot_pose, grid);
  const MapSearchResult r = aligner.searchMap(pf, lost_guess, scan);
  if (r.accepted && !r.at_edge && r.quality > 0.7) found = r.T;
  return r.accepted;
}

MapSearchResult a_node_that_searches_wide(ParticleFilter& pf, const std::vector<float>& scan, const Transform2D& guess) {
  LaserProperties props(0, 6.28f, 0.0174f, 0.12f, 3.5f, 0.95, 0.0, 0.04, 0.01, 0.5);
  ScanAlignment aligner(props, Transform2D(), false);
  bmapping::ICPSearch s;
  s.min_quality = 0.7;   // over a wide window against a map the default 0.5 does not separate a wrong room (tbnav_icp.h M9)
  s.wide = true;
  s.wide_when = bmapping::ICPWideWhen::OnRejectOrEdge;
  aligner.useDeviceICP(-1, bmapping::ICPMetric::PointToPoint, s);
  return aligner.searchMap(pf, guess, scan);
}

// node_calls_device_icp_align_map.cpp — COMPILE-ONLY: a mapping node that is put down in a map it already holds and wants its pose
// below one cell.  It builds the scan matcher and the filter as turtle_mapping_node.cpp does (:389-410), with
// -DTBNAV_SCAN_ALIGNMENT_DEVICE_ICP -DTBNAV_SCAN_ALIGNMENT_SEARCH (host/Makefile), calls ScanAlignment::relocalizeInMap and
// ScanAlignment::alignToMap (include/tbnav_icp.h, MAP ALIGNMENT A1-A11; additions, the reference has nothing like them) and reads
// every member of their results.  Nothing here runs.
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
using bmapping::ICPAlignMap;
using bmapping::ICPGlobal;
using bmapping::LaserProperties;
using bmapping::MapAlignResult;
using bmapping::MapRelocalizeResult;
using bmapping::ParticleFilter;
using bmapping::ScanAlignment;
using rigid2d::Transform2D;

static_assert(std::is_same<decltype(MapAlignResult::T), Transform2D>::value, "T is a pose in the world");
static_assert(std::is_same<decltype(MapAlignResult::ok), bool>::value, "ok is a flag");
static_assert(std::is_same<decltype(MapAlignResult::mse), double>::value, "mse is a double");

bool a_node_that_wants_its_pose_below_one_cell(const std::vector<float>& scan, Transform2D& found) {
  LaserProperties props(0, 6.28f, 0.0174f, 0.12f, 3.5f, 0.95, 0.0, 0.04, 0.01, 0.5);
  Transform2D Trs, robot_pose;
  GridMapper grid(0.05, -10.0, 10.0, -10.0, 10.0, props, Trs);
  ScanAlignment aligner(props, Trs);   // the device ICP and its search with the default parameters, by the two defines
  ParticleFilter pf(40, 50, 0.1, 0.2, 0.1, 0.2, 1e-10, 1e-10, 1e-10, 1e-10, 1e-8, 1e-8, 1, 20, 1, 10, aligner, robot_pose, grid);
  const MapRelocalizeResult r = aligner.relocalizeInMap(pf, scan);   // the defaults of both
  if (!r.found.accepted || !r.aligned) return false;
  found = r.T;
  return r.fine.ok && r.fine.iterations >= 1 && r.fine.correspondences >= 3 && r.fine.criterion >= 1 && r.fine.mse >= 0.0;
}

MapAlignResult a_node_that_has_a_guess_good_to_a_cell(ParticleFilter& pf, ScanAlignment& aligner, const Transform2D& guess,
                                                      const std::vector<float>& scan) {
  ICPAlignMap p;
  p.half_cells = 96;
  p.gate_cells = 6;
  p.feature_cells = 3;
  p.max_flatness = 0.2;
  const MapAlignResult r = aligner.alignToMap(pf, guess, scan, p);
  return r.ok ? r : aligner.alignToMap(pf, guess, scan);   // a failure hands the guess back: try the defaults
}

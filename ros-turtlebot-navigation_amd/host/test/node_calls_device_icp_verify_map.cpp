// node_calls_device_icp_verify_map.cpp — COMPILE-ONLY: a mapping node that is put down in a map it already holds and wants to know
// whether that map contradicts the pose it found.  It builds the scan matcher and the filter as turtle_mapping_node.cpp does
// (:389-410), with -DTBNAV_SCAN_ALIGNMENT_DEVICE_ICP -DTBNAV_SCAN_ALIGNMENT_SEARCH (host/Makefile), calls
// ScanAlignment::relocalizeInMapChecked and ScanAlignment::verifyInMap (include/tbnav_icp.h, MAP CHECK V1-V10; additions, the reference
// has nothing like them) and reads every member of their results.  Nothing here runs.
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
using bmapping::ICPVerifyMap;
using bmapping::LaserProperties;
using bmapping::MapRelocalizeCheckedResult;
using bmapping::MapVerifyResult;
using bmapping::ParticleFilter;
using bmapping::ScanAlignment;
using rigid2d::Transform2D;

static_assert(std::is_same<decltype(MapVerifyResult::accepted), bool>::value, "accepted is a flag");
static_assert(std::is_same<decltype(MapVerifyResult::free_cells), long long>::value, "the path counts are 64-bit");
static_assert(std::is_same<decltype(MapRelocalizeCheckedResult::T), Transform2D>::value, "T is a pose in the world");

bool a_node_that_wants_a_pose_its_map_does_not_contradict(const std::vector<float>& scan, Transform2D& found) {
  LaserProperties props(0, 6.28f, 0.0174f, 0.12f, 3.5f, 0.95, 0.0, 0.04, 0.01, 0.5);
  Transform2D Trs, robot_pose;
  GridMapper grid(0.05, -10.0, 10.0, -10.0, 10.0, props, Trs);
  ScanAlignment aligner(props, Trs);   // the device ICP and its search with the default parameters, by the two defines
  ParticleFilter pf(40, 50, 0.1, 0.2, 0.1, 0.2, 1e-10, 1e-10, 1e-10, 1e-10, 1e-8, 1e-8, 1, 20, 1, 10, aligner, robot_pose, grid);
  MapRelocalizeCheckedResult r = aligner.relocalizeInMapChecked(pf, scan);   // the defaults of all three
  if (!r.verified)   // a true pose the search's quality threw away (a guess far off, a table that misses walls) may still pass the check
    r = aligner.relocalizeInMapChecked(pf, scan, ICPGlobal(), ICPAlignMap(), ICPVerifyMap(), true);
  if (!r.checked || !r.aligned) return false;
  found = r.T;
  const MapVerifyResult& c = r.check;
  const bool sums = c.hit + c.through + c.missing + c.unseen + c.undecided == c.walked && c.walked == c.points - c.outside;
  return r.verified && c.accepted && sums && r.found.quality >= 0.0 && r.fine.iterations >= 1 && c.free_cells >= 0 && c.unknown_cells >= 0 &&
         c.sensor_cell[0] >= 0 && c.sensor_cell[1] >= 0 && c.sensor_class != 2;
}

MapVerifyResult a_node_that_checks_a_pose_it_was_given(ParticleFilter& pf, ScanAlignment& aligner, const Transform2D& pose,
                                                       const std::vector<float>& scan) {
  ICPVerifyMap p;
  p.half_cells = 128;
  p.slack_cells = 3;
  p.max_through_q10 = 51;
  p.max_missing_q10 = 51;
  p.min_hit_q10 = 614;
  const MapVerifyResult r = aligner.verifyInMap(pf, pose, scan, p);
  return r.accepted ? r : aligner.verifyInMap(pf, pose, scan);   // the defaults
}

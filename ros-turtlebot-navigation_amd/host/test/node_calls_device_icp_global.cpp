// node_calls_device_icp_global.cpp — COMPILE-ONLY: a mapping node that is put down somewhere in a map it already holds.  It builds the
// scan matcher and the filter as turtle_mapping_node.cpp does (:389-410), with -DTBNAV_SCAN_ALIGNMENT_DEVICE_ICP
// -DTBNAV_SCAN_ALIGNMENT_SEARCH (host/Makefile), calls ScanAlignment::localizeInMap (include/tbnav_icp.h, GLOBAL SEARCH L1-L10; an
// addition, the reference has nothing like it) with no guess, reads every member of its result, and refines the pose it found with
// searchMap.  Nothing here runs.
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
using bmapping::ICPGlobal;
using bmapping::LaserProperties;
using bmapping::MapLocalizeResult;
using bmapping::MapSearchResult;
using bmapping::ParticleFilter;
using bmapping::ScanAlignment;
using rigid2d::Transform2D;

static_assert(std::is_same<decltype(MapLocalizeResult::T), Transform2D>::value, "T is a pose in the world");
static_assert(std::is_same<decltype(MapLocalizeResult::quality), double>::value, "quality is a double");
static_assert(std::is_same<decltype(MapLocalizeResult::accepted), bool>::value, "accepted is a flag");
static_assert(std::is_same<decltype(MapLocalizeResult::blocks), long long>::value &&
                  std::is_same<decltype(MapLocalizeResult::refined_blocks), long long>::value,
              "the block counts are 64-bit");

bool a_node_that_is_put_down_in_its_map(const std::vector<float>& scan, Transform2D& found) {
  LaserProperties props(0, 6.28f, 0.0174f, 0.12f, 3.5f, 0.95, 0.0, 0.04, 0.01, 0.5);
  Transform2D Trs, robot_pose;
  GridMapper grid(0.05, -10.0, 10.0, -10.0, 10.0, props, Trs);
  ScanAlignment aligner(props, Trs);   // the device ICP and its search with the default parameters, by the two defines
  ParticleFilter pf(40, 50, 0.1, 0.2, 0.1, 0.2, 1e-10, 1e-10, 1e-10, 1e-10, 1e-8, 1e-8, 1, 20, 1, 10, aligner, robot_pose, grid);
  const MapLocalizeResult r = aligner.localizeInMap(pf, scan);   // the defaults: 360 headings, blocks of 8 x 8 cells, the whole map
  const bool pruned = r.refined_blocks < r.blocks && r.rounds >= 1;
  if (!r.accepted || r.points == 0 || r.occupied == 0 || r.score == 0u) return false;
  const MapSearchResult fine = aligner.searchMap(pf, r.T, scan);   // one cell and one step are the global search's accuracy
  found = fine.accepted ? fine.T : r.T;
  return pruned || (r.ia >= 0 && r.tx >= 0 && r.ty >= 0 && r.quality > 0.7);
}

MapLocalizeResult a_node_that_knows_the_room_it_is_in(ParticleFilter& pf, ScanAlignment& aligner, const std::vector<float>& scan) {
  ICPGlobal g;
  g.ang_count = 180;
  g.ang_step = 2.0 * 3.14159265358979323846 / 180.0;
  g.pool_log2 = 4;
  g.region[0] = 100; g.region[1] = 120; g.region[2] = 259; g.region[3] = 299;
  g.min_quality = 0.7;
  return aligner.localizeInMap(pf, scan, g);
}

// node_calls_device_icp_hyp.cpp — COMPILE-ONLY: a mapping node that is put down somewhere in a map it already holds, in a building that
// may look the same from several places.  It builds the scan matcher and the filter as turtle_mapping_node.cpp does (:389-410), with
// -DTBNAV_SCAN_ALIGNMENT_DEVICE_ICP -DTBNAV_SCAN_ALIGNMENT_SEARCH (host/Makefile), calls ScanAlignment::relocalizeInMapHypotheses and
// ScanAlignment::localizeInMapHypotheses (include/tbnav_icp.h, HYPOTHESES H1-H10; additions, the reference has nothing like them) and
// reads every member of their results.  Nothing here runs.
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
using bmapping::ICPHypotheses;
using bmapping::ICPVerifyMap;
using bmapping::LaserProperties;
using bmapping::MapHypothesesResult;
using bmapping::MapHypothesis;
using bmapping::MapHypothesisChecked;
using bmapping::MapRelocalizeHypothesesResult;
using bmapping::ParticleFilter;
using bmapping::ScanAlignment;
using rigid2d::Transform2D;

static_assert(std::is_same<decltype(MapHypothesis::T), Transform2D>::value, "T is a pose in the world");
static_assert(std::is_same<decltype(MapHypothesis::accepted), bool>::value, "accepted is a flag");
static_assert(std::is_same<decltype(MapHypothesesResult::candidates), long long>::value &&
                  std::is_same<decltype(MapHypothesesResult::floor_blocks), long long>::value,
              "the counts are 64-bit");
static_assert(std::is_same<decltype(MapRelocalizeHypothesesResult::ambiguous), bool>::value, "ambiguous is a flag");
static_assert(std::is_same<decltype(MapRelocalizeHypothesesResult::hypotheses), std::vector<MapHypothesisChecked>>::value, "one record per hypothesis");

// true: exactly one pose of the map explains the scan, and `found` is it
bool a_node_that_is_put_down_in_a_building_with_look_alike_rooms(const std::vector<float>& scan, Transform2D& found) {
  LaserProperties props(0, 6.28f, 0.0174f, 0.12f, 3.5f, 0.95, 0.0, 0.04, 0.01, 0.5);
  Transform2D Trs, robot_pose;
  GridMapper grid(0.05, -10.0, 10.0, -10.0, 10.0, props, Trs);
  ScanAlignment aligner(props, Trs);   // the device ICP and its search with the default parameters, by the two defines
  ParticleFilter pf(40, 50, 0.1, 0.2, 0.1, 0.2, 1e-10, 1e-10, 1e-10, 1e-10, 1e-8, 1e-8, 1, 20, 1, 10, aligner, robot_pose, grid);
  const MapRelocalizeHypothesesResult r = aligner.relocalizeInMapHypotheses(pf, scan);   // the defaults of all four
  int agree = 0;
  for (const MapHypothesisChecked& c : r.hypotheses) {
    const bool ran = c.aligned && c.checked;
    if (ran && c.verified && c.fine.ok && c.check.hit > c.check.through + c.check.missing && c.found.score > 0u && c.found.quality > 0.5) ++agree;
    if (c.found.accepted && c.found.ia >= 0 && c.found.tx >= 0 && c.found.ty >= 0) found = c.T;
  }
  found = r.T;
  const MapHypothesesResult& s = r.found;
  const bool pruned = s.floor_blocks <= s.refined_blocks && s.refined_blocks < s.blocks && s.rounds >= 1 && s.candidates >= s.n_peaks;
  return pruned && s.points > 0 && s.occupied > 0 && s.best_score >= s.floor_score && agree == r.verified_count && r.best == 0 && !r.ambiguous;
}

MapHypothesesResult a_node_that_wants_the_rivals_themselves(ParticleFilter& pf, ScanAlignment& aligner, const std::vector<float>& scan) {
  ICPGlobal g;
  g.ang_count = 72;
  g.ang_step = 2.0 * 3.14159265358979323846 / 72.0;
  ICPHypotheses y;
  y.max_hyp = 16;
  y.floor_q10 = 820;
  y.sep_cells = 12;
  y.sep_steps = 2;
  y.wrap = true;
  return aligner.localizeInMapHypotheses(pf, scan, g, y);
}

MapRelocalizeHypothesesResult a_node_that_checks_even_what_the_score_rejects(ParticleFilter& pf, ScanAlignment& aligner, const std::vector<float>& scan) {
  return aligner.relocalizeInMapHypotheses(pf, scan, ICPGlobal(), ICPHypotheses(), ICPAlignMap(), ICPVerifyMap(), true);
}

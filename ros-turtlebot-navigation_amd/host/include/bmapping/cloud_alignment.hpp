// bmapping/cloud_alignment.hpp — ScanAlignment with the reference's surface
// (reference bmapping/include/bmapping/cloud_alignment.hpp:28-80, cloud_alignment.cpp:37-72).
//
// The reference wraps pcl::IterativeClosestPoint (PCL, third party, version unpinned, not part of this project).  Here the
// matcher is a pluggable host callable, and the reference's bookkeeping is kept: the first call returns (true, identity)
// and stores the scan (cloud_alignment.cpp:43-50); a failed match does not refresh the stored scan (:62-71).
//
// useDeviceICP() installs the GPU point-to-point ICP (include/tbnav_icp.h, csrc/icp.hip): a restatement of PCL's
// IterativeClosestPoint with the reference's settings, whose arithmetic is fixed in that header.  Parity with PCL itself is
// unpinned.  A failed alignment prints "ICP FAILED TO CONVERGED!" on stdout as pclICP does (:202).  Copies of a
// ScanAlignment (ParticleFilter keeps one, particle_filter.hpp) share the device handle.
//
// Without a matcher the shim returns the initial guess (what a PCL ICP that converges onto its guess returns) and says so
// once on stderr.  Compiling with -DTBNAV_SCAN_ALIGNMENT_DEVICE_ICP makes the constructor call useDeviceICP(), so a node
// built unchanged against this header runs with the device ICP.  The define only changes a default
// argument, which is evaluated where the constructor is called: objects compiled with and without it link together.
//
// useDeviceICP(device, ICPMetric::PointToLine) installs the same device ICP with its point-to-line metric (tbnav_icp.h,
// POINT-TO-LINE METRIC): an addition with NO counterpart in the reference, which only ever runs PCL's point-to-point ICP.
// useDeviceICP(device) stays point-to-point.  Compiling with -DTBNAV_SCAN_ALIGNMENT_POINT_TO_LINE beside
// -DTBNAV_SCAN_ALIGNMENT_DEVICE_ICP makes the constructor choose the line metric; it too only changes a default argument
// (alone, without the first define, it has no effect).
//
// useDeviceICP(device, metric, ICPSearch) puts the device ICP's correlative search (tbnav_icp.h, CORRELATIVE SEARCH) in front
// of every alignment: a window of poses round the guess is scored against a table of the previous scan and the ICP starts from
// the best one when it is good enough, so a guess that is off by more than the ICP's basin (a wheel slip, a bumped robot)
// no longer ends in a confident wrong answer.  It too is an addition with NO counterpart in the reference, and off unless
// asked for: the two overloads above keep their meaning.  -DTBNAV_SCAN_ALIGNMENT_SEARCH beside
// -DTBNAV_SCAN_ALIGNMENT_DEVICE_ICP makes the constructor turn the search on with its default parameters; it only changes a
// default argument as well (alone it has no effect).
//
// ICPSearch::shape = true adds the shape of the search's score volume (tbnav_icp.h, items F1-F6; tbnav_icp_set_search_shape):
// along a direction in which the scores are flat, a corridor's axis, the guess is kept instead of being pulled to where the two
// scans overlay.  Off unless asked for.  -DTBNAV_SCAN_ALIGNMENT_SEARCH_SHAPE beside the three defines above makes the
// constructor's search carry shape = true; it only changes a default argument too (without the search it has no effect).
//
// ICPSearch::wide = true adds the search's wide second stage (tbnav_icp.h, items W1-W8; tbnav_icp_set_search_wide): a window of up
// to +-64 cells and +-180 steps, scored only when the first stage is rejected (wide_when = OnReject, the default), so a guess
// that is metres off is found and a good guess pays nothing.  Off unless asked for.  -DTBNAV_SCAN_ALIGNMENT_SEARCH_WIDE beside
// -DTBNAV_SCAN_ALIGNMENT_DEVICE_ICP and -DTBNAV_SCAN_ALIGNMENT_SEARCH makes the constructor's search carry wide = true; it only
// changes a default argument too (without the search it has no effect).
//
// searchMap(filter, guess_world, scan) (an addition too; tbnav_icp.h, MAP SEARCH M1-M9) scores a window of poses round a guess given
// in the WORLD against the map of the filter's best particle, on the device, with the search parameters useDeviceICP was given (the
// defaults without any): for a pose that has drifted over many scans, a robot that was picked up, a filter restarted in a map it
// already holds, where the previous scan is as wrong as the guess.  It needs useDeviceICP (std::logic_error otherwise), a filter on
// one GPU (std::runtime_error for one over several) whose cells are the search's; it is not wired into pclICPWrapper or SLAM.
//
// localizeInMap(filter, scan, ICPGlobal) (an addition too; tbnav_icp.h, GLOBAL SEARCH L1-L10) takes NO guess: every heading at every
// cell of the map of the filter's best particle is scored on the device, blocks of cells pruned by an exact bound.  Same needs as
// searchMap; the result is good to one cell and one angle step (alignToMap refines it below a cell; relocalizeInMap is the two in a row), and a symmetric
// building has several equal answers of which the lowest index is returned.
#ifndef TBNAV_BMAPPING_CLOUD_ALIGNMENT_HPP
#define TBNAV_BMAPPING_CLOUD_ALIGNMENT_HPP

#include <functional>
#include <iostream>
#include <memory>
#include <vector>

#include "bmapping/sensor_model.hpp"
#include "rigid2d/rigid2d.hpp"

#ifdef TBNAV_SCAN_ALIGNMENT_DEVICE_ICP
#define TBNAV_SCAN_ALIGNMENT_DEVICE_ICP_DEFAULT true
#else
#define TBNAV_SCAN_ALIGNMENT_DEVICE_ICP_DEFAULT false
#endif

#ifdef TBNAV_SCAN_ALIGNMENT_POINT_TO_LINE
#define TBNAV_SCAN_ALIGNMENT_METRIC_DEFAULT ::bmapping::ICPMetric::PointToLine
#else
#define TBNAV_SCAN_ALIGNMENT_METRIC_DEFAULT ::bmapping::ICPMetric::PointToPoint
#endif

#ifdef TBNAV_SCAN_ALIGNMENT_SEARCH
#define TBNAV_SCAN_ALIGNMENT_SEARCH_DEFAULT true
#else
#define TBNAV_SCAN_ALIGNMENT_SEARCH_DEFAULT false
#endif

#ifdef TBNAV_SCAN_ALIGNMENT_SEARCH_SHAPE
#define TBNAV_SCAN_ALIGNMENT_SEARCH_SHAPE_DEFAULT true
#else
#define TBNAV_SCAN_ALIGNMENT_SEARCH_SHAPE_DEFAULT false
#endif

#ifdef TBNAV_SCAN_ALIGNMENT_SEARCH_WIDE
#define TBNAV_SCAN_ALIGNMENT_SEARCH_WIDE_DEFAULT true
#else
#define TBNAV_SCAN_ALIGNMENT_SEARCH_WIDE_DEFAULT false
#endif

namespace bmapping {

using rigid2d::Transform2D;

/// (addition) what the device ICP minimises: PointToPoint is the reference's (PCL's) metric and the default
enum class ICPMetric { PointToPoint, PointToLine };

/// (addition) when the search's wide second stage runs: TBNAV_ICP_WIDE_ON_REJECT, _ON_REJECT_OR_EDGE, _ALWAYS
enum class ICPWideWhen { OnReject = 0, OnRejectOrEdge = 1, Always = 2 };

/// (addition) the correlative search in front of the device ICP: tbnav_icp_search_params with its defaults
struct ICPSearch {
  double resolution = 0.05;    ///< table cell (m)
  double half_extent = 4.0;    ///< half the table's side (m)
  double sigma = 0.05;         ///< Gaussian width of the stamp (m)
  int stamp_cells = 3;         ///< the stamp's half width in cells, 1..8
  int lin_cells = 6;           ///< window +-lin_cells cells in x and y, 0..16
  int ang_steps = 20;          ///< window +-ang_steps steps of ang_step, 0..90
  double ang_step = 3.14159265358979323846 / 180.0;
  int slack_q10 = 0;           ///< selection slack in 1/1024, 0..1023
  double min_quality = 0.5;    ///< acceptance threshold
  bool shape = false;          ///< the shape of the score volume (tbnav_icp_search_shape_params with its defaults below)
  int shape_drop_q10 = 256;    ///< how far below the chosen score a candidate still counts, in 1/1024, 0..1023
  double shape_flat_cells2 = 2.0;  ///< second moment (cells^2) above which a direction is flat, > 0
  bool wide = false;           ///< the wide second stage (tbnav_icp_search_wide_params with its defaults below)
  int wide_lin_cells = 48;     ///< its window +-wide_lin_cells cells, lin_cells..64
  int wide_ang_steps = 45;     ///< its window +-wide_ang_steps steps of ang_step, ang_steps..180
  ICPWideWhen wide_when = ICPWideWhen::OnReject;  ///< when it runs
};

class ParticleFilter;   // bmapping/particle_filter.hpp

/// (addition) what ScanAlignment::searchMap returns: tbnav_icp_search_info's T, quality, accepted and at_edge
struct MapSearchResult {
  Transform2D T;          ///< the best pose of the window, in the world (the guess's where nothing scored)
  double quality = 0.0;   ///< score / (255 * points), 0..1
  bool accepted = false;  ///< quality >= min_quality, with points in the scan and occupied cells in the window
  bool at_edge = false;   ///< the choice sits on the border of its window: the truth may lie outside it
};

/// (addition) the global search's parameters: tbnav_icp_global_params with its defaults
struct ICPGlobal {
  int ang_count = 360;         ///< headings, 1..720
  double ang_step = 3.14159265358979323846 / 180.0;
  int pool_log2 = 3;           ///< blocks of 2^pool_log2 cells a side, 1..5
  int region[4] = {-1, -1, -1, -1};   ///< tx0, ty0, tx1, ty1 inclusive cells; all -1: the whole map
  double min_quality = 0.5;    ///< acceptance threshold
};

/// (addition) what ScanAlignment::localizeInMap returns: tbnav_icp_global_info
struct MapLocalizeResult {
  Transform2D T;               ///< the best pose, in the world: a heading step and a cell centre
  double quality = 0.0;        ///< score / (255 * points), 0..1
  bool accepted = false;       ///< quality >= min_quality, with points in the scan and occupied cells in the map
  int ia = 0, tx = 0, ty = 0;  ///< the chosen heading and cell
  unsigned score = 0;
  int points = 0, occupied = 0;
  long long blocks = 0, refined_blocks = 0;   ///< all blocks of the search, and those whose candidates were scored
  int rounds = 0;
};

/// (addition) the map alignment's parameters: tbnav_icp_align_map_params with its defaults
struct ICPAlignMap {
  int half_cells = 128;        ///< the window +-half_cells round the guess's cell, 8..256
  int gate_cells = 10;         ///< a point pairs with an occupied cell at most this far from its own, 1..16
  int feature_cells = 2;       ///< the line of a cell is fitted over +-feature_cells, 1..4
  double max_flatness = 0.25;  ///< lmin / lmax above which a cell hands out no direction, 0 <= f < 1
};

/// (addition) what ScanAlignment::alignToMap returns: tbnav_icp_align_map's T, ok and tbnav_icp_info
struct MapAlignResult {
  Transform2D T;               ///< the aligned pose in the world; the guess unchanged when ok is false
  bool ok = false;             ///< converged (ITERATIONS, TRANSFORM, ABS_MSE or REL_MSE)
  int iterations = 0, correspondences = 0, criterion = 0;
  double mse = 0.0;
};

/// (addition) what ScanAlignment::relocalizeInMap returns: both records; aligned is false when the search was not accepted
struct MapRelocalizeResult {
  MapLocalizeResult found;
  MapAlignResult fine;
  bool aligned = false;
  Transform2D T;               ///< fine.T when aligned and fine.ok, else found.T
};

/// (addition) the map check's parameters: tbnav_icp_verify_map_params with its defaults
struct ICPVerifyMap {
  int half_cells = 96;         ///< the window +-half_cells round the sensor's cell, 8..128
  int slack_cells = 2;         ///< k: a wall within k cells of a beam's end explains it, 0..8
  int max_through_q10 = 102;   ///< accepted while through * 1024 <= this * walked, 0..1024
  int max_missing_q10 = 102;   ///< ... and missing * 1024 <= this * walked
  int min_hit_q10 = 512;       ///< ... and hit * 1024 >= this * walked
};

/// (addition) what ScanAlignment::verifyInMap returns: tbnav_icp_verify_map_info
struct MapVerifyResult {
  bool accepted = false;       ///< the map does not contradict the pose (tbnav_icp.h, MAP CHECK V7)
  int points = 0, outside = 0, walked = 0;
  int hit = 0, through = 0, missing = 0, unseen = 0, undecided = 0;   ///< they sum to walked
  long long free_cells = 0, unknown_cells = 0;
  int sensor_cell[2] = {0, 0};
  int sensor_class = 0;        ///< 0 unknown, 1 free, 2 occupied, 3 known and neither
};

/// (addition) what ScanAlignment::relocalizeInMapChecked returns: all three records.  aligned: the alignment ran; checked: the check ran
/// (at fine.T when the alignment converged, else at found.T); verified: it ran and accepts the pose
struct MapRelocalizeCheckedResult {
  MapLocalizeResult found;
  MapAlignResult fine;
  MapVerifyResult check;
  bool aligned = false, checked = false, verified = false;
  Transform2D T;               ///< the pose that was checked, or found.T when none was
};

/// (addition) the hypotheses' parameters: tbnav_icp_hyp_params with its defaults (tbnav_icp.h, HYPOTHESES H1)
struct ICPHypotheses {
  int max_hyp = 8;             ///< K: how many peaks come back, 1..64
  int floor_q10 = 768;         ///< a peak scores at least this share of the best score, in 1/1024, 1..1024
  int sep_cells = 8;           ///< no two peaks within this many cells of each other in x and y ..., 0..64
  int sep_steps = 10;          ///< ... and this many heading steps, 0..720
  bool wrap = true;            ///< headings NA - 1 and 0 are neighbours
};

/// (addition) what ScanAlignment::localizeInMapHypotheses returns: tbnav_icp_hypothesis per peak, best first, and tbnav_icp_hyp_info
struct MapHypothesis {
  Transform2D T;               ///< a heading step and a cell centre, in the world
  double quality = 0.0;
  bool accepted = false;       ///< quality >= min_quality, with points in the scan and occupied cells in the map
  int ia = 0, tx = 0, ty = 0;
  unsigned score = 0;
};
struct MapHypothesesResult {
  std::vector<MapHypothesis> hypotheses;   ///< the first min(max_hyp, n_peaks) peaks in descending score, then ascending index
  int n_peaks = 0;
  unsigned best_score = 0, floor_score = 0;
  int points = 0, occupied = 0;
  long long blocks = 0, floor_blocks = 0, refined_blocks = 0, candidates = 0;
  int rounds = 0;
};

/// (addition) one hypothesis through ScanAlignment::relocalizeInMapHypotheses.  aligned / checked: the alignment / the check ran on it
/// (the check at fine.T when the alignment converged, else at found.T); verified: it ran and accepts the pose
struct MapHypothesisChecked {
  MapHypothesis found;
  MapAlignResult fine;
  MapVerifyResult check;
  bool aligned = false, checked = false, verified = false;
  Transform2D T;               ///< the pose that was checked, or found.T when none was
};
struct MapRelocalizeHypothesesResult {
  MapHypothesesResult found;
  std::vector<MapHypothesisChecked> hypotheses;
  int verified_count = 0;
  int best = -1;               ///< the lowest index verified, -1 when none is
  bool ambiguous = false;      ///< verified_count > 1: the map holds more than one pose that explains the scan
  Transform2D T;               ///< best's pose, or hypothesis 0's when none is verified (the identity when there is no hypothesis)
};

class ScanAlignment {
 public:
  /// matcher(T_out, T_init, previous_scan, current_scan) -> converged
  using Matcher = std::function<bool(Transform2D&, const Transform2D&, const std::vector<float>&, const std::vector<float>&)>;

  ScanAlignment(const LaserProperties& props, const Transform2D& Trs, bool device_icp = TBNAV_SCAN_ALIGNMENT_DEVICE_ICP_DEFAULT,
                ICPMetric device_metric = TBNAV_SCAN_ALIGNMENT_METRIC_DEFAULT, bool device_search = TBNAV_SCAN_ALIGNMENT_SEARCH_DEFAULT,
                bool device_search_shape = TBNAV_SCAN_ALIGNMENT_SEARCH_SHAPE_DEFAULT,
                bool device_search_wide = TBNAV_SCAN_ALIGNMENT_SEARCH_WIDE_DEFAULT)
      : props_(props), Trs_(Trs) {
    if (device_icp && device_search) {
      ICPSearch search;
      search.shape = device_search_shape;
      search.wide = device_search_wide;
      useDeviceICP(-1, device_metric, search);
    } else if (device_icp) useDeviceICP(-1, device_metric);
  }

  /// plug in a real scan matcher (e.g. a PCL ICP wrapper in a catkin workspace that has PCL)
  void setMatcher(Matcher m) { matcher_ = std::move(m); }
  /// (addition) the GPU ICP as the matcher, on `device` (-1: the current one); throws std::runtime_error without a GPU
  void useDeviceICP(int device = -1) { useDeviceICP(device, ICPMetric::PointToPoint); }
  /// (addition) the same with the metric named: PointToLine has no counterpart in the reference (default window and gap)
  void useDeviceICP(int device, ICPMetric metric);
  /// (addition) the same with the correlative search in front of every alignment; throws std::invalid_argument for
  /// parameters outside their limits
  void useDeviceICP(int device, ICPMetric metric, const ICPSearch& search);

  /// (addition) the correlative search of `scan` against the map of the filter's best particle from a guess in the world
  /// (tbnav_icp.h, MAP SEARCH).  Throws std::logic_error without useDeviceICP, std::runtime_error for a filter over several GPUs,
  /// std::invalid_argument for a guess outside the map (the reference's out-of-world text) or cells that are not the filter's.
  MapSearchResult searchMap(ParticleFilter& filter, const Transform2D& guess_world, const std::vector<float>& scan);

  /// (addition) where `scan` was taken in the map of the filter's best particle, with no guess (tbnav_icp.h, GLOBAL SEARCH).
  /// Throws as searchMap does; std::invalid_argument for parameters outside their limits.
  MapLocalizeResult localizeInMap(ParticleFilter& filter, const std::vector<float>& scan, const ICPGlobal& params = {});

  /// (addition) `scan` aligned to the map of the filter's best particle from a guess in the world, below one cell (tbnav_icp.h, MAP
  /// ALIGNMENT A1-A11).  Throws as searchMap does; std::invalid_argument for parameters outside their limits.
  MapAlignResult alignToMap(ParticleFilter& filter, const Transform2D& guess_world, const std::vector<float>& scan,
                            const ICPAlignMap& params = {});
  /// (addition) localizeInMap, then alignToMap from its pose when it is accepted
  MapRelocalizeResult relocalizeInMap(ParticleFilter& filter, const std::vector<float>& scan, const ICPGlobal& global = {},
                                      const ICPAlignMap& align = {});

  /// (addition) the pose `pose_world` checked against the walls and the free space of the map of the filter's best particle with
  /// `scan` (tbnav_icp.h, MAP CHECK V1-V10).  Throws as alignToMap does.
  MapVerifyResult verifyInMap(ParticleFilter& filter, const Transform2D& pose_world, const std::vector<float>& scan,
                              const ICPVerifyMap& params = {});
  /// (addition) localizeInMap; alignToMap from its pose when it is accepted or even_if_rejected is set; then verifyInMap at the aligned
  /// pose, or at the found pose when the alignment did not converge.  relocalizeInMap itself is untouched.
  MapRelocalizeCheckedResult relocalizeInMapChecked(ParticleFilter& filter, const std::vector<float>& scan, const ICPGlobal& global = {},
                                                    const ICPAlignMap& align = {}, const ICPVerifyMap& verify = {},
                                                    bool even_if_rejected = false);

  /// (addition) the global search's separated peaks, best first (tbnav_icp.h, HYPOTHESES H1-H10).  Throws as localizeInMap does.
  MapHypothesesResult localizeInMapHypotheses(ParticleFilter& filter, const std::vector<float>& scan, const ICPGlobal& global = {},
                                              const ICPHypotheses& hyp = {});
  /// (addition) localizeInMapHypotheses, ONE tbnav_icp_align_map_batch from the hypotheses that are accepted (all of them when
  /// even_if_rejected) and ONE tbnav_icp_verify_map_batch of each at its aligned pose, or at its found pose where the alignment did not
  /// converge: three synchronous calls whatever max_hyp is.  relocalizeInMap and relocalizeInMapChecked are untouched.
  MapRelocalizeHypothesesResult relocalizeInMapHypotheses(ParticleFilter& filter, const std::vector<float>& scan, const ICPGlobal& global = {},
                                                          const ICPHypotheses& hyp = {}, const ICPAlignMap& align = {},
                                                          const ICPVerifyMap& verify = {}, bool even_if_rejected = false);

  bool pclICPWrapper(Transform2D& T, const Transform2D& T_init, const std::vector<float>& scan) {
    if (!have_prev_) {
      prev_scan_ = scan;
      have_prev_ = true;
      T = Transform2D();
      return true;
    }
    bool ok = true;
    if (matcher_) ok = matcher_(T, T_init, prev_scan_, scan);
    else {
      // No scan matcher plugged in: the initial guess goes back unchanged (what a PCL ICP that converges onto its guess returns).
      // A node linked against this header WITHOUT setMatcher() therefore runs on odometry alone — say so, once.
      if (!warned_) {
        std::cerr << "bmapping::ScanAlignment: no scan matcher set (setMatcher); pclICPWrapper returns its initial guess" << std::endl;
        warned_ = true;
      }
      T = T_init;
    }
    if (ok) prev_scan_ = scan;
    return ok;
  }

 private:
  void installDeviceICP(int device, ICPMetric metric, const ICPSearch* search);

  LaserProperties props_;
  Transform2D Trs_;
  Matcher matcher_;
  std::shared_ptr<void> device_;   // the tbnav_icp handle useDeviceICP made (the matcher holds it too); copies share it
  std::vector<float> prev_scan_;
  bool have_prev_ = false;
  bool warned_ = false;
};

}  // namespace bmapping
#endif

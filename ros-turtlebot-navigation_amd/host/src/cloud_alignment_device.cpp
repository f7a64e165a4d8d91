// cloud_alignment_device.cpp — ScanAlignment::useDeviceICP: the device ICP of include/tbnav_icp.h as the shim's matcher, with
// its point-to-point metric (the reference's) or its point-to-line metric (an addition), and optionally its correlative search
// in front of either (an addition too), with or without the shape of its score volume.
#include <iostream>
#include <memory>
#include <stdexcept>
#include <string>

#include "bmapping/cloud_alignment.hpp"
#include "bmapping/particle_filter.hpp"
#include "tbnav_icp.h"

namespace bmapping {

void ScanAlignment::useDeviceICP(int device, ICPMetric metric) { installDeviceICP(device, metric, nullptr); }

void ScanAlignment::useDeviceICP(int device, ICPMetric metric, const ICPSearch& search) { installDeviceICP(device, metric, &search); }

void ScanAlignment::installDeviceICP(int device, ICPMetric metric, const ICPSearch* search) {
  tbnav_icp_params p;
  tbnav_icp_default_params(&p);  // the reference's settings (cloud_alignment.cpp:21-34)
  p.beam_min = props_.beam_min; p.beam_max = props_.beam_max; p.beam_delta = props_.beam_delta;
  p.range_min = props_.range_min; p.range_max = props_.range_max;
  const auto trs = Trs_.displacement();
  p.Trs[0] = trs.theta; p.Trs[1] = trs.x; p.Trs[2] = trs.y;
  p.device = device;
  tbnav_icp* raw = nullptr;
  const int rc = tbnav_icp_create(&p, &raw);
  if (rc != TBNAV_OK) {
    std::string msg = std::string("bmapping::ScanAlignment::useDeviceICP: ") + tbnav_status_string(rc);
    const char* hip = tbnav_last_hip_error();
    if (hip && *hip) msg += std::string(" [") + hip + "]";
    throw std::runtime_error(msg);
  }
  // the matcher holds the handle: copies of this object (and of the std::function) share it
  std::shared_ptr<tbnav_icp> h(raw, tbnav_icp_destroy);
  device_ = h;
  if (metric == ICPMetric::PointToLine) {
    const int mrc = tbnav_icp_set_metric(raw, TBNAV_ICP_METRIC_LINE, 0, 0.0);  // the default window and gap
    if (mrc != TBNAV_OK) throw std::runtime_error(std::string("bmapping::ScanAlignment::useDeviceICP: ") + tbnav_status_string(mrc));
  }
  if (search) {
    tbnav_icp_search_params sp;
    tbnav_icp_default_search_params(&sp);
    sp.resolution = search->resolution; sp.half_extent = search->half_extent; sp.sigma = search->sigma;
    sp.stamp_cells = search->stamp_cells; sp.lin_cells = search->lin_cells; sp.ang_steps = search->ang_steps;
    sp.ang_step = search->ang_step; sp.slack_q10 = search->slack_q10; sp.min_quality = search->min_quality;
    const int src = tbnav_icp_set_search(raw, &sp);
    if (src == TBNAV_ERR_INVALID_ARG) throw std::invalid_argument("bmapping::ScanAlignment::useDeviceICP: search parameters outside their limits");
    if (src != TBNAV_OK) throw std::runtime_error(std::string("bmapping::ScanAlignment::useDeviceICP: ") + tbnav_status_string(src));
    if (search->shape) {
      tbnav_icp_search_shape_params fp;
      tbnav_icp_default_search_shape_params(&fp);
      fp.drop_q10 = search->shape_drop_q10; fp.flat_cells2 = search->shape_flat_cells2;
      const int frc = tbnav_icp_set_search_shape(raw, &fp);
      if (frc == TBNAV_ERR_INVALID_ARG) throw std::invalid_argument("bmapping::ScanAlignment::useDeviceICP: search shape parameters outside their limits");
      if (frc != TBNAV_OK) throw std::runtime_error(std::string("bmapping::ScanAlignment::useDeviceICP: ") + tbnav_status_string(frc));
    }
    if (search->wide) {
      tbnav_icp_search_wide_params wp;
      tbnav_icp_default_search_wide_params(&wp);
      wp.lin_cells = search->wide_lin_cells; wp.ang_steps = search->wide_ang_steps; wp.when = static_cast<int32_t>(search->wide_when);
      const int wrc = tbnav_icp_set_search_wide(raw, &wp);
      if (wrc == TBNAV_ERR_INVALID_ARG) throw std::invalid_argument("bmapping::ScanAlignment::useDeviceICP: wide search parameters outside their limits");
      if (wrc != TBNAV_OK) throw std::runtime_error(std::string("bmapping::ScanAlignment::useDeviceICP: ") + tbnav_status_string(wrc));
    }
  }
  matcher_ = [h](Transform2D& T, const Transform2D& T_init, const std::vector<float>& target, const std::vector<float>& source) {
    if (target.size() != source.size()) throw std::invalid_argument("bmapping::ScanAlignment: scans of different lengths");
    const auto g = T_init.displacement();
    const double tinit[3] = {g.theta, g.x, g.y};
    double out[3];
    tbnav_icp_info info{};
    const int rc = tbnav_icp_match(h.get(), target.data(), source.data(), (int32_t)source.size(), tinit, out, &info);
    if (rc != TBNAV_OK) {
      std::string msg = std::string("bmapping::ScanAlignment::pclICP: ") + tbnav_status_string(rc);
      const char* hip = tbnav_last_hip_error();
      if (hip && *hip) msg += std::string(" [") + hip + "]";
      if (rc == TBNAV_ERR_INVALID_ARG) throw std::invalid_argument(msg);
      throw std::runtime_error(msg);
    }
    if (info.criterion < TBNAV_ICP_ITERATIONS || info.criterion > TBNAV_ICP_REL_MSE) {
      std::cout << "ICP FAILED TO CONVERGED!" << std::endl;  // cloud_alignment.cpp:202
      return false;
    }
    T = Transform2D(rigid2d::Vector2D(out[1], out[2]), out[0]);  // :206-217
    return true;
  };
}

MapSearchResult ScanAlignment::searchMap(ParticleFilter& filter, const Transform2D& guess_world, const std::vector<float>& scan) {
  if (!device_) throw std::logic_error("bmapping::ScanAlignment::searchMap: useDeviceICP first");
  if (filter.g_) throw std::runtime_error("bmapping::ScanAlignment::searchMap: a filter over several GPUs is not supported");
  const auto g = guess_world.displacement();
  const double tinit[3] = {g.theta, g.x, g.y};
  tbnav_icp_search_info info{};
  const int rc = tbnav_icp_search_map(static_cast<tbnav_icp*>(device_.get()), filter.h_, TBNAV_ICP_MAP_BEST_PARTICLE, scan.data(),
                                      (int32_t)scan.size(), tinit, &info);
  if (rc != TBNAV_OK) {
    const std::string text = tbnav_status_string(rc);
    if (rc == TBNAV_ERR_OUT_OF_WORLD) throw std::invalid_argument(text);  // what the reference throws (grid_mapper.cpp:856)
    std::string msg = "bmapping::ScanAlignment::searchMap: " + text;
    if (rc == TBNAV_ERR_INVALID_ARG) throw std::invalid_argument(msg);
    const char* hip = tbnav_last_hip_error();
    if (hip && *hip) msg += std::string(" [") + hip + "]";
    throw std::runtime_error(msg);
  }
  MapSearchResult out;
  out.T = Transform2D(rigid2d::Vector2D(info.T[1], info.T[2]), info.T[0]);
  out.quality = info.quality;
  out.accepted = info.accepted != 0;
  out.at_edge = info.at_edge != 0;
  return out;
}

MapLocalizeResult ScanAlignment::localizeInMap(ParticleFilter& filter, const std::vector<float>& scan, const ICPGlobal& params) {
  if (!device_) throw std::logic_error("bmapping::ScanAlignment::localizeInMap: useDeviceICP first");
  if (filter.g_) throw std::runtime_error("bmapping::ScanAlignment::localizeInMap: a filter over several GPUs is not supported");
  tbnav_icp_global_params gp;
  tbnav_icp_default_global_params(&gp);
  gp.ang_count = params.ang_count;
  gp.ang_step = params.ang_step;
  gp.pool_log2 = params.pool_log2;
  for (int i = 0; i < 4; ++i) gp.region[i] = params.region[i];
  gp.min_quality = params.min_quality;
  tbnav_icp_global_info info{};
  const int rc = tbnav_icp_localize_map(static_cast<tbnav_icp*>(device_.get()), filter.h_, TBNAV_ICP_MAP_BEST_PARTICLE, scan.data(),
                                        (int32_t)scan.size(), &gp, &info);
  if (rc != TBNAV_OK) {
    std::string msg = std::string("bmapping::ScanAlignment::localizeInMap: ") + tbnav_status_string(rc);
    if (rc == TBNAV_ERR_INVALID_ARG) throw std::invalid_argument(msg);
    const char* hip = tbnav_last_hip_error();
    if (hip && *hip) msg += std::string(" [") + hip + "]";
    throw std::runtime_error(msg);
  }
  MapLocalizeResult out;
  out.T = Transform2D(rigid2d::Vector2D(info.T[1], info.T[2]), info.T[0]);
  out.quality = info.quality;
  out.accepted = info.accepted != 0;
  out.ia = info.ia; out.tx = info.tx; out.ty = info.ty;
  out.score = info.score;
  out.points = info.points; out.occupied = info.occupied;
  out.blocks = info.blocks; out.refined_blocks = info.refined_blocks;
  out.rounds = info.rounds;
  return out;
}

MapAlignResult ScanAlignment::alignToMap(ParticleFilter& filter, const Transform2D& guess_world, const std::vector<float>& scan,
                                         const ICPAlignMap& params) {
  if (!device_) throw std::logic_error("bmapping::ScanAlignment::alignToMap: useDeviceICP first");
  if (filter.g_) throw std::runtime_error("bmapping::ScanAlignment::alignToMap: a filter over several GPUs is not supported");
  tbnav_icp_align_map_params ap;
  tbnav_icp_default_align_map_params(&ap);
  ap.half_cells = params.half_cells;
  ap.gate_cells = params.gate_cells;
  ap.feature_cells = params.feature_cells;
  ap.max_flatness = params.max_flatness;
  const auto g = guess_world.displacement();
  const double tinit[3] = {g.theta, g.x, g.y};
  double out[3] = {0.0, 0.0, 0.0};
  int32_t ok = 0;
  tbnav_icp_info info{};
  const int rc = tbnav_icp_align_map(static_cast<tbnav_icp*>(device_.get()), filter.h_, TBNAV_ICP_MAP_BEST_PARTICLE, scan.data(),
                                     (int32_t)scan.size(), tinit, &ap, out, &ok, &info);
  if (rc != TBNAV_OK) {
    const std::string text = tbnav_status_string(rc);
    if (rc == TBNAV_ERR_OUT_OF_WORLD) throw std::invalid_argument(text);  // what the reference throws (grid_mapper.cpp:856)
    std::string msg = "bmapping::ScanAlignment::alignToMap: " + text;
    if (rc == TBNAV_ERR_INVALID_ARG) throw std::invalid_argument(msg);
    const char* hip = tbnav_last_hip_error();
    if (hip && *hip) msg += std::string(" [") + hip + "]";
    throw std::runtime_error(msg);
  }
  MapAlignResult r;
  r.T = ok ? Transform2D(rigid2d::Vector2D(out[1], out[2]), out[0]) : guess_world;
  r.ok = ok != 0;
  r.iterations = info.iterations; r.correspondences = info.correspondences; r.criterion = info.criterion;
  r.mse = info.mse;
  return r;
}

MapRelocalizeResult ScanAlignment::relocalizeInMap(ParticleFilter& filter, const std::vector<float>& scan, const ICPGlobal& global,
                                                   const ICPAlignMap& align) {
  MapRelocalizeResult r;
  r.found = localizeInMap(filter, scan, global);
  r.T = r.found.T;
  if (!r.found.accepted) return r;
  r.fine = alignToMap(filter, r.found.T, scan, align);
  r.aligned = true;
  if (r.fine.ok) r.T = r.fine.T;
  return r;
}

MapVerifyResult ScanAlignment::verifyInMap(ParticleFilter& filter, const Transform2D& pose_world, const std::vector<float>& scan,
                                           const ICPVerifyMap& params) {
  if (!device_) throw std::logic_error("bmapping::ScanAlignment::verifyInMap: useDeviceICP first");
  if (filter.g_) throw std::runtime_error("bmapping::ScanAlignment::verifyInMap: a filter over several GPUs is not supported");
  tbnav_icp_verify_map_params vp;
  tbnav_icp_default_verify_map_params(&vp);
  vp.half_cells = params.half_cells;
  vp.slack_cells = params.slack_cells;
  vp.max_through_q10 = params.max_through_q10;
  vp.max_missing_q10 = params.max_missing_q10;
  vp.min_hit_q10 = params.min_hit_q10;
  const auto g = pose_world.displacement();
  const double T[3] = {g.theta, g.x, g.y};
  tbnav_icp_verify_map_info info{};
  const int rc = tbnav_icp_verify_map(static_cast<tbnav_icp*>(device_.get()), filter.h_, TBNAV_ICP_MAP_BEST_PARTICLE, scan.data(),
                                      (int32_t)scan.size(), T, &vp, &info);
  if (rc != TBNAV_OK) {
    const std::string text = tbnav_status_string(rc);
    if (rc == TBNAV_ERR_OUT_OF_WORLD) throw std::invalid_argument(text);  // what the reference throws (grid_mapper.cpp:856)
    std::string msg = "bmapping::ScanAlignment::verifyInMap: " + text;
    if (rc == TBNAV_ERR_INVALID_ARG) throw std::invalid_argument(msg);
    const char* hip = tbnav_last_hip_error();
    if (hip && *hip) msg += std::string(" [") + hip + "]";
    throw std::runtime_error(msg);
  }
  MapVerifyResult r;
  r.accepted = info.accepted != 0;
  r.points = info.points; r.outside = info.outside; r.walked = info.walked;
  r.hit = info.hit; r.through = info.through; r.missing = info.missing; r.unseen = info.unseen; r.undecided = info.undecided;
  r.free_cells = info.free_cells; r.unknown_cells = info.unknown_cells;
  r.sensor_cell[0] = info.sensor_cell[0]; r.sensor_cell[1] = info.sensor_cell[1];
  r.sensor_class = info.sensor_class;
  return r;
}

MapRelocalizeCheckedResult ScanAlignment::relocalizeInMapChecked(ParticleFilter& filter, const std::vector<float>& scan, const ICPGlobal& global,
                                                                 const ICPAlignMap& align, const ICPVerifyMap& verify, bool even_if_rejected) {
  MapRelocalizeCheckedResult r;
  r.found = localizeInMap(filter, scan, global);
  r.T = r.found.T;
  if (!r.found.accepted && !even_if_rejected) return r;
  r.fine = alignToMap(filter, r.found.T, scan, align);
  r.aligned = true;
  if (r.fine.ok) r.T = r.fine.T;
  r.check = verifyInMap(filter, r.T, scan, verify);
  r.checked = true;
  r.verified = r.check.accepted;
  return r;
}

namespace {
[[noreturn]] void throw_status(const char* where, int rc) {
  const std::string text = tbnav_status_string(rc);
  if (rc == TBNAV_ERR_OUT_OF_WORLD) throw std::invalid_argument(text);  // what the reference throws (grid_mapper.cpp:856)
  std::string msg = std::string("bmapping::ScanAlignment::") + where + ": " + text;
  if (rc == TBNAV_ERR_INVALID_ARG) throw std::invalid_argument(msg);
  const char* hip = tbnav_last_hip_error();
  if (hip && *hip) msg += std::string(" [") + hip + "]";
  throw std::runtime_error(msg);
}
}  // namespace

MapHypothesesResult ScanAlignment::localizeInMapHypotheses(ParticleFilter& filter, const std::vector<float>& scan, const ICPGlobal& global,
                                                           const ICPHypotheses& hyp) {
  if (!device_) throw std::logic_error("bmapping::ScanAlignment::localizeInMapHypotheses: useDeviceICP first");
  if (filter.g_) throw std::runtime_error("bmapping::ScanAlignment::localizeInMapHypotheses: a filter over several GPUs is not supported");
  tbnav_icp_global_params gp;
  tbnav_icp_default_global_params(&gp);
  gp.ang_count = global.ang_count;
  gp.ang_step = global.ang_step;
  gp.pool_log2 = global.pool_log2;
  for (int i = 0; i < 4; ++i) gp.region[i] = global.region[i];
  gp.min_quality = global.min_quality;
  tbnav_icp_hyp_params hp;
  tbnav_icp_default_hyp_params(&hp);
  hp.max_hyp = hyp.max_hyp;
  hp.floor_q10 = hyp.floor_q10;
  hp.sep_cells = hyp.sep_cells;
  hp.sep_steps = hyp.sep_steps;
  hp.wrap = hyp.wrap ? 1 : 0;
  std::vector<tbnav_icp_hypothesis> ys(TBNAV_ICP_HYP_MAX);
  tbnav_icp_hyp_info info{};
  const int rc = tbnav_icp_localize_map_hyp(static_cast<tbnav_icp*>(device_.get()), filter.h_, TBNAV_ICP_MAP_BEST_PARTICLE, scan.data(),
                                            (int32_t)scan.size(), &gp, &hp, ys.data(), (int32_t)ys.size(), &info);
  if (rc != TBNAV_OK) throw_status("localizeInMapHypotheses", rc);
  MapHypothesesResult out;
  for (int i = 0; i < info.n; ++i) {
    MapHypothesis y;
    y.T = Transform2D(rigid2d::Vector2D(ys[i].T[1], ys[i].T[2]), ys[i].T[0]);
    y.quality = ys[i].quality;
    y.accepted = ys[i].accepted != 0;
    y.ia = ys[i].ia; y.tx = ys[i].tx; y.ty = ys[i].ty;
    y.score = ys[i].score;
    out.hypotheses.push_back(y);
  }
  out.n_peaks = info.n_peaks;
  out.best_score = info.best_score; out.floor_score = info.floor_score;
  out.points = info.points; out.occupied = info.occupied;
  out.blocks = info.blocks; out.floor_blocks = info.floor_blocks; out.refined_blocks = info.refined_blocks; out.candidates = info.candidates;
  out.rounds = info.rounds;
  return out;
}

MapRelocalizeHypothesesResult ScanAlignment::relocalizeInMapHypotheses(ParticleFilter& filter, const std::vector<float>& scan,
                                                                       const ICPGlobal& global, const ICPHypotheses& hyp,
                                                                       const ICPAlignMap& align, const ICPVerifyMap& verify,
                                                                       bool even_if_rejected) {
  MapRelocalizeHypothesesResult r;
  r.found = localizeInMapHypotheses(filter, scan, global, hyp);
  std::vector<int> take;
  for (size_t i = 0; i < r.found.hypotheses.size(); ++i) {
    MapHypothesisChecked c;
    c.found = r.found.hypotheses[i];
    c.T = c.found.T;
    r.hypotheses.push_back(c);
    if (c.found.accepted || even_if_rejected) take.push_back((int)i);
  }
  if (!r.hypotheses.empty()) r.T = r.hypotheses[0].T;
  if (take.empty()) return r;
  tbnav_icp* h = static_cast<tbnav_icp*>(device_.get());
  const int32_t n = (int32_t)take.size();
  const std::vector<int32_t> particles((size_t)n, TBNAV_ICP_MAP_BEST_PARTICLE);
  std::vector<double> tinit((size_t)n * 3), tout((size_t)n * 3);
  for (int32_t k = 0; k < n; ++k) {
    const auto g = r.hypotheses[take[k]].found.T.displacement();
    tinit[3 * k] = g.theta; tinit[3 * k + 1] = g.x; tinit[3 * k + 2] = g.y;
  }
  tbnav_icp_align_map_params ap;
  tbnav_icp_default_align_map_params(&ap);
  ap.half_cells = align.half_cells;
  ap.gate_cells = align.gate_cells;
  ap.feature_cells = align.feature_cells;
  ap.max_flatness = align.max_flatness;
  std::vector<int32_t> ok((size_t)n);
  std::vector<tbnav_icp_info> infos((size_t)n);
  int rc = tbnav_icp_align_map_batch(h, filter.h_, scan.data(), (int32_t)scan.size(), n, particles.data(), tinit.data(), &ap, tout.data(),
                                     ok.data(), infos.data());
  if (rc != TBNAV_OK) throw_status("relocalizeInMapHypotheses", rc);
  std::vector<double> tcheck((size_t)n * 3);
  for (int32_t k = 0; k < n; ++k) {
    MapHypothesisChecked& c = r.hypotheses[take[k]];
    c.aligned = true;
    c.fine.ok = ok[k] != 0;
    c.fine.T = ok[k] ? Transform2D(rigid2d::Vector2D(tout[3 * k + 1], tout[3 * k + 2]), tout[3 * k]) : c.found.T;
    c.fine.iterations = infos[k].iterations; c.fine.correspondences = infos[k].correspondences; c.fine.criterion = infos[k].criterion;
    c.fine.mse = infos[k].mse;
    if (c.fine.ok) c.T = c.fine.T;
    // the doubles the calls themselves hold, not a round trip through Transform2D
    for (int j = 0; j < 3; ++j) tcheck[3 * k + j] = ok[k] ? tout[3 * k + j] : tinit[3 * k + j];
  }
  tbnav_icp_verify_map_params vp;
  tbnav_icp_default_verify_map_params(&vp);
  vp.half_cells = verify.half_cells;
  vp.slack_cells = verify.slack_cells;
  vp.max_through_q10 = verify.max_through_q10;
  vp.max_missing_q10 = verify.max_missing_q10;
  vp.min_hit_q10 = verify.min_hit_q10;
  std::vector<tbnav_icp_verify_map_info> checks((size_t)n);
  rc = tbnav_icp_verify_map_batch(h, filter.h_, scan.data(), (int32_t)scan.size(), n, particles.data(), tcheck.data(), &vp, checks.data());
  if (rc != TBNAV_OK) throw_status("relocalizeInMapHypotheses", rc);
  for (int32_t k = 0; k < n; ++k) {
    MapHypothesisChecked& c = r.hypotheses[take[k]];
    const tbnav_icp_verify_map_info& info = checks[k];
    c.checked = true;
    c.check.accepted = info.accepted != 0;
    c.check.points = info.points; c.check.outside = info.outside; c.check.walked = info.walked;
    c.check.hit = info.hit; c.check.through = info.through; c.check.missing = info.missing; c.check.unseen = info.unseen;
    c.check.undecided = info.undecided;
    c.check.free_cells = info.free_cells; c.check.unknown_cells = info.unknown_cells;
    c.check.sensor_cell[0] = info.sensor_cell[0]; c.check.sensor_cell[1] = info.sensor_cell[1];
    c.check.sensor_class = info.sensor_class;
    c.verified = c.check.accepted;
    if (c.verified) {
      if (r.best < 0) r.best = take[k];
      ++r.verified_count;
    }
  }
  r.ambiguous = r.verified_count > 1;
  if (r.best >= 0) r.T = r.hypotheses[r.best].T;
  return r;
}

}  // namespace bmapping

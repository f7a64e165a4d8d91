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

}  // namespace bmapping

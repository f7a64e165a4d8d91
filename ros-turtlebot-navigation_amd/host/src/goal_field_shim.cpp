// goal_field_shim.cpp — planner::GoalField over the C-ABI of include/tbnav_nav.h.  Status codes become the exceptions the other
// shims throw (std::invalid_argument for a bad argument and for the reference's out-of-world text, std::runtime_error otherwise);
// there is no CPU path.
#include <cmath>
#include <stdexcept>
#include <string>

#include "bmapping/particle_filter.hpp"
#include "planner/goal_field.hpp"
#include "tbnav_nav.h"

namespace planner {
namespace {
void check(int rc, const char* where) {
  if (rc == TBNAV_OK) return;
  const std::string text = tbnav_status_string(rc);
  if (rc == TBNAV_ERR_OUT_OF_WORLD) throw std::invalid_argument(text);  // what the reference throws (grid_mapper.cpp:856)
  std::string msg = std::string(where) + ": " + text;
  if (rc == TBNAV_ERR_INVALID_ARG) throw std::invalid_argument(msg);
  const char* hip = tbnav_last_hip_error();
  if (hip && *hip) msg += std::string(" [") + hip + "]";
  throw std::runtime_error(msg);
}
}  // namespace

std::vector<std::uint8_t> navCostFromDistance(const std::vector<double>& occ_dist, int nx, int ny, double r_robot, double r_inflate, double k) {
  if (!(0.0 <= r_robot && r_robot < r_inflate) || !(0.0 <= k && k <= 63.0))
    throw std::invalid_argument("navCostFromDistance: 0 <= r_robot < r_inflate and 0 <= k <= 63 are required");
  if (nx < 0 || ny < 0 || occ_dist.size() != (size_t)nx * (size_t)ny) throw std::invalid_argument("navCostFromDistance: occ_dist.size() != nx * ny");
  std::vector<std::uint8_t> c(occ_dist.size());
  for (size_t i = 0; i < c.size(); ++i) {
    const double d = occ_dist[i];
    double t = (r_inflate - d) / (r_inflate - r_robot);
    t = t > 0.0 ? t : 0.0;   // (a NaN goes to 0)
    t = t < 1.0 ? t : 1.0;
    c[i] = (std::uint8_t)(d <= r_robot ? 0.0 : 1.0 + std::rint(k * t * t));
  }
  return c;
}

GoalField::GoalField(int nx, int ny, double xmin, double ymin, double resolution)
    : nx_(nx), ny_(ny), xmin_(xmin), ymin_(ymin), resolution_(resolution) {
  tbnav_nav_params p{};
  p.nx = nx; p.ny = ny; p.xmin = xmin; p.ymin = ymin; p.resolution = resolution; p.device = -1;
  check(tbnav_nav_create(&p, &h_), "planner::GoalField");
}
GoalField::~GoalField() { tbnav_nav_destroy(h_); }
GoalField::GoalField(GoalField&& o) noexcept
    : h_(o.h_), nx_(o.nx_), ny_(o.ny_), xmin_(o.xmin_), ymin_(o.ymin_), resolution_(o.resolution_) { o.h_ = nullptr; }

void GoalField::setCost(const std::vector<std::uint8_t>& cost) {
  if (cost.size() != (size_t)nx_ * (size_t)ny_) throw std::invalid_argument("setCost: cost.size() != nx * ny");
  check(tbnav_nav_set_cost(h_, cost.data()), "setCost");
}
void GoalField::setCostFrom(bmapping::ParticleFilter& filter, double r_robot, double r_inflate, double k) {
  if (filter.g_) throw std::runtime_error("setCostFrom: a filter over several GPUs is not supported");
  check(tbnav_nav_set_cost_from_rbpf(h_, filter.h_, TBNAV_NAV_BEST_PARTICLE, r_robot, r_inflate, k), "setCostFrom");
}
std::array<int, 2> GoalField::cellOf(double x, double y) const {
  int32_t ix = 0, iy = 0;
  check(tbnav_nav_cell_of(h_, x, y, &ix, &iy), "cellOf");
  return {ix, iy};
}
void GoalField::solve(double x, double y) {
  const auto c = cellOf(x, y);
  check(tbnav_nav_solve(h_, c[0], c[1]), "solve");
}
std::vector<Frontier> GoalField::findFrontiers(bmapping::ParticleFilter& filter, int min_cells) {
  if (filter.g_) throw std::runtime_error("findFrontiers: a filter over several GPUs is not supported");
  tbnav_nav_frontier_info info{};
  check(tbnav_nav_find_frontiers(h_, filter.h_, TBNAV_NAV_BEST_PARTICLE, min_cells, &info), "findFrontiers");
  std::vector<tbnav_nav_frontier> recs((size_t)info.clusters);
  int32_t n = 0;
  if (info.clusters > 0) check(tbnav_nav_frontier_list(h_, recs.data(), info.clusters, &n), "findFrontiers");
  std::vector<Frontier> out((size_t)n);
  for (int i = 0; i < n; ++i) {
    const tbnav_nav_frontier& r = recs[(size_t)i];
    Frontier& f = out[(size_t)i];
    f.root = {r.root[0], r.root[1]};
    f.size = r.size;
    f.seeds = r.seeds != 0;
    f.box = {r.box[0], r.box[1], r.box[2], r.box[3]};
    f.cx = xmin_ + ((double)r.sum_ix / (double)r.size + 0.5) * resolution_;
    f.cy = ymin_ + ((double)r.sum_iy / (double)r.size + 0.5) * resolution_;
  }
  return out;
}
void GoalField::markVisited(double x, double y, double radius_m) {
  const auto c = cellOf(x, y);
  const double cells = std::rint(radius_m / resolution_);
  if (!(cells >= 0.0 && cells <= (double)TBNAV_NAV_MAX_VISIT_RADIUS)) throw std::invalid_argument("markVisited: the radius must be 0 .. 64 cells");
  check(tbnav_nav_mark_visited(h_, c[0], c[1], (int32_t)cells), "markVisited");
}
void GoalField::clearVisited() { check(tbnav_nav_clear_visited(h_), "clearVisited"); }
void GoalField::solveGoals(const std::vector<std::array<double, 2>>& goals) {
  std::vector<int32_t> cells;
  cells.reserve(2 * goals.size());
  for (const auto& g : goals) {
    const auto c = cellOf(g[0], g[1]);
    cells.push_back(c[0]); cells.push_back(c[1]);
  }
  check(tbnav_nav_solve_goals(h_, cells.data(), (int32_t)goals.size()), "solveGoals");
}
bool GoalField::solveToFrontiers() {
  const int rc = tbnav_nav_solve_frontiers(h_);
  if (rc == TBNAV_ERR_UNSUPPORTED) return false;   // the find left no seed
  check(rc, "solveToFrontiers");
  return true;
}
namespace {
int32_t range_cells_of(double range_m, double resolution) {
  const double cells = std::rint(range_m / resolution);
  if (!(cells >= 1.0 && cells <= (double)TBNAV_NAV_MAX_GAIN_RANGE)) throw std::invalid_argument("findFrontiersGain: the range must be 1 .. 128 cells");
  return (int32_t)cells;
}
}  // namespace
std::vector<FrontierGain> GoalField::findFrontiersGain(bmapping::ParticleFilter& filter, double range_m, int min_cells) {
  if (filter.g_) throw std::runtime_error("findFrontiersGain: a filter over several GPUs is not supported");
  check(tbnav_nav_find_frontiers_gain(h_, filter.h_, TBNAV_NAV_BEST_PARTICLE, min_cells, range_cells_of(range_m, resolution_), nullptr, nullptr),
        "findFrontiersGain");
  return frontierGainList();
}
std::array<double, 5> GoalField::profileFindFrontiersGain(bmapping::ParticleFilter& filter, double range_m, int min_cells) {
  if (filter.g_) throw std::runtime_error("profileFindFrontiersGain: a filter over several GPUs is not supported");
  float ms[5] = {0, 0, 0, 0, 0};
  check(tbnav_nav_profile_find_frontiers_gain(h_, filter.h_, TBNAV_NAV_BEST_PARTICLE, min_cells, range_cells_of(range_m, resolution_), nullptr, nullptr, ms),
        "profileFindFrontiersGain");
  return {ms[0] * 1e3, ms[1] * 1e3, ms[2] * 1e3, ms[3] * 1e3, ms[4] * 1e3};
}
GainInfo GoalField::lastGain() const {
  tbnav_nav_gain_info gi{};
  check(tbnav_nav_last_gain(h_, &gi), "lastGain");
  GainInfo out;
  out.computed = gi.computed != 0;
  out.range_cells = gi.range_cells; out.rays = gi.rays; out.viewpoints = gi.viewpoints; out.gain_min = gi.gain_min; out.gain_max = gi.gain_max;
  out.best = {gi.best[0], gi.best[1]};
  return out;
}
std::vector<std::uint32_t> GoalField::frontierGain() {
  std::vector<std::uint32_t> gain((size_t)nx_ * ny_);
  check(tbnav_nav_get_frontier_gain(h_, gain.data()), "frontierGain");
  return gain;
}
std::vector<FrontierGain> GoalField::frontierGainList() {
  int32_t n = 0;
  const int rc = tbnav_nav_frontier_gain_list(h_, nullptr, 0, &n);   // the number first: "buffer too small" with n set
  if (n <= 0) { check(rc, "frontierGainList"); return {}; }
  std::vector<tbnav_nav_frontier_gain> recs((size_t)n);
  check(tbnav_nav_frontier_gain_list(h_, recs.data(), n, &n), "frontierGainList");
  std::vector<FrontierGain> out((size_t)n);
  for (int i = 0; i < n; ++i) {
    out[(size_t)i].root = {recs[(size_t)i].root[0], recs[(size_t)i].root[1]};
    out[(size_t)i].gain_max = recs[(size_t)i].gain_max;
    out[(size_t)i].best = {recs[(size_t)i].best[0], recs[(size_t)i].best[1]};
  }
  return out;
}
std::vector<std::string> GoalField::lastGainKernels() const {
  char names[160];
  check(tbnav_nav_last_gain_kernels(h_, names, (int32_t)sizeof names), "lastGainKernels");
  std::vector<std::string> out;
  std::string cur;
  for (const char* c = names; ; ++c) {
    if (*c == ';' || *c == '\0') { if (!cur.empty()) out.push_back(cur); cur.clear(); if (*c == '\0') break; }
    else cur += *c;
  }
  return out;
}
bool GoalField::solveToFrontiersRanked(int gain_weight) {
  const int rc = tbnav_nav_solve_frontiers_ranked(h_, gain_weight);
  if (rc == TBNAV_ERR_UNSUPPORTED) return false;   // the find left no seed
  check(rc, "solveToFrontiersRanked");
  return true;
}
std::vector<std::uint32_t> GoalField::costToGo() {
  std::vector<std::uint32_t> d((size_t)nx_ * ny_);
  check(tbnav_nav_get_cost_to_go(h_, d.data()), "costToGo");
  return d;
}
std::vector<float> GoalField::field(double cap) {
  std::vector<float> v((size_t)nx_ * ny_);
  check(tbnav_nav_get_field(h_, cap, v.data()), "field");
  return v;
}
std::vector<std::array<int, 2>> GoalField::path(double x, double y) {
  const auto c = cellOf(x, y);
  int32_t n = 0;
  const int rc = tbnav_nav_path(h_, c[0], c[1], nullptr, 0, &n);   // the length first: "buffer too small" with n set
  if (n <= 0) check(rc, "path");
  std::vector<int32_t> cells((size_t)2 * n);
  check(tbnav_nav_path(h_, c[0], c[1], cells.data(), n, &n), "path");
  std::vector<std::array<int, 2>> out((size_t)n);
  for (int i = 0; i < n; ++i) out[i] = {cells[2 * i], cells[2 * i + 1]};
  return out;
}
void GoalField::applyTo(controller::MPPI& mppi, double cap, double weight) {
  check(mppi.g_ ? tbnav_nav_apply_to_mppi_group(h_, mppi.g_, cap, weight) : tbnav_nav_apply_to_mppi(h_, mppi.h_, cap, weight), "applyTo");
}
int GoalField::rounds() const {
  tbnav_nav_solve_info info{};
  check(tbnav_nav_last_solve(h_, &info, nullptr, 0), "rounds");
  return info.rounds;
}

}  // namespace planner

// planner/goal_field.hpp — planner::GoalField: the exact shortest-path cost-to-go to a goal cell over a cost grid, solved on the
// MI355X through the C-ABI of include/tbnav_nav.h (its sections G1-G6 are the specification), and handed to controller::MPPI as a
// cost field without a host round trip.  Not in the reference: its planner package (planner/include/planner/dstar_light.hpp, D* Lite
// over the 8-connected grid with a move priced by the cell entered, dstar_light.cpp:367-461) is never seen by its controller.  A node
// that owns the filter's distance field does
//     planner::GoalField nav(nx, ny, xmin, ymin, resolution);
//     nav.setCost(planner::navCostFromDistance(occ_dist, nx, ny, r_robot, r_inflate, k));
//     nav.solve(goal.x, goal.y);  nav.applyTo(mppi, cap, weight);
// and one that owns the filter itself replaces the second line by nav.setCostFrom(filter, r_robot, r_inflate, k): the grid comes from
// the best particle's map on the device (G7-G9).  A node that EXPLORES has no waypoint to type: it replaces the solve by
//     nav.findFrontiers(filter);  if (!nav.solveToFrontiers()) { /* nothing left to explore */ }
// — the goals are the frontiers of the best particle's map, the border between what it has seen to be free and what it has not seen
// (G10-G16) — and calls nav.markVisited(x, y, radius) where it arrives at a frontier that its scans do not clear.  One that would
// rather drive a little farther to a frontier with more behind it replaces the two calls by
//     nav.findFrontiersGain(filter, range_m);  if (!nav.solveToFrontiersRanked(gain_weight)) { /* nothing left */ }
// (G17-G20: every seed's gain is the unknown cells a scan of that range would look at from it).
// and links libtbnav_host.so + libtbnav_hip.so.
#ifndef TBNAV_PLANNER_GOAL_FIELD_HPP
#define TBNAV_PLANNER_GOAL_FIELD_HPP

#include <array>
#include <cstdint>
#include <string>
#include <vector>

#include "controller/mppi.hpp"

struct tbnav_nav;  // C-ABI handle
namespace bmapping { class ParticleFilter; }  // bmapping/particle_filter.hpp

namespace planner {

/// A cost grid (tbnav_nav.h G2) from distances to the nearest obstacle (nx * ny of them, metres, [nx][ny] with x slow): 0 (blocked)
/// where d <= r_robot; elsewhere 1 + rint(k * t * t), t = (r_inflate - d) / (r_inflate - r_robot) clamped to 0 .. 1 — 1 in the open,
/// 1 + k at the robot's radius; formed in double.  Throws std::invalid_argument unless 0 <= r_robot < r_inflate, 0 <= k <= 63 and
/// occ_dist.size() == nx * ny.
std::vector<std::uint8_t> navCostFromDistance(const std::vector<double>& occ_dist, int nx, int ny, double r_robot, double r_inflate, double k);

/// One cluster of frontier cells (tbnav_nav.h G12, G16).
struct Frontier {
  std::array<int, 2> root{};   ///< the cell whose index ix * ny + iy is the cluster's label: its least
  int size = 0;                ///< cells
  bool seeds = false;          ///< size >= the find's min_cells: its cells are goals of solveToFrontiers
  std::array<int, 4> box{};    ///< ix_min, iy_min, ix_max, iy_max
  double cx = 0.0, cy = 0.0;   ///< the centroid in world coordinates (the mean of the cells' centres)
};

/// What the last find with gain left (tbnav_nav.h G19).
struct GainInfo {
  bool computed = false;          ///< the handle holds the gain of its last find
  int range_cells = 0, rays = 0, viewpoints = 0, gain_min = 0, gain_max = 0;
  std::array<int, 2> best{{-1, -1}};   ///< the least cell index with gain_max; (-1, -1) with no viewpoint
};

/// One cluster's gain (tbnav_nav.h G19).
struct FrontierGain {
  std::array<int, 2> root{};           ///< as in Frontier
  int gain_max = 0;                    ///< the most over the cluster's cells; 0 where the cluster is no seed
  std::array<int, 2> best{{-1, -1}};   ///< the least cell index of the cluster with it; (-1, -1) where it is no seed
};

class GoalField {
 public:
  /// G1: nx x ny cells of `resolution` metres, (xmin, ymin) the outer corner of cell (0, 0).  Throws std::invalid_argument on a grid
  /// the library rejects and std::runtime_error without a GPU (there is no CPU path).
  GoalField(int nx, int ny, double xmin, double ymin, double resolution);
  ~GoalField();
  GoalField(const GoalField&) = delete;  // the handle owns device memory
  GoalField& operator=(const GoalField&) = delete;
  GoalField(GoalField&& o) noexcept;

  /// G2: nx * ny costs, 0 = blocked, 1 .. 64 the multiplier a move pays for entering the cell; what the next solve uses.
  void setCost(const std::vector<std::uint8_t>& cost);
  /// G7-G9: the grid navCostFromDistance would give for the distance field of the filter's best particle, formed on the device from
  /// that particle's occupancy bits — no distance field is stored, nothing crosses the host.  This grid must be the filter's (side,
  /// xmin, ymin, resolution), else std::invalid_argument, as for r_robot, r_inflate, k outside 0 <= r_robot < r_inflate <= 10,
  /// 0 <= k <= 63.  Throws std::runtime_error for a filter built with n_gpus > 1 and where r_inflate reaches further than 31 cells.
  void setCostFrom(bmapping::ParticleFilter& filter, double r_robot, double r_inflate, double k);
  /// G3-G4 with the goal at the cell of the world position (x, y).  Throws std::invalid_argument when that position is outside the
  /// grid (the reference's "NOT in the bounds of the world") or its cell is blocked; the last solution then stays.
  void solve(double x, double y);
  /// G10-G13 on the map of the filter's best particle: frontier cells, their 8-connected clusters, and as seeds the cells of the
  /// clusters of at least min_cells cells.  Returns one Frontier per cluster in ascending label order.  Needs a cost grid (setCost /
  /// setCostFrom) and this grid to be the filter's, else std::invalid_argument, as for min_cells < 1; std::runtime_error for a filter
  /// built with n_gpus > 1.
  std::vector<Frontier> findFrontiers(bmapping::ParticleFilter& filter, int min_cells = 8);
  /// G14: the disc of radius_m (rounded to cells, at most 64) round the cell of (x, y) joins the visited mask: no cell of it is a
  /// frontier cell any more.  Throws std::invalid_argument for a position outside the grid or a radius outside 0 .. 64 cells.
  void markVisited(double x, double y, double radius_m);
  void clearVisited();
  /// G15: the cost-to-go to the NEAREST of the world positions (x, y).  Throws like solve where one of them is outside or blocked.
  void solveGoals(const std::vector<std::array<double, 2>>& goals);
  /// G15 with the seeds of the last findFrontiers as goals, taken from the device.  false where that find left no seed — nothing left
  /// to explore; the last solution then stays.  Throws std::invalid_argument before any find, or when the cost grid or the visited
  /// mask was set again since.
  bool solveToFrontiers();
  /// G17-G19: findFrontiers, and in the same call the gain of every seed cell: the distinct unknown cells that integer rays of
  /// range_m (rounded to cells, 1 .. 128) see from it in the same particle's map.  One FrontierGain per cluster, in findFrontiers' order.
  /// Throws like findFrontiers, and std::invalid_argument for a range outside 1 .. 128 cells.
  std::vector<FrontierGain> findFrontiersGain(bmapping::ParticleFilter& filter, double range_m, int min_cells = 8);
  GainInfo lastGain() const;                       ///< tbnav_nav_last_gain
  std::vector<std::uint32_t> frontierGain();       ///< G18, [nx][ny]; 0 where the cell is no seed
  std::vector<FrontierGain> frontierGainList();    ///< G19, one per cluster in ascending label order
  std::vector<std::string> lastGainKernels() const;   ///< the gain's kernels of the last find with gain, as a profiler prints them
  /// findFrontiersGain with events between the stages: microseconds of mark, label, sizes, seeds, gain (a measurement hook).
  std::array<double, 5> profileFindFrontiersGain(bmapping::ParticleFilter& filter, double range_m, int min_cells = 8);
  /// G20: solveToFrontiers with every seed starting at gain_weight * (gain_max - its gain), 0 <= gain_weight <= 4096: a seed that sees
  /// more may be farther by that much.  false where the find left no seed.  Throws std::invalid_argument where the last find had no
  /// gain, the cost grid or the visited mask was set again since, or the weight is out of range.  path() then ends at the seed reached.
  bool solveToFrontiersRanked(int gain_weight);
  std::vector<std::uint32_t> costToGo();          ///< G4, [nx][ny]; 0xFFFFFFFF = blocked or unreached
  std::vector<float> field(double cap);            ///< G5, metres to go capped at `cap`
  /// G6 from the cell of (x, y): (ix, iy) pairs, start and goal included.  Throws std::runtime_error from a blocked or unreached start.
  std::vector<std::array<int, 2>> path(double x, double y);
  /// tbnav_nav_apply_to_mppi(_group): field(cap) becomes the controller's cost field with this grid's geometry and `weight`,
  /// device to device.
  void applyTo(controller::MPPI& mppi, double cap, double weight);

  int nx() const { return nx_; }
  int ny() const { return ny_; }
  int rounds() const;        ///< rounds the last solve took (tbnav_nav_last_solve)

 private:
  std::array<int, 2> cellOf(double x, double y) const;
  tbnav_nav* h_ = nullptr;
  int nx_ = 0, ny_ = 0;
  double xmin_ = 0.0, ymin_ = 0.0, resolution_ = 1.0;
};

}  // namespace planner
#endif

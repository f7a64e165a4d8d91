// planner/goal_field.hpp — planner::GoalField: the exact shortest-path cost-to-go to a goal cell over a cost grid, solved on the
// MI355X through the C-ABI of include/tbnav_nav.h (its sections G1-G6 are the specification), and handed to controller::MPPI as a
// cost field without a host round trip.  Not in the reference: its planner package (planner/include/planner/dstar_light.hpp, D* Lite
// over the 8-connected grid with a move priced by the cell entered, dstar_light.cpp:367-461) is never seen by its controller.  A node
// that owns the filter's distance field does
//     planner::GoalField nav(nx, ny, xmin, ymin, resolution);
//     nav.setCost(planner::navCostFromDistance(occ_dist, nx, ny, r_robot, r_inflate, k));
//     nav.solve(goal.x, goal.y);  nav.applyTo(mppi, cap, weight);
// and one that owns the filter itself replaces the second line by nav.setCostFrom(filter, r_robot, r_inflate, k): the grid comes from
// the best particle's map on the device (G7-G9).
// and links libtbnav_host.so + libtbnav_hip.so.
#ifndef TBNAV_PLANNER_GOAL_FIELD_HPP
#define TBNAV_PLANNER_GOAL_FIELD_HPP

#include <array>
#include <cstdint>
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
  std::vector<std::uint32_t> costToGo();           ///< G4, [nx][ny]; 0xFFFFFFFF = blocked or unreached
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
};

}  // namespace planner
#endif

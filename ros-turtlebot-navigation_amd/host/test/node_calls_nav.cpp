// node_calls_nav.cpp — COMPILE-ONLY translation unit: the calls of a node that owns the filter's distance field, a
// planner::GoalField and the controller — nuturtle_robot/src/mppi_waypoints_node.cpp:186-265 on controller::MPPI (as
// host/test/node_calls.cpp spells them) plus what pulls the robot round what the mapper has drawn: a cost grid derived from the
// distance field, the cost-to-go to the waypoint's cell solved on the device, and its hand-over to the controller without a host
// round trip.  Nothing here runs.
#include <array>
#include <cstdint>
#include <vector>

#include "controller/mppi.hpp"
#include "planner/goal_field.hpp"
#include "rigid2d/diff_drive.hpp"
#include "rigid2d/rigid2d.hpp"
#include "rigid2d/utilities.hpp"

void mppi_waypoints_node_calls_with_goal_field() {
  double wheel_radius = 0.033, wheel_base = 0.16, lambda = 0.01, max_rot_motor = 6.35495, ul_var = 0.9, ur_var = 0.9;
  double horizon = 2.0, time_step = 0.02, ul_init = 0.0, ur_init = 0.0, goal_thresh = 0.05;
  int rollouts = 128;
  // the field carries the pull towards the waypoint: the quadratic loss keeps the heading term only
  std::vector<double> Q{0.0, 0.0, 1.0}, R{0.1, 0.1}, P1{1e3, 1e3, 1e3};
  rigid2d::Pose pose;

  controller::CartModel cart_model(wheel_radius, wheel_base);                                 // :186
  controller::LossFunc loss_func(Q, R, P1);                                                   // :187
  controller::MPPI mppi(cart_model, loss_func, lambda, max_rot_motor, ul_var, ur_var, horizon, time_step, rollouts);  // :188-196
  mppi.setInitialControls(ul_init, ur_init);                                                  // :199

  // the addition: the map's distance field (metres, [nx][ny], x slow) -> a cost grid -> metres to go to the waypoint -> the controller
  const int nx = 80, ny = 80;
  const double map_resolution = 0.05, map_xmin = -1.0, map_ymin = -2.0, r_robot = 0.10, r_inflate = 0.45, k = 8.0, cap = 10.0, weight = 1e4;
  std::vector<double> occ_dist((size_t)nx * ny, 10.0);
  planner::GoalField nav(nx, ny, map_xmin, map_ymin, map_resolution);
  rigid2d::Pose wpt;
  wpt.x = 2.025; wpt.y = 0.025; wpt.theta = 0.0;
  mppi.setWaypoint(wpt);                                                                      // :216, :257
  // ... at every map update, and whenever the waypoint changes:
  nav.setCost(planner::navCostFromDistance(occ_dist, nx, ny, r_robot, r_inflate, k));
  nav.solve(wpt.x, wpt.y);
  nav.applyTo(mppi, cap, weight);
  // a node that wants waypoints instead reads the path
  const std::vector<std::array<int, 2>> cells = nav.path(pose.x, pose.y);
  const std::vector<std::uint32_t> d = nav.costToGo();
  const std::vector<float> metres = nav.field(cap);
  (void)cells.size(); (void)d.size(); (void)metres.size();

  rigid2d::DiffDrive diff_drive(pose, wheel_base, wheel_radius);                              // :205
  const auto d2g = rigid2d::euclideanDistance(wpt.x, wpt.y, pose.x, pose.y);                  // :238
  if (d2g < goal_thresh) mppi.setWaypoint(wpt);
  rigid2d::WheelVelocities wheel_vel = mppi.newControls(pose);                                // :265
  rigid2d::Twist2D cmd = diff_drive.wheelsToTwist(wheel_vel);                                 // :276
  (void)cmd.vx; (void)cmd.w;
  mppi.clearCostField();
}

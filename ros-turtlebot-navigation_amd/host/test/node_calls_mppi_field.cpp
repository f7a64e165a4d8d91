// node_calls_mppi_field.cpp — COMPILE-ONLY translation unit: the calls of nuturtle_robot/src/mppi_waypoints_node.cpp:186-265 on
// controller::MPPI (as host/test/node_calls.cpp spells them) plus what a node adds to avoid what the mapper has drawn: a cost
// field derived from a distance field and handed to the controller.  Nothing here runs.
#include <vector>

#include "controller/mppi.hpp"
#include "rigid2d/diff_drive.hpp"
#include "rigid2d/rigid2d.hpp"
#include "rigid2d/utilities.hpp"

void mppi_waypoints_node_calls_with_cost_field() {
  double wheel_radius = 0.033, wheel_base = 0.16, lambda = 0.01, max_rot_motor = 6.35495, ul_var = 0.9, ur_var = 0.9;
  double horizon = 1.0, time_step = 0.01, ul_init = 0.0, ur_init = 0.0, goal_thresh = 0.05;
  int rollouts = 5;
  std::vector<double> Q{1e4, 1e4, 1.0}, R{0.1, 0.1}, P1{1e3, 1e3, 1e3};
  rigid2d::Pose pose;

  controller::CartModel cart_model(wheel_radius, wheel_base);                                 // :186
  controller::LossFunc loss_func(Q, R, P1);                                                   // :187
  controller::MPPI mppi(cart_model, loss_func, lambda, max_rot_motor, ul_var, ur_var, horizon, time_step, rollouts);  // :188-196
  mppi.setInitialControls(ul_init, ur_init);                                                  // :199

  // the addition: the map's distance field (metres, [nx][ny], x slow) -> an inflated cost -> the controller
  const int nx = 80, ny = 80;
  const double map_resolution = 0.05, map_min = -2.0, r_robot = 0.10, r_inflate = 0.45;
  std::vector<double> occ_dist((size_t)nx * ny, 10.0);
  controller::CostField field;
  field.nx = nx; field.ny = ny; field.xmin = map_min; field.ymin = map_min; field.resolution = map_resolution; field.weight = 2e4;
  field.values = controller::costFieldFromDistance(occ_dist, nx, ny, r_robot, r_inflate);
  mppi.setCostField(field);

  rigid2d::DiffDrive diff_drive(pose, wheel_base, wheel_radius);                              // :205
  rigid2d::Pose wpt;
  wpt.x = 1.0; wpt.y = 0.0; wpt.theta = 1.5707;
  mppi.setWaypoint(wpt);                                                                      // :216, :257
  const auto d2g = rigid2d::euclideanDistance(wpt.x, wpt.y, pose.x, pose.y);                  // :238
  if (d2g < goal_thresh) mppi.setWaypoint(wpt);
  rigid2d::WheelVelocities wheel_vel = mppi.newControls(pose);                                // :265
  rigid2d::Twist2D cmd = diff_drive.wheelsToTwist(wheel_vel);                                 // :276
  (void)cmd.vx; (void)cmd.w;
  mppi.clearCostField();
}

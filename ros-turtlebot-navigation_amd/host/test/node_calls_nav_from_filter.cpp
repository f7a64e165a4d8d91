// node_calls_nav_from_filter.cpp — COMPILE-ONLY translation unit: the calls of a node that owns the filter, a planner::GoalField and
// the controller — bmapping/src/turtle_mapping_node.cpp:389-410, :474 on bmapping::ParticleFilter and
// nuturtle_robot/src/mppi_waypoints_node.cpp:186-265 on controller::MPPI (as host/test/node_calls.cpp spells them) — plus what links
// the three on the device: the planner's cost grid and the controller's inflation field taken from the map of the filter's best
// particle (include/tbnav_nav.h G7-G9).  No distance field is made up, stored or moved.  Nothing here runs.
#include <array>
#include <cstdint>
#include <vector>

#include "bmapping/cloud_alignment.hpp"
#include "bmapping/grid_mapper.hpp"
#include "bmapping/particle_filter.hpp"
#include "bmapping/sensor_model.hpp"
#include "controller/mppi.hpp"
#include "planner/goal_field.hpp"
#include "rigid2d/diff_drive.hpp"
#include "rigid2d/rigid2d.hpp"

void mapping_planning_and_control_node_calls() {
  float beam_min = 0, beam_max = 6.28f, beam_delta = 0.0174f, range_min = 0.12f, range_max = 3.5f;
  double z_hit = 0.95, z_short = 0.0, z_max = 0.04, z_rand = 0.01, sigma_hit = 0.5;
  double map_resolution = 0.05, map_min = -2.0, map_max = 2.0;
  int num_particles = 40, num_samples_mode = 50;
  std::vector<float> scan(360, 1.0f);
  rigid2d::Transform2D robot_pose, Trs;
  bmapping::LaserProperties props(beam_min, beam_max, beam_delta, range_min, range_max, z_hit, z_short, z_max, z_rand, sigma_hit);
  bmapping::GridMapper grid(map_resolution, map_min, map_max, map_min, map_max, props, Trs);
  bmapping::ScanAlignment aligner(props, Trs);
  bmapping::ParticleFilter filter(num_particles, num_samples_mode, 0.1, 0.2, 0.1, 0.2, 1e-10, 1e-10, 1e-10, 1e-10, 1e-8, 1e-8, 1, 20, 1, 10,
                                  aligner, robot_pose, grid);

  double wheel_radius = 0.033, wheel_base = 0.16, lambda = 0.01, max_rot_motor = 6.35495, ul_var = 0.9, ur_var = 0.9;
  double horizon = 2.0, time_step = 0.02;
  int rollouts = 128;
  std::vector<double> Q{0.0, 0.0, 1.0}, R{0.1, 0.1}, P1{1e3, 1e3, 1e3};
  controller::CartModel cart_model(wheel_radius, wheel_base);
  controller::LossFunc loss_func(Q, R, P1);
  controller::MPPI mppi(cart_model, loss_func, lambda, max_rot_motor, ul_var, ur_var, horizon, time_step, rollouts);
  mppi.setInitialControls(0.0, 0.0);

  // the planner's grid is the filter's: the same side, corner and resolution
  const int side = 80;
  const double r_robot = 0.10, r_inflate = 0.45, k = 8.0, cap = 10.0, weight = 1e4;
  planner::GoalField nav(side, side, map_min, map_min, map_resolution);
  rigid2d::Pose pose, cur_odom, prev_odom, wpt;
  wpt.x = 1.025; wpt.y = 0.025; wpt.theta = 0.0;
  mppi.setWaypoint(wpt);

  // ... at every scan:
  rigid2d::Twist2D vb;
  filter.SLAM(scan, vb, cur_odom, prev_odom);
  nav.setCostFrom(filter, r_robot, r_inflate, k);   // the best particle's map -> the cost grid, on the device
  nav.solve(wpt.x, wpt.y);
  nav.applyTo(mppi, cap, weight);                   // metres to go round the walls -> the controller
  const std::vector<std::array<int, 2>> cells = nav.path(pose.x, pose.y);
  (void)cells.size();
  rigid2d::WheelVelocities wheel_vel = mppi.newControls(pose);
  (void)wheel_vel;

  // a node without a planner keeps the walls away with the inflation field of the same map
  mppi.setCostFieldFrom(filter, r_robot, r_inflate, 2e4);
  wheel_vel = mppi.newControls(pose);
  mppi.clearCostField();
}

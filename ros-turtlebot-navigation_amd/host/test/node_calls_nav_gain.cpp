// node_calls_nav_gain.cpp — COMPILE-ONLY translation unit: the loop of a node that EXPLORES and RANKS its frontiers.  It owns the
// filter, a planner::GoalField and the controller as host/test/node_calls_nav_frontier.cpp does; where that node drives to the NEAREST
// seed, this one asks of every seed what a scan from it would reveal (include/tbnav_nav.h G17-G19) and lets a seed that sees more be
// farther by gain_weight per cell (G20).  Nothing here runs.
#include <array>
#include <cmath>
#include <string>
#include <vector>

#include "bmapping/cloud_alignment.hpp"
#include "bmapping/grid_mapper.hpp"
#include "bmapping/particle_filter.hpp"
#include "bmapping/sensor_model.hpp"
#include "controller/mppi.hpp"
#include "planner/goal_field.hpp"
#include "rigid2d/diff_drive.hpp"
#include "rigid2d/rigid2d.hpp"

void ranking_node_calls() {
  float beam_min = 0, beam_max = 6.28f, beam_delta = 0.0174f, range_min = 0.12f, range_max = 3.5f;
  double z_hit = 0.95, z_short = 0.0, z_max = 0.04, z_rand = 0.01, sigma_hit = 0.5;
  double map_resolution = 0.05, map_min = -4.0, map_max = 4.0;
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
  const int side = 160, min_cells = 8, gain_weight = 2;
  const double r_robot = 0.10, r_inflate = 0.45, k = 8.0, cap = 10.0, weight = 1e4, arrived = 0.15, mark_radius = 0.5;
  const double gain_range = 2.0;   // metres: 40 cells, a little over half the scanner's range
  planner::GoalField nav(side, side, map_min, map_min, map_resolution);
  rigid2d::Pose pose, cur_odom, prev_odom;

  // ... at every scan:
  rigid2d::Twist2D vb;
  bool exploring = true;
  while (exploring) {
    filter.SLAM(scan, vb, cur_odom, prev_odom);
    nav.setCostFrom(filter, r_robot, r_inflate, k);                          // the best particle's map -> the cost grid
    const std::vector<planner::FrontierGain> gains = nav.findFrontiersGain(filter, gain_range, min_cells);   // ... -> its frontiers, and what each seed would see
    const planner::GainInfo gi = nav.lastGain();
    (void)gains.size(); (void)gi.gain_max;
    exploring = nav.solveToFrontiersRanked(gain_weight);                     // a seed that sees more may be farther
    if (!exploring) break;                                                   // nothing left to explore
    nav.applyTo(mppi, cap, weight);
    const std::vector<std::array<int, 2>> cells = nav.path(pose.x, pose.y);  // ends at the seed reached
    if ((double)cells.size() * map_resolution < arrived) nav.markVisited(pose.x, pose.y, mark_radius);   // on a frontier the scans do not clear
    rigid2d::WheelVelocities wheel_vel = mppi.newControls(pose);
    (void)wheel_vel;
  }
  // for people: the gain of every cell, the kernels that formed it, and the stages' times
  const std::vector<std::uint32_t> gain = nav.frontierGain();
  const std::vector<planner::FrontierGain> list = nav.frontierGainList();
  const std::vector<std::string> kernels = nav.lastGainKernels();
  const std::array<double, 5> us = nav.profileFindFrontiersGain(filter, gain_range, min_cells);
  (void)gain.size(); (void)list.size(); (void)kernels.size(); (void)us[4];
}

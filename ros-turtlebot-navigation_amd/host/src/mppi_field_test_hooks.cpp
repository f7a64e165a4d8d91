// mppi_field_test_hooks.cpp — extern "C" access for tests/ to what controller::MPPI gained with the cost field (include/tbnav_mppi.h,
// COST FIELD): the host function that derives a field from distances (no GPU needed), ticks through the class with a field set and
// the host twister seeded, and a closed loop round an obstacle.  Same conventions as test_hooks.cpp; not part of the product surface.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <exception>
#include <stdexcept>
#include <string>
#include <vector>

#include "controller/mppi.hpp"
#include "rigid2d/utilities.hpp"

namespace {
std::string g_field_err;
// params = (wheel_radius, wheel_base, lambda, max_wheel_vel, ul_var, ur_var, horizon, dt, Q0..2, R0..1, P0..2) as in test_hooks.cpp;
// geom = (xmin, ymin, resolution, weight)
controller::MPPI make(const double* params, int rollouts, int n_gpus) {
  controller::CartModel cart(params[0], params[1]);
  controller::LossFunc loss({params[8], params[9], params[10]}, {params[11], params[12]}, {params[13], params[14], params[15]});
  return controller::MPPI(cart, loss, params[2], params[3], params[4], params[5], params[6], params[7], rollouts, n_gpus,
                          std::vector<int>(n_gpus > 1 ? n_gpus : 0, 0));
}
controller::CostField field_of(int nx, int ny, const double geom[4], const float* values) {
  controller::CostField f;
  f.nx = nx; f.ny = ny; f.xmin = geom[0]; f.ymin = geom[1]; f.resolution = geom[2]; f.weight = geom[3];
  f.values.assign(values, values + (size_t)nx * ny);
  return f;
}
}  // namespace

extern "C" {

const char* hst_field_last_error() { return g_field_err.c_str(); }

// controller::costFieldFromDistance; 0 = ok, 1 = it threw std::invalid_argument, 2 = anything else
int hst_cost_field_from_distance(const double* dist, int nx, int ny, double r_robot, double r_inflate, float* out) {
  try {
    const std::vector<float> c = controller::costFieldFromDistance(std::vector<double>(dist, dist + (size_t)nx * ny), nx, ny, r_robot, r_inflate);
    std::memcpy(out, c.data(), sizeof(float) * c.size());
    return 0;
  } catch (const std::invalid_argument& e) { g_field_err = e.what(); return 1; }
  catch (const std::exception& e) { g_field_err = e.what(); return 2; }
}

// n_ticks through the class (n_gpus members on device 0 when > 1) with a field set and the host twister seeded: (ul, ur) per tick
// and u[2][T].  Returns T; -1 on an exception; -2 when setCostField threw std::invalid_argument (no tick is run then).
int hst_mppi_field_tick(const double* params, int rollouts, int n_gpus, uint64_t seed, const double wpt[3] /*x,y,theta*/,
                        const double x0[3] /*x,y,theta*/, const double uinit[2], int nx, int ny, const double geom[4], const float* values,
                        int n_ticks, double* out_ul_ur, double* u_out) {
  try {
    controller::MPPI mppi = make(params, rollouts, n_gpus);
    try { mppi.setCostField(field_of(nx, ny, geom, values)); }
    catch (const std::invalid_argument& e) { g_field_err = e.what(); return -2; }
    rigid2d::getTwister().seed(seed);
    mppi.setInitialControls(uinit[0], uinit[1]);
    rigid2d::Pose w; w.x = wpt[0]; w.y = wpt[1]; w.theta = wpt[2];
    mppi.setWaypoint(w);
    rigid2d::Pose ps; ps.x = x0[0]; ps.y = x0[1]; ps.theta = x0[2];
    for (int t = 0; t < n_ticks; ++t) {
      const auto u = mppi.newControls(ps);
      out_ul_ur[2 * t] = u.ul; out_ul_ur[2 * t + 1] = u.ur;
    }
    const auto uu = mppi.controls();
    std::memcpy(u_out, uu.data(), sizeof(double) * uu.size());
    return mppi.steps();
  } catch (const std::exception& e) { g_field_err = e.what(); return -1; }
}

// Closed loop from (0, 0, 0) to `goal` with the field set (with_field != 0) or not: newControls (host twister) -> one plant step of
// the exact-arc model, DiffDrive::feedforward(wheelsToTwist(u) * dt), until the robot is within goal_thresh.  least_clearance: the
// least distance to the surface of the disc (cx, cy, radius).  Returns the ticks used, max_ticks + 1 if it never arrived, -1 on an
// exception.
int hst_mppi_field_closed_loop(const double* params, int rollouts, uint64_t seed, const double goal[3], double goal_thresh, int max_ticks,
                               int with_field, int nx, int ny, const double geom[4], const float* values, const double disc[3],
                               double* least_clearance) {
  try {
    controller::MPPI mppi = make(params, rollouts, 1);
    if (with_field) mppi.setCostField(field_of(nx, ny, geom, values));
    rigid2d::getTwister().seed(seed);
    mppi.setInitialControls(0.0, 0.0);
    rigid2d::Pose w; w.x = goal[0]; w.y = goal[1]; w.theta = goal[2];
    mppi.setWaypoint(w);
    rigid2d::Pose start;
    rigid2d::DiffDrive plant(start, params[1], params[0]);
    double least = 1e300;
    for (int tick = 1; tick <= max_ticks; ++tick) {
      const rigid2d::WheelVelocities u = mppi.newControls(plant.pose());
      rigid2d::Twist2D cmd = plant.wheelsToTwist(u);
      cmd.w *= params[7]; cmd.vx *= params[7]; cmd.vy = 0.0;
      plant.feedforward(cmd);
      const rigid2d::Pose p = plant.pose();
      least = std::fmin(least, std::hypot(p.x - disc[0], p.y - disc[1]) - disc[2]);
      if (std::hypot(p.x - goal[0], p.y - goal[1]) < goal_thresh) { *least_clearance = least; return tick; }
    }
    *least_clearance = least;
    return max_ticks + 1;
  } catch (const std::exception& e) { g_field_err = e.what(); return -1; }
}

}  // extern "C"

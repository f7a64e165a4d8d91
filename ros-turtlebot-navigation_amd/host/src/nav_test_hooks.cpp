// nav_test_hooks.cpp — extern "C" access for tests/ to planner::GoalField (host/include/planner/goal_field.hpp): the host function
// that derives a cost grid from distances (no GPU needed) and one solve with its path through the class.  Same conventions as
// mppi_field_test_hooks.cpp; not part of the product surface.
#include <cstdint>
#include <cstring>
#include <exception>
#include <stdexcept>
#include <string>
#include <vector>

#include "planner/goal_field.hpp"

namespace {
std::string g_nav_err;
}

extern "C" {

const char* hst_nav_last_error() { return g_nav_err.c_str(); }

// planner::navCostFromDistance; 0 = ok, 1 = it threw std::invalid_argument, 2 = anything else
int hst_nav_cost_from_distance(const double* dist, int nx, int ny, double r_robot, double r_inflate, double k, uint8_t* out) {
  try {
    const std::vector<uint8_t> c = planner::navCostFromDistance(std::vector<double>(dist, dist + (size_t)nx * ny), nx, ny, r_robot, r_inflate, k);
    std::memcpy(out, c.data(), c.size());
    return 0;
  } catch (const std::invalid_argument& e) { g_nav_err = e.what(); return 1; }
  catch (const std::exception& e) { g_nav_err = e.what(); return 2; }
}

// GoalField(nx, ny, geom = (xmin, ymin, resolution)); setCost; solve(goal_xy); costToGo -> d_out[nx*ny]; field(cap) -> field_out;
// path(start_xy) -> path_out[path_cap][2], *path_len = its length (copied up to path_cap).  Returns the solve's rounds (> 0);
// -1 on an exception; -2 on std::invalid_argument.
int hst_nav_solve(int nx, int ny, const double geom[3], const uint8_t* cost, const double goal_xy[2], const double start_xy[2], double cap,
                  uint32_t* d_out, float* field_out, int32_t* path_out, int path_cap, int* path_len) {
  try {
    planner::GoalField nav(nx, ny, geom[0], geom[1], geom[2]);
    nav.setCost(std::vector<uint8_t>(cost, cost + (size_t)nx * ny));
    nav.solve(goal_xy[0], goal_xy[1]);
    const auto d = nav.costToGo();
    std::memcpy(d_out, d.data(), sizeof(uint32_t) * d.size());
    const auto f = nav.field(cap);
    std::memcpy(field_out, f.data(), sizeof(float) * f.size());
    const auto p = nav.path(start_xy[0], start_xy[1]);
    *path_len = (int)p.size();
    for (int i = 0; i < (int)p.size() && i < path_cap; ++i) { path_out[2 * i] = p[i][0]; path_out[2 * i + 1] = p[i][1]; }
    return nav.rounds();
  } catch (const std::invalid_argument& e) { g_nav_err = e.what(); return -2; }
  catch (const std::exception& e) { g_nav_err = e.what(); return -1; }
}

}  // extern "C"

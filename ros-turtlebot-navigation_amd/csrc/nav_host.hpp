// nav_host.hpp — the goal field's handle and what its two host files share (nav.hip: create / solve / results / hand-over of the solved
// field; nav_from_map.hip: the cost grid taken from a filter's occupancy bits on the device, tbnav_nav.h G7-G9).
#ifndef TBNAV_NAV_HOST_HPP
#define TBNAV_NAV_HOST_HPP
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "tbnav_nav.h"

struct tbnav_nav {
  tbnav_nav_params p;
  int device = 0, n = 0, tiles_x = 0, tiles_y = 0;
  double inv = 0.0;                 // 1.0 / resolution (G1)
  uint8_t* d_cost = nullptr;        // [nx][ny] what the next solve uses
  uint8_t* d_cost_solved = nullptr; // [nx][ny] what the last solve used, where that grid was set on the device (cost_solved is fetched from here)
  uint8_t* d_infl = nullptr;        // [kInflBytes] G7's cost table of the last tbnav_nav_set_cost_from_rbpf
  unsigned* d_d = nullptr;          // [nx][ny] the last solve's cost-to-go
  float* d_field = nullptr;         // [nx][ny] G5 of the last get_field / apply
  unsigned* d_flags = nullptr;      // [2][tiles] active tiles of even and odd rounds
  unsigned* d_rec = nullptr;        // [batch][2] a batch's round records
  // host copies: the grid set last, and the one the last solve used (G6 walks over it).  A grid set on the device leaves them behind:
  // each is fetched at its first use (cost_host_valid / cost_solved_valid), never at the set.
  std::vector<uint8_t> cost, cost_solved;
  std::vector<uint8_t> infl;        // host side of d_infl (alive while the copy is in flight)
  std::vector<unsigned> d_host;     // the downloaded cost-to-go (filled at its first use after a solve)
  bool cost_set = false, solved = false, d_host_valid = false, cost_host_valid = false, cost_solved_valid = false;
  bool from_map = false;            // tbnav_nav_set_cost_from_rbpf has run on this handle (tbnav_nav_last_cost_kernel)
  tbnav_nav_solve_info info{0, {0, 0}, 0, 0, {0, 0}, 0};
};

namespace tbnav_nk {
// room for a table of TBNAV_NAV_MAX_REACH^2 + 1 entries and the open value
constexpr int kInflEntries = TBNAV_NAV_MAX_REACH * TBNAV_NAV_MAX_REACH + 2;
}  // namespace tbnav_nk

#endif

// rbpf_plan_check — csrc/rbpf_plan.hpp (what the host decides before it launches an RBPF kernel) as a stand-alone program: one input
// tuple per line on stdin, the plan on stdout.  tests/test_rbpf_plan.py compiles it with g++ alone — no HIP, no library — and holds
// every answer against the Python restatements (tests/raycast_cases.py, propose_cases.py, scanmatch_cases.py) with `==`.
//   R range_max ordered resolution trs_x trs_y rmax Bv need THREADS ADAPT CELL16 BAND_ROWS ref_field
//       -> tile_cap threads wps c16 ev cap_win lds hash_words need        (threads 0: the beam-ordered kernel)
//   P k Bv df_mode xsize words range_max spread resolution  -> occ_half slice_bytes lds sm_lds threads fits
//   S sr_theta sr_x sr_y mn_theta mn_x mn_y                   -> sampling_spread, 17 significant digits
//   H range_max trs_x trs_y ticp_x ticp_y u_vx spread matcher_travel resolution whole_map xsize  -> lookup_half_cells
//   E xsize words                                             -> edt_cols_for
#include <cstdio>

#include "rbpf_plan.hpp"

using namespace tbnav_rk;

int main() {
  char line[512];
  long n = 0;
  while (std::fgets(line, sizeof line, stdin)) {
    ++n;
    if (line[0] == 'R') {
      double range_max, res, tx, ty, rmax;
      int ordered, Bv, need, threads, adapt, cell16, band_rows, ref_field;
      if (std::sscanf(line + 1, "%lf %d %lf %lf %lf %lf %d %d %d %d %d %d %d", &range_max, &ordered, &res, &tx, &ty, &rmax, &Bv, &need, &threads,
                      &adapt, &cell16, &band_rows, &ref_field) != 13) { std::fprintf(stderr, "line %ld: bad R tuple\n", n); return 2; }
      const double Trs[3] = {0.0, tx, ty};
      const int tile_cap = ordered ? 0 : tile_cap_for(range_max, Trs, res);
      const RaycastPlan p = plan_raycast(RaycastIn{tile_cap, res, {0.0, tx, ty}, rmax, Bv, threads, adapt, cell16, band_rows, need, ref_field != 0});
      std::printf("%d %d %d %d %d %ld %zu %d %d\n", tile_cap, p.threads, p.wps, p.c16 ? 1 : 0, p.ev, p.cap_win, p.lds, p.hash_words, p.need);
    } else if (line[0] == 'P') {
      ProposeIn in{};
      if (std::sscanf(line + 1, "%d %d %d %d %d %lf %lf %lf", &in.k, &in.Bv, &in.df_mode, &in.xsize, &in.words, &in.range_max, &in.spread,
                      &in.resolution) != 8) { std::fprintf(stderr, "line %ld: bad P tuple\n", n); return 2; }
      const ProposePlan p = plan_propose(in);
      std::printf("%d %zu %zu %zu %d %d\n", p.occ_half, p.slice_bytes, p.lds, p.sm_lds, p.threads, p.fits ? 1 : 0);
    } else if (line[0] == 'S') {
      double sr[3], mn[3];
      if (std::sscanf(line + 1, "%lf %lf %lf %lf %lf %lf", sr, sr + 1, sr + 2, mn, mn + 1, mn + 2) != 6) { std::fprintf(stderr, "line %ld: bad S tuple\n", n); return 2; }
      std::printf("%.17g\n", sampling_spread(sr, mn));
    } else if (line[0] == 'H') {
      double range_max, tx, ty, ix, iy, uvx, spread, travel, res;
      int whole, xsize;
      if (std::sscanf(line + 1, "%lf %lf %lf %lf %lf %lf %lf %lf %lf %d %d", &range_max, &tx, &ty, &ix, &iy, &uvx, &spread, &travel, &res, &whole,
                      &xsize) != 11) { std::fprintf(stderr, "line %ld: bad H tuple\n", n); return 2; }
      const double Trs[3] = {0.0, tx, ty}, T_icp[3] = {0.0, ix, iy}, u[3] = {0.0, uvx, 0.0};
      std::printf("%d\n", lookup_half_cells(range_max, Trs, T_icp, u, spread, travel, res, whole != 0, xsize));
    } else if (line[0] == 'E') {
      int xsize, words;
      if (std::sscanf(line + 1, "%d %d", &xsize, &words) != 2) { std::fprintf(stderr, "line %ld: bad E tuple\n", n); return 2; }
      std::printf("%d\n", edt_cols_for(xsize, words));
    } else if (line[0] != '\n' && line[0] != '#') {
      std::fprintf(stderr, "line %ld: unknown tuple\n", n);
      return 2;
    }
  }
  return 0;
}

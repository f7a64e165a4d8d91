// mppi_plan_check — csrc/mppi_plan.hpp (what the host decides before it launches an MPPI kernel) as a stand-alone program: one input
// tuple per line on stdin, the plan on stdout.  tests/test_mppi_plan.py compiles it with g++ alone — no HIP, no library — and holds
// every answer against the Python restatements (tests/mppi_cases.py) with `==`.  A kernel name comes last on its line (it has blanks);
// `listed` says whether the form is in its family's list (mppi_plan.hpp: TBNAV_MPPI_*_FORMS), i.e. whether a launcher would find it.
//   C K T cus                                          -> S lds_from prefix_rg scan_tc fused_dev fused_rng fused_r fused_S
//   O T K value                                        -> ok scan_tc fused_r fused_S fused_dev fused_rng
//   Q fused_rng fused_r K n_ticks                      -> rng_in_kernel ahead_wanted graph_worth_it
//   R T K dyn trig scan_tc prefix_rg lds_from field_on -> grid block_y lds lds_from prefix_rows listed name
//   F T K dyn trig sampler fused_r fused_S rng         -> grid block lds listed name
//   M T K G S direct err_words wide_on ahead           -> tpr_log2 blocks ahead_blocks grid block listed name
//   L                                                  -> every form of every list by name, separated by ';'
#include <cstdio>

#include "mppi_plan.hpp"

using namespace tbnav_mk;

static const char* name_of(const KernelForm& f) {
  static char buf[96];
  form_name(f, buf, sizeof buf);
  return buf;
}

int main() {
  char line[256];
  long n = 0;
  while (std::fgets(line, sizeof line, stdin)) {
    ++n;
    int v[8];
    const int got = std::sscanf(line + 1, "%d %d %d %d %d %d %d %d", v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7);
    auto bad = [&](int want) { if (got != want) std::fprintf(stderr, "line %ld: bad %c tuple\n", n, line[0]); return got != want; };
    if (line[0] == 'C') {
      if (bad(3)) return 2;
      const CreatePlan p = plan_create(v[0], v[1], v[2]);
      std::printf("%d %d %d %d %d %d %d %d\n", p.S, p.lds_from, p.prefix_rg, p.scan_tc, p.fused_dev ? 1 : 0, p.fused_rng ? 1 : 0, p.fused_r, p.fused_S);
    } else if (line[0] == 'O') {
      if (bad(3)) return 2;
      const KernelOption o = plan_kernel_option(v[0], v[1], v[2]);
      std::printf("%d %d %d %d %d %d\n", o.ok ? 1 : 0, o.scan_tc, o.fused_r, o.fused_S, o.fused_dev ? 1 : 0, o.fused_rng ? 1 : 0);
    } else if (line[0] == 'Q') {
      if (bad(4)) return 2;
      const bool in_kernel = rng_in_kernel(v[0] != 0, v[1]);
      std::printf("%d %d %d\n", in_kernel ? 1 : 0, ahead_wanted(v[0] != 0, v[1]) ? 1 : 0, graph_worth_it(in_kernel, v[1], v[2], v[3]) ? 1 : 0);
    } else if (line[0] == 'R') {
      if (bad(8)) return 2;
      const RolloutPlan p = plan_rollout(RolloutIn{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7] != 0});
      std::printf("%d %d %zu %d %d %d %s\n", p.grid, p.block_y, p.lds, p.lds_from, p.prefix_rows, form_listed(p.form) ? 1 : 0, name_of(p.form));
    } else if (line[0] == 'F') {
      if (bad(8)) return 2;
      const FusedPlan p = plan_fused(FusedIn{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7] != 0});
      std::printf("%d %d %zu %d %s\n", p.grid, p.block, p.lds, form_listed(p.form) ? 1 : 0, name_of(p.form));
    } else if (line[0] == 'M') {
      if (bad(8)) return 2;
      const CombinePlan p = plan_combine(v[0], v[1], v[2], v[3], v[4] != 0, v[5] != 0, v[6] != 0, v[7] != 0);
      std::printf("%d %d %d %d %d %d %s\n", p.tpr_log2, p.blocks, p.ahead_blocks, p.grid, p.block, form_listed(p.form) ? 1 : 0, name_of(p.form));
    } else if (line[0] == 'L') {
#define TBNAV_X(...) std::printf("%s;", name_of(form_of(fam, nargs, __VA_ARGS__)));
      int fam = kFused, nargs = 4;     TBNAV_MPPI_FUSED_FORMS(TBNAV_X)
      fam = kScan; nargs = 3;          TBNAV_MPPI_SCAN_FORMS(TBNAV_X)
      fam = kPrefix; nargs = 1;        TBNAV_MPPI_PREFIX_FORMS(TBNAV_X)
      fam = kCost;                     TBNAV_MPPI_COST_FORMS(TBNAV_X)
      fam = kField;                    TBNAV_MPPI_FIELD_FORMS(TBNAV_X)
      fam = kCombine; nargs = 2;       TBNAV_MPPI_COMBINE_FORMS(TBNAV_X)
#undef TBNAV_X
      std::printf("%s\n", name_of(form_of(kCombineWide)));
    } else if (line[0] != '\n' && line[0] != '#') {
      std::fprintf(stderr, "line %ld: unknown tuple\n", n);
      return 2;
    }
  }
  return 0;
}

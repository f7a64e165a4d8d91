// mppi_plan.hpp — what the host DECIDES before it launches an MPPI kernel, as plain arithmetic: the sizes the kernels and the selection
// share, which kernel a (K, T) takes on a chip of so many CUs (plan_create), what a forced TBNAV_MPPI_OPT_KERNEL value turns that into
// (plan_kernel_option), and which instantiation a tick launches with what grid, block and LDS (plan_rollout, plan_fused, plan_combine).
// One X-macro list of forms per template family: the explicit instantiations (mppi_rollout.hip, mppi_softmin.hip, mppi_field.hip),
// the launchers' dispatch and the LDS attributes are all made from it.  No HIP runtime call and no handle type: g++ -std=c++17
// compiles this header alone, and tests/mppi_plan_check.cpp holds it against the Python restatements (tests/mppi_cases.py) without a
// GPU.  mppi_device.hpp includes it for the kernels; mppi.hip / mppi_field.hip fill the inputs from the handle and launch what comes back.
#ifndef TBNAV_MPPI_PLAN_HPP
#define TBNAV_MPPI_PLAN_HPP
#include <cstddef>
#include <cstdio>
#include <initializer_list>

namespace tbnav_mk {

constexpr int kWave = 64;
constexpr int kSliceThreads = 256;
constexpr int kSliceItems = 8;
constexpr int kSlice = kSliceThreads * kSliceItems;  // rollouts per K-slice record
constexpr int kMaxLdsBytes = 160 * 1024;
constexpr int kGroup = 4;        // steps per group of the one-lane-per-rollout kernels (independent trig chains)
constexpr int kRoundGroups = 3;  // groups per round of mppi_rollout_prefix
#ifndef TBNAV_AHEAD_PAIRS
#define TBNAV_AHEAD_PAIRS 1  // noise pairs per lane of the combine's sampler blocks (TBNAV_MPPI_OPT_NOISE_AHEAD; 1, 2, 4 measured: docs/lab_notebook.md)
#endif
#ifndef TBNAV_COMBINE_WAVES
#define TBNAV_COMBINE_WAVES 1  // one wave per workgroup: the groups spread over as many CUs as there are time steps (K = 1024 tick 8.9 -> 8.4 us against four waves)
#endif

// ---- the forms: every instantiation of every template family, X(template arguments), in the order they are instantiated ------------------
#define TBNAV_MPPI_COST_FORMS(X) X(1) X(2) X(3) X(4)      // mppi_rollout_cost<TRIG>
#define TBNAV_MPPI_PREFIX_FORMS(X) X(1) X(2) X(3)         // mppi_rollout_prefix<RG>
// mppi_rollout_scan<TRIG, TC, MAXW>  (TRIG 2 — a fresh sincos every step — is an A-B setting of the sequential / fused kernels; here
// it takes the three-evaluation form: its eleven instantiations spilled up to 1.2 KB per lane and nothing selected them)
#define TBNAV_MPPI_SCAN_FORMS_TR(X, TR) \
  X(TR, 4, 16) X(TR, 4, 12) X(TR, 5, 12) X(TR, 6, 12) X(TR, 7, 16) X(TR, 8, 16) X(TR, 8, 12) X(TR, 10, 12) X(TR, 12, 12) X(TR, 16, 12) X(TR, 20, 12)
#define TBNAV_MPPI_SCAN_FORMS(X) TBNAV_MPPI_SCAN_FORMS_TR(X, 1) TBNAV_MPPI_SCAN_FORMS_TR(X, 3)
// mppi_rollout_fused<TRIG, R, TL, RNG>: resident noise with 4, 8, 16 rollouts per workgroup, the fp32 sampler with 8 and 16; then
// the fp64 sampler (round 6: the handle's default, TBNAV_MPPI_OPT_SAMPLER = 1) in every dynamics' kernel
#define TBNAV_MPPI_FUSED_FORMS_TL(X, TR, RR, RG) X(TR, RR, 1, RG) X(TR, RR, 2, RG)
#define TBNAV_MPPI_FUSED_FORMS_TR(X, TR)                                                                              \
  TBNAV_MPPI_FUSED_FORMS_TL(X, TR, 4, 0) TBNAV_MPPI_FUSED_FORMS_TL(X, TR, 8, 0) TBNAV_MPPI_FUSED_FORMS_TL(X, TR, 16, 0) \
  TBNAV_MPPI_FUSED_FORMS_TL(X, TR, 8, 1) TBNAV_MPPI_FUSED_FORMS_TL(X, TR, 16, 1)
#define TBNAV_MPPI_FUSED_FORMS(X)                                                                                     \
  TBNAV_MPPI_FUSED_FORMS_TR(X, 2) TBNAV_MPPI_FUSED_FORMS_TR(X, 3) TBNAV_MPPI_FUSED_FORMS_TR(X, 4)                     \
  TBNAV_MPPI_FUSED_FORMS_TL(X, 2, 8, 2) TBNAV_MPPI_FUSED_FORMS_TL(X, 2, 16, 2) TBNAV_MPPI_FUSED_FORMS_TL(X, 3, 8, 2)  \
  TBNAV_MPPI_FUSED_FORMS_TL(X, 3, 16, 2) TBNAV_MPPI_FUSED_FORMS_TL(X, 4, 8, 2) TBNAV_MPPI_FUSED_FORMS_TL(X, 4, 16, 2)
// mppi_rollout_field<TRIG>  (TRIG 2 takes the three-evaluation form here, as in the time-parallel kernel)
#define TBNAV_MPPI_FIELD_FORMS(X) X(1) X(3) X(4)
// mppi_combine<KEEP, MODE>  (MODE 0: one group of records, every single-GPU tick; 1: records of several ranks through an all-gather; 2: the direct exchange)
#define TBNAV_MPPI_COMBINE_FORMS(X) X(2, 0) X(4, 0) X(8, 0) X(2, 1) X(4, 1) X(8, 1) X(2, 2) X(4, 2) X(8, 2)

enum Family { kNoKernel = 0, kFused, kScan, kPrefix, kCost, kField, kCombine, kCombineWide };
// A kernel family and its template arguments (n of them): what a plan names, a launcher dispatches on and the handle remembers
struct KernelForm {
  int family = kNoKernel, n = 0, arg[4] = {0, 0, 0, 0};
  bool is(int fam, int a0, int a1 = 0, int a2 = 0, int a3 = 0) const { return family == fam && arg[0] == a0 && arg[1] == a1 && arg[2] == a2 && arg[3] == a3; }
};
inline KernelForm form_of(int family, int n = 0, int a0 = 0, int a1 = 0, int a2 = 0, int a3 = 0) { return KernelForm{family, n, {a0, a1, a2, a3}}; }
// is the form one of its family's list?  (A launcher answers TBNAV_ERR_UNSUPPORTED to one that is not; no plan below names one.)
inline bool form_listed(const KernelForm& f) {
#define TBNAV_X(...) || f.is(fam, __VA_ARGS__)
  int fam = kFused;  if (f.family == fam) return false TBNAV_MPPI_FUSED_FORMS(TBNAV_X);
  fam = kScan;       if (f.family == fam) return false TBNAV_MPPI_SCAN_FORMS(TBNAV_X);
  fam = kPrefix;     if (f.family == fam) return false TBNAV_MPPI_PREFIX_FORMS(TBNAV_X);
  fam = kCost;       if (f.family == fam) return false TBNAV_MPPI_COST_FORMS(TBNAV_X);
  fam = kField;      if (f.family == fam) return false TBNAV_MPPI_FIELD_FORMS(TBNAV_X);
  fam = kCombine;    if (f.family == fam) return false TBNAV_MPPI_COMBINE_FORMS(TBNAV_X);
#undef TBNAV_X
  return f.family == kCombineWide;
}
// the instantiation as the profiler spells it (tbnav_mppi_last_kernel_names); "" for nothing launched yet
inline void form_name(const KernelForm& f, char* out, size_t cap) {
  static const char* const names[] = {"", "mppi_rollout_fused", "mppi_rollout_scan", "mppi_rollout_prefix", "mppi_rollout_cost", "mppi_rollout_field",
                                      "mppi_combine", "mppi_combine_wide"};
  if (!out || cap == 0) return;
  const int fam = f.family >= kNoKernel && f.family <= kCombineWide ? f.family : kNoKernel;
  int at = std::snprintf(out, cap, "%s", names[fam]);
  for (int q = 0; q < f.n && q < 4 && at >= 0 && (size_t)at < cap; ++q)
    at += std::snprintf(out + at, cap - (size_t)at, "%s%d%s", q ? ", " : "<", f.arg[q], q + 1 == f.n ? ">" : "");
}

// ---- sizes --------------------------------------------------------------------------------------------------------------------------------
constexpr int ceil_div(int a, int b) { return (a + b - 1) / b; }
// dynamic LDS of the one-lane-per-rollout kernels (mppi_rollout_cost, mppi_rollout_field): u_lds [2*T], then the losses of steps lds_from .. T-1, [T - lds_from][64]
constexpr size_t staged_lds_bytes(int T, int lds_from) { return (size_t)2 * T * sizeof(double) + (size_t)(T - lds_from) * kWave * sizeof(double); }
constexpr size_t fused_lds_bytes(int T, int R) { return (size_t)3 * T * (R + 1) * sizeof(double); }

// ---- create: which kernel a (K, T) takes on a chip of `cus` CUs -----------------------------------------------------------------------------
struct CreatePlan {
  int S = 0;          // K-slice records per time step
  int lds_from = 0;   // first time step whose loss is staged in LDS (0 = all of them)
  int prefix_rg = 0;  // > 0: mppi_rollout_prefix with this late region (groups)
  int scan_tc = 0;    // steps per thread of the time-parallel kernel (0 = sequential kernel)
  bool fused_dev = false, fused_rng = false;   // resident-noise / device-noise ticks take the fused kernel
  int fused_r = 0, fused_S = 0;                // its rollouts per workgroup and records per time step
};
inline CreatePlan plan_create(int K, int T, int cus) {
  CreatePlan p;
  p.S = ceil_div(K, kSlice);
  const long waves = ceil_div(K, kWave);   // one-wave workgroups of the one-lane-per-rollout kernels
  // How many steps' losses fit in LDS while the whole grid stays resident in ONE round:
  // blocks per CU needed = ceil(blocks / CUs) (at most 8 considered), LDS budget per block = 160 KB / that.
  long per_cu = (waves + cus - 1) / cus;
  per_cu = per_cu < 1 ? 1 : (per_cu > 8 ? 8 : per_cu);
  const long budget = (long)kMaxLdsBytes / per_cu - 512 - (long)(2 * T * sizeof(double));
  long steps_in_lds = budget > 0 ? budget / (long)(kWave * sizeof(double)) : 0;
  if (steps_in_lds > T) steps_in_lds = T;
  p.lds_from = T - (int)steps_in_lds;
  p.lds_from = ((p.lds_from + 3) / 4) * 4;  // whole groups of 4 steps switch staging together
  if (p.lds_from > T) p.lds_from = T;
  // round 3: the prefix-form kernel takes the streaming shape whenever a late region of 1, 2 or 3 groups leaves whole rounds
  // of three groups (one of the three always does) and at least one round — whatever T: it stages nothing in LDS
  if (T % 4 == 0 && waves >= 2 * cus)
    for (int rg : {1, 2, 3}) if ((T / 4 - rg) % kRoundGroups == 0 && T / 4 - rg >= kRoundGroups) { p.prefix_rg = rg; break; }
  // time-parallel kernel: up to 16 chunks (waves) per workgroup
  for (int tc : {4, 5, 6, 8, 10, 12, 16, 20})
    if (ceil_div(T, tc) <= 12) { p.scan_tc = tc; break; }
  // The time-parallel kernel exists to create waves when the rollout count alone cannot fill the chip;
  // once K/64 one-wave workgroups cover >= 2 waves per CU-SIMD pair the sequential kernel (fewer
  // registers, no chunk barriers) is faster (measured on MI355X: K=65536,T=100 87 us vs 121 us;
  // K=1024,T=50 32 us vs 11 us).
  // Measured on MI355X (tools/mppi_size_sweep.py, T = 25 / 50 / 100, tick in us, resident noise):
  //   K        fused<8>      time-parallel     sequential
  //   2048     11.3          15.2              29.4            (T = 50)
  //   4096     20.1          20.5              49.2            (T = 100)
  //   8192     32.9          23.6              52.1
  //   16384    54.6          29.3              56.1
  //   32768    100           47.1              55.1
  //   49152    -             66.2              62.1
  //   65536    165 (T = 50)  86.6              76.1
  // one wave per rollout (fused) costs 5x the instructions of one lane per rollout and only pays while the chip is
  // otherwise empty; the time-parallel kernel carries the middle; the sequential one takes over once K/64 one-wave
  // workgroups are ~2.5 per CU.  (Round 1 switched fused -> sequential at 2 per CU and never used the middle kernel
  // below T = 129: K = 16384 ran at half speed.)
  if (2 * waves > 5 * cus) p.scan_tc = 0;
  // fused rollout + partials (lanes = time): T must fit two steps per lane.  With the perturbations drawn inside it the
  // fused kernel saves the sample kernel's launch and 16 B per rollout-step, so device-noise ticks stay with it longer
  // (K = 8192, T = 100: 33.1 us against 36.1 for sample + time-parallel; K = 12288, T = 50: 38.9 against 29.7).
  const bool fused_ok = T <= 2 * kWave && p.scan_tc > 0;
  // (re-measured after the combine learnt to keep a lane's records in registers and to spread over one-wave workgroups —
  //  the fused kernel's many records were what made it lose earlier: K = 8192, T = 100: fused with 16 rollouts per workgroup
  //  20.4 us, time-parallel 22.6; with device noise 21.3 against 35.5)
  p.fused_dev = fused_ok && 2 * waves <= cus;        // K <= 8192 at 256 CUs
  p.fused_rng = fused_ok && 2 * waves <= cus;
  // rollouts per workgroup: 8 spreads K = 1024 over 128 CUs (9.0 us against 10.0 with 16: latency-bound); from ~2048 up the
  // chip is covered anyway and 16 halve the records the combine reads (K = 2048: 11.6 -> 10.7 us, 3072: 14.7 -> 12.1,
  // 4096, T = 100: 20.1 -> 15.6)
  p.fused_r = (p.fused_dev || p.fused_rng) ? (8 * waves <= cus ? 8 : 16) : 0;   // 8 up to K = 2048 (K = 2048, T = 50: 9.2 us against 10.0; 3072: 11.6 against 10.5)
  p.fused_S = p.fused_r ? ceil_div(K, p.fused_r) : 0;
  return p;
}

// ---- TBNAV_MPPI_OPT_KERNEL: a forced choice ---------------------------------------------------------------------------------------------------
// 0: mppi_rollout_cost (sequential); n > 0: mppi_rollout_scan with n steps per thread; -4 / -8 / -16: fused, that many rollouts per workgroup
struct KernelOption { bool ok = false; int scan_tc = 0, fused_r = 0, fused_S = 0; bool fused_dev = false, fused_rng = false; };
inline KernelOption plan_kernel_option(int T, int K, int value) {
  KernelOption o;
  if (value < 0) {
    o.fused_r = -value;
    if (!(T <= 2 * kWave && (o.fused_r == 4 || o.fused_r == 8 || o.fused_r == 16))) return KernelOption{};
  } else if (value > 0) {
    const int cmax = (value == 4 || value == 7 || value == 8) ? 16 : 12;   // chunks (waves) per workgroup the form admits
    bool known = false;
    for (int t : {4, 5, 6, 7, 8, 10, 12, 16, 20}) known |= t == value;
    if (!known || ceil_div(T, value) > cmax) return KernelOption{};
    o.scan_tc = value;
  }
  o.ok = true;
  o.fused_dev = o.fused_r > 0;                      // a forced choice holds for both kinds of tick (in-kernel noise exists for 8 and 16:
  o.fused_rng = o.fused_r == 8 || o.fused_r == 16;  //  a 4-rollout workgroup samples first)
  o.fused_S = o.fused_r ? ceil_div(K, o.fused_r) : 0;
  return o;
}

// ---- small predicates -------------------------------------------------------------------------------------------------------------------------
// the perturbations can be drawn inside the fused kernel: its in-kernel form exists for 8 and 16 rollouts per workgroup (either
// sampler); fused_rng: device-noise ticks take the fused kernel at all (never a handle with a cost field)
inline bool rng_in_kernel(bool fused_rng, int fused_r) { return fused_rng && (fused_r == 8 || fused_r == 16); }
// Noise ahead (TBNAV_MPPI_OPT_NOISE_AHEAD) where the tick is latency-bound: 8 rollouts per workgroup (K <= 2048 at 256 CUs), the
// single-GPU combine (one group of K / 8 records per step: never the four-wave form) with most of the chip idle beside it.
inline bool ahead_wanted(bool fused_rng, int fused_r) { return fused_rng && fused_r == 8; }
// a batch of device-noise ticks is worth a captured graph only where the tick is short enough for the launches themselves to matter:
// K = 1024: 8.25 -> 8.15 us per tick on a fast host, 8.9 -> 8.3 on a slower one; from K = 2048 up the device is the bound and the
// replay is 1-3 % slower than plain launches
inline bool graph_worth_it(bool in_kernel_noise, int fused_r, int K, int n_ticks) { return in_kernel_noise && fused_r == 8 && K <= 1536 && n_ticks >= 2; }

// ---- the rollout launch of the three-kernel tick -------------------------------------------------------------------------------------------
struct RolloutIn { int T, K, dyn, trig, scan_tc, prefix_rg, lds_from; bool field_on; };
struct RolloutPlan {
  KernelForm form;
  int grid = 0, block_y = 1;   // workgroups; waves per workgroup (block = (kWave, block_y))
  size_t lds = 0;              // dynamic LDS
  int lds_from = 0;            // RolloutArgs::lds_from of the launch
  int prefix_rows = 0;         // rows of J that hold exclusive prefixes afterwards (mppi_rollout_prefix)
};
inline RolloutPlan plan_rollout(const RolloutIn& in) {
  RolloutPlan p;
  p.grid = ceil_div(in.K, kWave);
  const bool arc = in.dyn == 1;
  if (in.field_on) {   // a cost field: its own kernel, whatever the handle's choice
    p.form = form_of(kField, 1, arc ? 4 : (in.trig == 1 ? 1 : 3));
    p.lds_from = in.lds_from;
    p.lds = staged_lds_bytes(in.T, in.lds_from);
  } else if (in.scan_tc > 0 && !arc) {   // (the arc dynamics live in the fused and the sequential kernels)
    const int tc = in.scan_tc, C = ceil_div(in.T, tc);   // chunks = waves of a workgroup
    const bool listed = tc == 4 || tc == 5 || tc == 6 || tc == 7 || tc == 8 || tc == 10 || tc == 12 || tc == 16;
    const int mw = (tc == 7 || ((tc == 4 || tc == 8) && C > 12)) ? 16 : 12;
    p.form = form_of(kScan, 3, in.trig == 1 ? 1 : 3, listed ? tc : 20, mw);
    p.block_y = C;
    p.lds = ((size_t)2 * in.T + (size_t)4 * C * kWave) * sizeof(double);
  } else if (in.prefix_rg > 0 && !arc && in.trig == 1) {
    p.form = form_of(kPrefix, 1, in.prefix_rg < 3 ? in.prefix_rg : 3);
    p.lds = (size_t)2 * in.T * sizeof(double);
    p.prefix_rows = in.T - kGroup * in.prefix_rg;
  } else {
    p.form = form_of(kCost, 1, arc ? 4 : (in.trig >= 1 && in.trig <= 2 ? in.trig : 3));
    p.lds_from = in.lds_from;
    p.lds = staged_lds_bytes(in.T, in.lds_from);
  }
  return p;
}

// ---- rollout + partial records in one launch (small K) ----------------------------------------------------------------------------------------
struct FusedIn { int T, K, dyn, trig, sampler, fused_r, fused_S; bool rng; };   // rng: the perturbations are drawn inside the kernel
struct FusedPlan { KernelForm form; int grid = 0, block = 0; size_t lds = 0; };
inline FusedPlan plan_fused(const FusedIn& in) {
  FusedPlan p;
  const int TR = in.dyn == 1 ? 4 : (in.trig == 3 ? 3 : 2), TL = in.T <= kWave ? 1 : 2;
  // in-kernel noise: instantiated for 8 and 16 rollouts per workgroup (the handle's own choices) — the caller checks (rng_in_kernel)
  const int R = in.rng ? (in.fused_r == 16 ? 16 : 8) : (in.fused_r == 8 || in.fused_r == 4 ? in.fused_r : 16);
  // (RNG 2 = the fp64 sampler, the handle's default; RNG 1 = the fp32 one, TBNAV_MPPI_OPT_SAMPLER = 0)
  const int RG = !in.rng ? 0 : (in.sampler == 1 ? 2 : 1);
  p.form = form_of(kFused, 4, TR, R, TL, RG);
  p.grid = in.fused_S;
  p.block = kWave * in.fused_r;
  p.lds = fused_lds_bytes(in.T, in.fused_r);
  return p;
}

// ---- the combine ------------------------------------------------------------------------------------------------------------------------------
// G groups of S records per time step.  direct: the direct exchange's words are polled; err_words: records that came through an
// all-gather may carry a failed rank's poison and raise the error words; ahead: a single-GPU combine also draws the next tick's noise
struct CombinePlan {
  KernelForm form;
  int tpr_log2 = 0;      // lanes per time step = 1 << tpr_log2: the power of two >= the record count, at most a wave
  int blocks = 0;        // workgroups that serve time steps
  int ahead_blocks = 0;  // sampler workgroups behind them, TBNAV_AHEAD_PAIRS pairs per lane (MODE 0 only)
  int grid = 0, block = 0;
};
inline CombinePlan plan_combine(int T, int K, int G, int S, bool direct, bool err_words, bool wide_on, bool ahead) {
  CombinePlan p;
  const int n = G * S, wpb = TBNAV_COMBINE_WAVES;  // records per step; waves per workgroup
  // lanes per time step and the time steps' blocks are formed here, once, and handed to the kernel: they are launch-uniform,
  // and used to head its chain as a loop and an integer division
  while ((1 << p.tpr_log2) < n && (1 << p.tpr_log2) < kWave) ++p.tpr_log2;
  const int steps_per_block = wpb * (kWave >> p.tpr_log2);
  p.blocks = ceil_div(T, steps_per_block);
  // (which form: the direct exchange polls; records that came through an all-gather may carry a failed rank's poison; one group has neither —
  //  and with more than 256 records per step, the fused kernel's at K = 4097 ... 8192, it gets four waves per time step)
  const int mode = direct ? 2 : (G > 1 && err_words) ? 1 : 0;
  if (mode == 0 && G == 1 && S > 4 * kWave && S <= 16 * kWave && wide_on) {
    p.form = form_of(kCombineWide);
    p.grid = T;
    p.block = 4 * kWave;
    return p;
  }
  const int keep = (n > 4 * kWave && n <= 8 * kWave) ? 8 : (n > 2 * kWave && n <= 4 * kWave) ? 4 : 2;
  p.form = form_of(kCombine, 2, keep, mode);
  const long pairs_per_block = (long)wpb * kWave * TBNAV_AHEAD_PAIRS;
  p.ahead_blocks = (ahead && mode == 0) ? (int)(((long)K * T + pairs_per_block - 1) / pairs_per_block) : 0;
  p.grid = p.blocks + p.ahead_blocks;
  p.block = wpb * kWave;
  return p;
}

}  // namespace tbnav_mk
#endif  // TBNAV_MPPI_PLAN_HPP

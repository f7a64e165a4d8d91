// rbpf_plan.hpp — what the host DECIDES before it launches an RBPF kernel, as plain arithmetic: the sizes the kernels and the selection
// share, which map-update and proposal instantiation a scan gets and with how much LDS, and the small rules of create and of the
// window refresh.  No HIP runtime call and no handle type: g++ -std=c++17 compiles this header alone, and tests/rbpf_plan_check.cpp
// holds it against the Python restatements (tests/raycast_cases.py, propose_cases.py, scanmatch_cases.py) without a GPU.
// rbpf_device.hpp includes it for the kernels; rbpf.hip / rbpf_api.hip fill the inputs from the handle and launch what comes back.
#ifndef TBNAV_RBPF_PLAN_HPP
#define TBNAV_RBPF_PLAN_HPP
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <initializer_list>

// (common.hpp pulls the HIP runtime in, which this header must do without: the qualifier lives here)
#ifndef TBNAV_HD
#ifdef __HIPCC__
#define TBNAV_HD __host__ __device__
#else
#define TBNAV_HD
#endif
#endif

namespace tbnav_rk {

constexpr int kWave = 64;
constexpr int kMaxLds = 160 * 1024;
#ifndef TBNAV_PROPOSE_THREADS
#define TBNAV_PROPOSE_THREADS 256
#endif
constexpr int kProposeThreads = TBNAV_PROPOSE_THREADS;
constexpr int kUnCap = 16;  // unstable beams handled by the per-pair path of the proposal kernel
constexpr int kMixLut = 1024;
constexpr int kNormChunk = 2048;
constexpr int kBoxEv = 8;     // events a slot holds before it is replayed exhaustively
// tile u32[cap] | ev u16[bv][kBoxEv] (a slot's first 8 bytes become its replayed value once its events are read) | hot values f64[64] | exy i32[bv] | ecnt u16[bv]
constexpr int kBoxEvFour = 4; // ... in the four-workgroups-per-CU form (8 bytes a slot: exactly the replayed value; the bench room's box fits with them)
TBNAV_HD constexpr size_t box_lds_bytes(size_t cap, size_t bv, size_t ev = kBoxEv) { return 4 * cap + 2 * ev * bv + 8 * 64 + 4 * bv + 2 * ((bv + 1) & ~(size_t)1); }
// the 16-bit cell form: half the cell array + the slot table (hash_words u32, a power of two >= 2 x (bv + 64) slots)
TBNAV_HD constexpr size_t box16_hash_words(size_t bv) { size_t h = 256; while (h < 2 * (bv + 64)) h *= 2; return h; }
TBNAV_HD constexpr size_t box16_lds_bytes(size_t cap, size_t bv, size_t ev = kBoxEv) { return box_lds_bytes(cap, bv, ev) - 2 * cap + 4 * box16_hash_words(bv); }
constexpr size_t kBoxStaticLds = 896;  // the kernel's __shared__ variables (tools/kernel_resources.py rbpf_raycast: 856 B since mt_src, round 5), rounded up
// (512 threads: three workgroups = 24 waves per CU when the LDS array is sized by what the boxes need, see plan_raycast —
//  6 waves per SIMD leave 80 registers a lane: the kernel needs 77 and spills nothing; 1024 threads: two workgroups = 32 waves, 64)
constexpr size_t edt_lds_bytes(int xs, int words, int C) { return (size_t)xs * words * 8 + (size_t)xs * C * 5; }

// ---- create's rules ---------------------------------------------------------------------------------------------------------------------
// Columns a workgroup of the LDS distance transform takes: 64, 32, or — larger maps (xsize > ~640, e.g. BASELINE configs[4]'s
// 2000 x 2000) — 0: no LDS distance transform.  The SLAM path then always answers lookups by query, and an on-demand field is
// produced cell by cell with the same query.
inline int edt_cols_for(int xsize, int words) {
  for (int C : {64, 32}) if (edt_lds_bytes(xsize, words, C) <= (size_t)kMaxLds) return C;
  return 0;
}
// Cells of the map update's LDS tile (0 = the beam-ordered kernel, always): every beam shorter than range_max ends within this many
// cells of the robot cell (+2 for the laser offset / rounding)
inline int tile_cap_for(double range_max, const double Trs[3], double resolution) {
  const double reach = range_max + std::sqrt(Trs[1] * Trs[1] + Trs[2] * Trs[2]);
  const long side = 2 * ((long)std::ceil(reach / resolution) + 2) + 1;
  return (side * side <= 30000) ? (int)(side * side) : 0;
}

// ---- the map update ---------------------------------------------------------------------------------------------------------------------
struct RaycastIn {
  int tile_cap; double resolution; double Trs[3];
  double rmax; int Bv;                        // the scan's longest valid beam, its valid beams
  int threads, adapt, cell16, band_rows;      // TBNAV_RBPF_OPT_RAYCAST_THREADS / _ADAPT / _CELL16 / _BAND_ROWS
  int need;                                   // the mapped word of the boxes' need, read ONCE by the caller
  bool ref_field;
};
struct RaycastPlan {
  int threads = -1;            // 512 | 1024: rbpf_raycast_box<threads, wps, c16, ev>; 0: the beam-ordered rbpf_raycast; -1: nothing launched yet
  int wps = 8; bool c16 = false; int ev = kBoxEv;
  long cap_win = 0;            // cells of the LDS array
  size_t lds = 0;              // dynamic LDS of the box alone (the launch takes more when the normalise rides along)
  int hash_words = 0;
  int need = 0;                // the need the selection used (0: not known yet, or RAYCAST_ADAPT 0)
  int grid = 0;                // (the launch's: its workgroups)
  bool box() const { return threads > 0; }
};
// workgroup 0's two arrays of the riding normalise never decide a residency: four workgroups hold them
static_assert(4 * (2 * 8 * (size_t)kNormChunk + kBoxStaticLds) <= (size_t)kMaxLds, "a launch whose LDS is the normalise's fits four per CU");
inline bool box_fits(int R, size_t bytes) { return (size_t)R * (bytes + kBoxStaticLds) <= (size_t)kMaxLds; }

inline RaycastPlan plan_raycast(const RaycastIn& in) {
  RaycastPlan p;
  const int bvn = in.Bv > 0 ? in.Bv : 1;
  int nt = in.threads;
  const bool nt_auto = nt == 0;
  if (nt == 0) nt = 1024;
  p.need = in.adapt ? in.need : 0;
  // rbpf_raycast_box: one u32 per cell of the box, the box padded to whole groups of 8 cells along y
  long cap_win = 0, cap4 = 0;
  if (in.tile_cap > 0) {
    // every end point lies within `reach` of the robot's position: at most floor(2 reach / res) + 2 rows or columns (+1 spare);
    // along y the box is padded to whole pairs of cells
    const double reach = in.rmax + std::hypot(in.Trs[1], in.Trs[2]);
    const long side = (long)std::floor(2.0 * reach / in.resolution) + 3;
    cap_win = (side * ((side + 2) & ~1L) + 7) & ~7L;
    // ... but no more than lets TWO workgroups share a CU's 160 KB (the kernel works a larger box through in bands of rows;
    // at least one padded row must fit)
    const long cap_fit = ((78L * 1024 - (long)box_lds_bytes(0, (size_t)bvn) - (long)kBoxStaticLds) / 4) & ~7L;
    if (cap_win > cap_fit) cap_win = std::max(cap_fit, (side + 9) & ~7L);
    // (test hook: at most about this many rows of the box per band, to drive the band loop on small maps)
    if (in.band_rows > 0) cap_win = std::min(cap_win, (in.band_rows * ((side + 2) & ~1L) + 7) & ~7L);
    // ... and no more than the particles' boxes needed lately (+ 1/8 + 512 words for what a scan's motion changes): the bound
    // above is the scan's longest beam in every direction from every pose, a room's box is a fraction of that — the array is
    // what keeps a CU at two workgroups.  A box that outgrows the guess costs its particle a second band, not correctness.
    if (p.need > 0) {
      const long want = ((long)p.need + p.need / 8 + 512 + 7) & ~7L;
      cap_win = std::min(cap_win, std::max(want, (side + 9) & ~7L));
      // FOUR 512-thread workgroups per CU — every one of 1000 particles resident at once instead of 768 and a second, partial
      // round (round 4; measured 24.6 / 30.8 / 37.1 us with 1 / 2 / 3 workgroups per CU, 48.3 for 1000 particles on 768 slots) —
      // when the boxes' need plus a margin of three rows or so fits a quarter of the CU's LDS.  The margin is tighter than the
      // three-per-CU form's 1/8 + 512: a box that outgrows it costs its particle a second band, never correctness.
      cap4 = std::max(((long)p.need + 256 + 7) & ~7L, (side + 9) & ~7L);
    }
  }
  // Residency the launch gets: R workgroups per CU need R x (dynamic + static LDS) <= 160 KB (box_fits); 4 and 3 per CU are 512-thread
  // workgroups (64 / 80 registers a lane), 2 per CU 1024 threads (64).  Two cell formats: 32-bit words (slot in the word) and,
  // when that buys a higher residency, 16-bit words + a slot table (C16: a few more instructions per walk step).  Measured at
  // cfg3, N = 1000 / 4000, 32-bit words: 1024 x 2: 55.8 / 191 us; 512 x 2: 54.4 / 199; 512 x 3: 47.9 / 163; 512 x 4 (four
  // events a slot instead of eight: what lets the bench room's 8272-cell boxes in): 41.7 / 143.
  const bool may4 = in.adapt != 2 && cap4 > 0 && cap4 <= cap_win;
  int wps = 8;
  bool c16 = false;
  const bool pick = nt_auto || nt == 512;
  const bool c16_ok = in.cell16 != 0 && cap_win > 0 && cap_win < 65528 && in.Bv + 64 < 32768;
  // (measured, N = 1000: the 16-bit form costs ~15 % at EQUAL residency — 57.2 against 49.8 us at three per CU: twice the
  //  same-dword collisions of the LDS adds where rays converge, the sub-word arithmetic of every step — so going from three to
  //  four per CU with it loses, 51.5 against 49.8 us, and it is used only where the 32-bit form is stuck at TWO per CU: the
  //  SURVEY room's 13 860-cell boxes, 63.7 -> 60.7 us)
  // (four per CU: with eight events a slot where they fit, with four where only they do — measured in a 3 x 1.9 m room whose cells take
  //  5-10 events: 39.4 us with four-event slots against 37.7 with three workgroups per CU and eight)
  size_t ev_slot = kBoxEv;  // (what the instantiation holds per slot)
  const bool force4 = in.adapt == 3;  // (tests: four-event slots wherever four workgroups fit)
  if (pick && may4 && !force4 && box_fits(4, box_lds_bytes((size_t)cap4, (size_t)bvn, kBoxEv))) { nt = 512; cap_win = cap4; }
  else if (pick && may4 && box_fits(4, box_lds_bytes((size_t)cap4, (size_t)bvn, kBoxEvFour))) { nt = 512; cap_win = cap4; ev_slot = kBoxEvFour; }
  else if (pick && cap_win > 0 && box_fits(3, box_lds_bytes((size_t)cap_win, (size_t)bvn))) { nt = 512; wps = 6; }
  else if (pick && may4 && c16_ok && box_fits(4, box16_lds_bytes((size_t)cap4, (size_t)bvn, kBoxEv))) { nt = 512; cap_win = cap4; c16 = true; }
  // (no 16-bit form with four-event slots: its niche — boxes that fit four per CU only with BOTH economies — is a few hundred cells wide, and
  //  the instantiation was the one map-update kernel left with a spill; such boxes run three per CU in <512, 6, true, 8>)
  else if (pick && c16_ok && box_fits(3, box16_lds_bytes((size_t)cap_win, (size_t)bvn))) { nt = 512; wps = 6; c16 = true; }
  else if (nt == 512) wps = 6;
  if (in.cell16 == 2 && c16_ok && nt == 512) c16 = true;   // (tests / A-B: the 16-bit form wherever it can run)
  if (c16) ev_slot = kBoxEv;   // (the 16-bit form has eight-event slots only)
  p.lds = c16 ? box16_lds_bytes((size_t)cap_win, (size_t)bvn, ev_slot) : box_lds_bytes((size_t)cap_win, (size_t)bvn, ev_slot);
  p.wps = wps; p.c16 = c16; p.ev = (int)ev_slot; p.cap_win = cap_win;
  p.hash_words = c16 ? (int)box16_hash_words((size_t)bvn) : 0;
  // default: box counters (rbpf_raycast_box).  The beam-ordered kernel: scans the LDS tile cannot hold, and the reference
  // distance-field mode (it logs the occupied-set changes in the reference's order)
  const bool box = cap_win > 0 && !in.ref_field && in.Bv < 32768 - kWave && nt >= 512 && p.lds <= (size_t)kMaxLds - 4096;
  p.threads = !box ? 0 : (nt == 512 ? 512 : 1024);
  return p;
}

// ---- the proposal and what runs in front of it ----------------------------------------------------------------------------------------
// how far the sampled poses sit from the pose they are drawn round, at most (metres): eight standard deviations of the wider noise
inline double sampling_spread(const double sample_range[3], const double motion_noise[3]) {
  double sig = 0.0;
  for (int q = 1; q < 3; ++q) sig = std::max(sig, std::max(sample_range[q], motion_noise[q]));
  return 8.0 * std::sqrt(sig);
}
// Half-width (cells) of the window the stored field is refreshed in before a scan.  Every lookup of the call lies within `half`
// metres of the particle's CURRENT position: the sampled poses sit at T(pose)*T_icp (or the motion-model pose) +- the sampling
// noise, the laser at |Trs| from them, and a valid beam ends less than range_max from the laser.  With the scan matcher on, the
// samples sit round the MATCHED pose and the matcher's own trial poses look cells up too: a trial pose of round r is at most
// (r + 1) * lstep from T(pose)*T_icp and r < max_moves, so its travel is bounded by max_moves * lstep (3.2 m with the default
// step) — matcher_travel, 0 without it.  whole_map (the legacy full-field mode), or a window wider than the map: xsize.
inline int lookup_half_cells(double range_max, const double Trs[3], const double T_icp[3], const double u[3], double spread,
                             double matcher_travel, double resolution, bool whole_map, int xsize) {
  const double move = std::max(std::hypot(T_icp[1], T_icp[2]), std::fabs(u[1]));
  double half = range_max + std::hypot(Trs[1], Trs[2]) + move + spread;
  if (matcher_travel > 0.0) half += matcher_travel;
  const int half_cells = (int)std::ceil(half / resolution) + 3;
  return (whole_map || half_cells > xsize) ? xsize : half_cells;
}

struct ProposeIn { int k, Bv, df_mode, xsize, words; double range_max, spread, resolution; };
struct ProposePlan {
  int occ_half = 0; size_t slice_bytes = 0;   // the LDS slice of the occupancy bitmap (query mode): its half-width in cells, 0 = none
  size_t lds = 0, sm_lds = 0;                 // dynamic LDS of rbpf_propose / of rbpf_scanmatch
  int threads = 0;                            // rbpf_propose<threads, dn>; 0: nothing launched yet
  bool fits = false;                          // false: scan x samples too large for one workgroup's LDS
  bool dn = false;                            // (the launch's: noise drawn inside the kernel)
};
inline ProposePlan plan_propose(const ProposeIn& in) {
  ProposePlan p;
  const size_t bvn = in.Bv > 0 ? in.Bv : 1;
  if (in.df_mode == 2) {
    // LDS copy of the occupancy bitmap round each particle's sensor: reach of a lookup (range_max + sampling
    // spread) plus a margin for the walk to the nearest obstacle; shrunk, then dropped, if it would not fit
    const int reach = (int)std::ceil((in.range_max + in.spread) / in.resolution) + 2;
    for (int margin : {48, 16, 0}) {
      const int half = reach + margin;
      const int rows = std::min(in.xsize, 2 * half + 1), nw = std::min(in.words, (2 * half + 1 + 63) / 64 + 1);
      const size_t bytes = (size_t)rows * nw * 8 + (size_t)rows * 4;
      if (bytes <= 48 * 1024) { p.occ_half = half; p.slice_bytes = bytes; break; }
    }
  }
  p.lds = sizeof(double) * ((12 + kUnCap) * (size_t)in.k + 3 * bvn) + sizeof(unsigned int) * 4 * bvn + p.slice_bytes;
  p.sm_lds = 2 * sizeof(double) * bvn + sizeof(double) * kMixLut + sizeof(unsigned long long) * 4 * bvn + p.slice_bytes;
  p.fits = p.lds <= (size_t)kMaxLds - 3072;
  // workgroup size: four waves when four workgroups fit a CU's LDS (the 360-beam scans: 38 KB each), eight when the scan's
  // tables leave room for two or three only (1080 beams: 58 KB) — measured: 360 beams 32 us per 1000 particles with 256
  // threads against 43 with 512; the configs[4] shard 0.80 ms with 256 against 0.61 with 512
  p.threads = (p.lds + 3072 > (size_t)kMaxLds / 4) ? 2 * kProposeThreads : kProposeThreads;
  return p;
}

}  // namespace tbnav_rk
#endif  // TBNAV_RBPF_PLAN_HPP

// nav_host.hpp — the goal field's handle and what its host files share (nav.hip: create / solve / results / hand-over of the solved
// field; nav_from_map.hip: the cost grid taken from a filter's occupancy bits on the device, tbnav_nav.h G7-G9; nav_frontier.hip: the
// frontiers of a particle's map, their clusters, and the solves that start from several goals, G10-G16; nav_gain.hip: the seeds'
// information gain and the ranked solve, G17-G20): the rounds of a tiled fixed point, the handle's allocations and lazy host copies,
// the optional stage timing, and the filter as the source of a grid.  What the kernels share is nav_tiles.hpp.
#ifndef TBNAV_NAV_HOST_HPP
#define TBNAV_NAV_HOST_HPP
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "common.hpp"
#include "nav_tiles.hpp"
#include "rbpf_host.hpp"
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
  // G10-G16 (nav_frontier.hip).  Everything below is allocated at the first use of that file's calls, never at create.
  unsigned* d_front = nullptr;      // [nx][tiles_y] frontier bits: row ix, word iy >> 5, bit iy & 31 (TilePool::bm's layout)
  unsigned* d_seed = nullptr;       // [nx][tiles_y] ... of the seeds
  unsigned* d_visited = nullptr;    // [nx][tiles_y] ... of the visited mask
  unsigned* d_label = nullptr;      // [nx][ny] G12's labels
  unsigned* d_size = nullptr;       // [nx][ny] cells per cluster, at the cluster's root
  unsigned* d_fflags = nullptr;     // [2][tiles] active tiles of the labelling's even and odd rounds
  unsigned* d_frec = nullptr;       // [batch][2] its round records
  unsigned* d_fcount = nullptr;     // [4] frontier cells, clusters, seed clusters, seed cells
  int* d_goals = nullptr;           // [goals_cap][2] the list of tbnav_nav_solve_goals
  int goals_cap = 0;
  std::vector<unsigned> visited;    // host side of d_visited: the mask lives here (G14) and is uploaded when it changed
  bool visited_dirty = true;
  std::vector<unsigned> label_host; // the downloaded labels (filled at their first use after a find)
  bool label_host_valid = false;
  // a find's seeds are goals only while the grid and the mask it saw are the ones in force: every successful set of either counts
  uint64_t cost_epoch = 0, visited_epoch = 0, found_cost_epoch = 0, found_visited_epoch = 0;
  tbnav_nav_frontier_info finfo{0, 0, 0, 0, 0, 0, 0, 0, 0};
  // G17-G20 (nav_gain.hip), allocated at the first find with gain or ranked solve
  unsigned* d_gunk = nullptr;       // [nx][tiles_y] UNKNOWN bits of the particle's map (d_front's layout)
  unsigned* d_gocc = nullptr;       // [nx][tiles_y] OCCUPIED bits, and the columns of a ragged last word past the map's side
  unsigned* d_glist = nullptr;      // [glist_cap] the viewpoints' cell indices, in no order
  int glist_cap = 0;
  short* d_grays = nullptr;         // [kGainMaxRays][2] E(R) of grays_range
  int grays_range = 0;
  unsigned* d_gain = nullptr;       // [nx][ny] G18's gain, 0 off the viewpoints
  unsigned long long* d_gstat = nullptr;   // [0] max of gain << 32 | ~cell, [1] max of ~gain, [2] (as unsigned) the list's slot counter
  unsigned* d_start = nullptr;      // [nx][ny] the last ranked solve's start values, UNREACHED off its seeds (G6 generalised walks over it)
  std::vector<unsigned> gain_host, start_host;   // downloaded at their first use
  bool gain_host_valid = false, start_host_valid = false;
  bool ranked = false;              // the last solve was a ranked one: tbnav_nav_path stops by start_host
  int gain_rmax = 0;                // nav_frontier_gain's instantiation of the last find with gain, 0: none ran
  tbnav_nav_gain_info ginfo{0, 0, 0, 0, 0, 0, {-1, -1}};
  std::vector<void**> buffers;     // the d_ members that hold an allocation (dev_alloc lists them, destroy walks them)
};

namespace tbnav_nk {
// room for a table of TBNAV_NAV_MAX_REACH^2 + 1 entries and the open value
constexpr int kInflEntries = TBNAV_NAV_MAX_REACH * TBNAV_NAV_MAX_REACH + 2;

// Rounds per batch: in open space the front crosses about a tile per round, so half the tiles along both sides is a batch or two
// per solve; at least 4 (a host read costs several launches), at most kMaxBatch (what a finished solve wastes on launches that find
// no active tile).  Doubling the batch while a solve goes on was measured and lost: the serpentine's 100 rounds are bound by their
// sweeps, not by the host's reads (5.5 against 5.7 ms), and the 400 x 400 solves paid 13 more empty launches (0.65 against 0.61 ms).
constexpr int kMaxBatch = 32;
inline int batch_rounds(const tbnav_nav* h) {
  const int b = (h->tiles_x + h->tiles_y) / 2;
  return b < 4 ? 4 : (b > kMaxBatch ? kMaxBatch : b);
}

// The host side of a tiled fixed-point iteration (nav_relax_tiles, nav_frontier_label): rounds are enqueued in batches on `stream`,
// launch(cur, nxt, rec) being one round over the active tiles of `flags` ([2][tiles]: even and odd rounds; the even array holds round
// 0's tiles, the odd one is zero); one record per batch is read (rec[0] tiles visited, rec[1] tiles in which something changed) and the
// first round that changed nothing ends it — the proof of the fixed point.
template <class Launch>
int run_rounds(tbnav_nav* h, unsigned* flags, unsigned* d_rec, hipStream_t stream, Launch launch, int* rounds_out, int* launches_out, long long* visits_out) {
  const int tiles = h->tiles_x * h->tiles_y, B = batch_rounds(h);
  // an iteration that moved one cell per round would need fewer than n rounds; these never need more
  const long long round_cap = (long long)h->n + kMaxBatch;
  unsigned rec[2 * kMaxBatch];
  int rounds = 0, launches = 0;
  long long visits = 0;
  for (int r0 = 0; rounds == 0; r0 += B) {
    if (r0 > round_cap) return TBNAV_ERR_UNSUPPORTED;
    TBNAV_HIP(hipMemsetAsync(d_rec, 0, sizeof(unsigned) * 2 * B, stream));
    for (int r = 0; r < B; ++r) launch(flags + ((r0 + r) & 1) * tiles, flags + ((r0 + r + 1) & 1) * tiles, d_rec + 2 * r);
    TBNAV_HIP(hipGetLastError());
    launches += B;
    if (stream) {
      TBNAV_HIP(hipMemcpyAsync(rec, d_rec, sizeof(unsigned) * 2 * B, hipMemcpyDeviceToHost, stream));
      TBNAV_HIP(hipStreamSynchronize(stream));
    } else {
      TBNAV_HIP(hipMemcpy(rec, d_rec, sizeof(unsigned) * 2 * B, hipMemcpyDeviceToHost));   // waits for the batch
    }
    for (int r = 0; r < B && rounds == 0; ++r) {
      visits += rec[2 * r];
      if (rec[2 * r + 1] == 0) rounds = r0 + r + 1;   // nothing changed, so nothing was marked: every later round finds no tile
    }
  }
  *rounds_out = rounds; *launches_out = launches; *visits_out = visits;
  return TBNAV_OK;
}

// nav.hip: the rounds of nav_relax_tiles from whatever start d_d and d_flags hold (nav_reset / nav_reset_goals have been enqueued on the
// null stream; the handle's device is current), and what a finished solve leaves in the handle.  h->solved is false while it runs.
int relax_from_start(tbnav_nav* h, int goal_ix, int goal_iy);
// nav_frontier.hip: G10-G13 with the stages' times where they are asked for (ms[4]); the handle's gain, if it had one, is gone afterwards
int find_frontiers(tbnav_nav* h, tbnav_rbpf* pf, int32_t particle, int32_t min_cells, tbnav_nav_frontier_info* info, float* ms);

// words of a bit mask over the grid in TilePool::bm's layout, [nx][tiles_y]: the frontier, seed and visited bits, the gain's classes
inline size_t mask_words(const tbnav_nav* h) { return (size_t)h->p.nx * h->tiles_y; }
inline bool in_grid(const tbnav_nav* h, int ix, int iy) { return ix >= 0 && ix < h->p.nx && iy >= 0 && iy < h->p.ny; }

// `count` elements on the device into `slot`, a d_ member of the handle (its device is current); what the member held is freed once
// the new allocation stands
template <class T>
hipError_t dev_alloc(tbnav_nav* h, T*& slot, size_t count) {
  T* p = nullptr;
  const hipError_t e = hipMalloc((void**)&p, sizeof(T) * count);
  if (e != hipSuccess) return e;
  if (slot) (void)hipFree(slot);
  else h->buffers.push_back((void**)&slot);
  slot = p;
  return hipSuccess;
}

// the lazy host copies: dev[n] into `host` unless `valid` says it is there already
template <class T>
int fetch_once(tbnav_nav* h, const T* dev, std::vector<T>& host, bool& valid) {
  if (valid) return TBNAV_OK;
  tbnav::DeviceGuard guard(h->device);
  if (!guard.ok) return TBNAV_ERR_NO_DEVICE;
  host.resize((size_t)h->n);
  TBNAV_HIP(hipMemcpy(host.data(), dev, sizeof(T) * (size_t)h->n, hipMemcpyDeviceToHost));
  valid = true;
  return TBNAV_OK;
}

// Optional event timing round the stages of a profile call: `stamps` events on `stream`, stage i lying between stamps i and i + 1.
// Where no times are asked for (!on) no event exists and every call does nothing.
struct StageTimer {
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  hipStream_t stream;
  int n;
  StageTimer(bool on, int stamps, hipStream_t st) : stream(st), n(on ? stamps : 0) {}
  ~StageTimer() { for (int i = 0; i < n; ++i) if (ev[i]) (void)hipEventDestroy(ev[i]); }
  hipError_t create() {
    hipError_t e = hipSuccess;
    for (int i = 0; i < n && e == hipSuccess; ++i) e = hipEventCreate(&ev[i]);
    return e;
  }
  hipError_t stamp(int i) { return n ? hipEventRecord(ev[i], stream) : hipSuccess; }
  hipError_t elapsed(int i, float* ms) { return n ? hipEventElapsedTime(ms, ev[i], ev[i + 1]) : hipSuccess; }   // (once the stream has been waited for)
};

// ---- a particle of a filter as the source of a grid (nav_from_map.hip, nav_frontier.hip) ----
inline bool particle_ok(const tbnav_rbpf* pf, int32_t particle) {
  return particle == TBNAV_NAV_BEST_PARTICLE || (particle >= 0 && particle < pf->N);
}
inline ParticleRef particle_ref(const tbnav_rbpf* pf, int32_t particle) {
  return ParticleRef{pf->d_table[pf->cur], particle == TBNAV_NAV_BEST_PARTICLE ? pf->d_best : nullptr, particle, pf->TW, pf->TT, pf->xsize};
}
// the arg-max of the weights into pf->d_best where the best particle is asked for, on the filter's stream (its device is current)
inline int enqueue_best(tbnav_rbpf* pf, int32_t particle) {
  if (particle != TBNAV_NAV_BEST_PARTICLE) return TBNAV_OK;
  const StatePtrs sp = state_ptrs(pf->d_state[pf->cur], pf->N);
  hipLaunchKernelGGL(rbpf_argmax, dim3(1), dim3(256), 0, pf->stream, pf->N, sp.weight, sp.pose, pf->d_best, pf->d_best_pose);
  TBNAV_HIP(hipGetLastError());
  return TBNAV_OK;
}
// G8: the handle and the filter describe one grid (else TBNAV_ERR_INVALID_ARG) on one device (else TBNAV_ERR_UNSUPPORTED)
inline int same_grid(const tbnav_nav* h, const tbnav_rbpf* pf) {
  if (h->p.nx != pf->xsize || h->p.ny != pf->xsize || pf->ysize != pf->xsize || h->p.xmin != pf->p.xmin || h->p.ymin != pf->p.ymin ||
      h->p.resolution != pf->p.resolution)
    return TBNAV_ERR_INVALID_ARG;
  return h->device != pf->device ? TBNAV_ERR_UNSUPPORTED : TBNAV_OK;
}
}  // namespace tbnav_nk

#endif

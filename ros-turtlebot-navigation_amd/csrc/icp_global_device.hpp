// icp_global_device.hpp — what the global search's kernels (icp_global.hip) and the hypotheses' kernels behind them (icp_hyp.hip)
// share: the layout of the byte maps, the packed offsets, the search's geometry and the record the host reads.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "icp_device.hpp"

namespace tbnav_icpdev {

constexpr int kGlobalMargin = 32;    // zero cells before cell 0 of the byte maps: the largest s, so pool(-s, .) is stored too

// what the host reads: one record, then the histogram
struct GlobalRec {
  unsigned long long key;   // max of score << 32 | ~linear index
  uint32_t maxb;            // the largest bound
  uint32_t points;          // valid source points
  uint32_t occupied;
  uint32_t nlist;           // icp_global_list's slot counter
  uint32_t pad[2];
};
static_assert(sizeof(GlobalRec) == 32, "the histogram behind it stays aligned");

// the byte maps: cell (ci, cj) at [(ci + kGlobalMargin) * P + cj + kGlobalMargin]; a coordinate clamped to -kGlobalMargin .. side reads
// what the unclamped one would: zero outside the map (lik), zero outside -(s - 1) .. side - 1 (pool)
__device__ __forceinline__ int clamp_cell(int v, int side) { return min(max(v, -kGlobalMargin), side); }
__device__ __forceinline__ int off_x(uint32_t o) { return (int)(short)(o & 0xffffu); }
__device__ __forceinline__ int off_y(uint32_t o) { return (int)(short)(o >> 16); }

struct SearchArgs {
  int side, P, s, q;
  int tx0, ty0, w, h;        // the region
  int nbx, nby;
  int n_beams;
};

// HYPOTHESES (tbnav_icp.h H1-H10): what icp_hyp.hip's launches need beside SearchArgs
struct HypArgs {
  uint32_t t;                // H2's floor, >= 1
  int NA, Ba, B;             // headings; a bin is Ba headings x B x B cells
  int nba, nbbx, nbby;       // bins per axis
  int sep_cells, sep_steps, wrap, K;
  uint32_t list_cap, cand_cap;
};

// the counters and the chosen keys icp_hyp_select leaves
struct HypRec {
  uint32_t ncand;            // candidates with score >= t (all of them, listed or not)
  uint32_t npeaks;
  uint32_t pad[2];
  unsigned long long keys[TBNAV_ICP_HYP_MAX];   // the first K peaks in descending key order, 0 behind them
};

// icp_hyp.hip: collect, knock and select behind a filled list of blocks (rec->nlist of them, at most a.list_cap listed), on `stream`;
// bins (uint64 [bins]) and alive (uint8 [bins]) are zeroed / set here.  Nothing is waited for.
int hyp_enqueue(hipStream_t stream, const SearchArgs& a, const HypArgs& ha, int threads, const uint8_t* lik, const uint32_t* off,
                const uint32_t* cnt, const uint32_t* list, const GlobalRec* rec, unsigned long long* cands, uint8_t* flags,
                unsigned long long* peaks, unsigned long long* bins, uint8_t* alive, HypRec* hrec);

}  // namespace tbnav_icpdev

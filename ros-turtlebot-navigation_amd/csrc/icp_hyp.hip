// icp_hyp.hip — the global search's separated peaks (include/tbnav_icp.h, HYPOTHESES, items H1-H10; an addition with no counterpart
// in the reference; restated in tests/icp_hyp_restatement.py).  The global search (icp_global.hip) finds the best score and lists the
// blocks whose bound reaches the floor t; behind that list:
//   icp_hyp_collect  one workgroup per listed block: its candidates' scores as icp_global_refine takes them; every candidate with
//                    score >= t is appended to a list of keys (score << 32 | ~index; one atomic add per wave) and folded into its bin
//                    of (sep_steps + 1) x (sep_cells + 1)^2 candidates with a 64-bit atomicMax
//   icp_hyp_knock    one lane per listed candidate: every bin that can hold a candidate of its window is looked at, and a bin's
//                    winner that lies inside the window with a lesser key loses its alive flag
//   icp_hyp_select   one workgroup: the alive winners are the peaks (H4); they are flagged, counted and compacted, and the first K
//                    in key order are left for the host (K passes of a workgroup-wide maximum below the previous key)
// Why that is exact: a bin is no wider than a window's half extent + 1, so its members lie in each other's windows and a peak is its
// bin's winner; and every candidate of a winner's window lies in a bin the winner's neighbours reach.  Winners are NOT compared with
// winners only: any listed candidate may knock.  Integers only.  No workgroup waits for another; every loop is bounded by the points,
// s, the bins round a candidate, the candidates or K.
#include <hip/hip_runtime.h>

#include "common.hpp"
#include "icp_device.hpp"
#include "icp_global_device.hpp"
#include "icp_search_device.hpp"
#include "tbnav_icp.h"

namespace {

using namespace tbnav_icpdev;

constexpr int kLanes = tbnav_icpdev::kWave;
constexpr int kMargin = kGlobalMargin;

struct Cand {
  int ia, tx, ty;
};

__device__ __forceinline__ Cand cand_of(unsigned long long key, int side) {
  const uint32_t lin = ~(uint32_t)key;
  const uint32_t row = lin / (uint32_t)side;
  Cand c;
  c.ty = (int)(lin - row * (uint32_t)side);
  c.ia = (int)(row / (uint32_t)side);
  c.tx = (int)(row - (uint32_t)c.ia * (uint32_t)side);
  return c;
}

__device__ __forceinline__ uint32_t bin_of(const Cand& c, const SearchArgs& a, const HypArgs& ha) {
  return (uint32_t)(((c.ia / ha.Ba) * ha.nbbx + (c.tx - a.tx0) / ha.B) * ha.nbby + (c.ty - a.ty0) / ha.B);
}

// blockIdx.x: the place in the list
__global__ __launch_bounds__(kThreads) void icp_hyp_collect(SearchArgs a, HypArgs ha, const uint8_t* __restrict__ lik,
                                                            const uint32_t* __restrict__ off, const uint32_t* __restrict__ cnt,
                                                            const uint32_t* __restrict__ list, const GlobalRec* __restrict__ rec,
                                                            unsigned long long* __restrict__ cands, unsigned long long* __restrict__ bins,
                                                            HypRec* __restrict__ hrec) {
  __shared__ uint32_t s_off[TBNAV_ICP_MAX_BEAMS];
  const int tid = threadIdx.x, lane = tid & (kLanes - 1);
  if (blockIdx.x >= min(rec->nlist, ha.list_cap)) return;
  const uint32_t blk = list[blockIdx.x];
  const int per = a.nbx * a.nby;
  const int ia = (int)(blk / (uint32_t)per), r = (int)(blk - (uint32_t)ia * (uint32_t)per);
  const int Bx = r / a.nby, By = r - Bx * a.nby;
  const int bx = a.tx0 + (Bx << a.q), by = a.ty0 + (By << a.q);
  const int n = (int)min(cnt[ia], (uint32_t)min(a.n_beams, TBNAV_ICP_MAX_BEAMS));
  for (int i = tid; i < n; i += blockDim.x) s_off[i] = off[(size_t)ia * a.n_beams + i];
  __syncthreads();
  // the trip count is the workgroup's, so a wave's lanes reach the ballot together
  for (int base = 0; base < a.s * a.s; base += blockDim.x) {
    const int c = base + tid;
    const int tx = bx + (c >> a.q), ty = by + (c & (a.s - 1));
    const bool live = c < a.s * a.s && tx < a.tx0 + a.w && ty < a.ty0 + a.h;          // a ragged block
    uint32_t sum = 0u;
    if (live) {
      for (int p = 0; p < n; ++p) {
        const uint32_t o = s_off[p];
        const int x = clamp_cell(tx + off_x(o), a.side), y = clamp_cell(ty + off_y(o), a.side);
        sum += lik[(size_t)(x + kMargin) * a.P + (y + kMargin)];
      }
    }
    const bool keep = live && sum >= ha.t;
    const unsigned long long vote = __ballot(keep);
    if (vote == 0ull) continue;
    uint32_t first = 0u;
    if (lane == 0) first = atomicAdd(&hrec->ncand, (uint32_t)__popcll(vote));
    first = (uint32_t)__shfl((int)first, 0, kLanes);
    if (keep) {
      const unsigned long long key = ((unsigned long long)sum << 32) | (uint32_t)~(((uint32_t)ia * a.side + tx) * a.side + ty);
      const uint32_t slot = first + (uint32_t)__popcll(vote & ((1ull << lane) - 1ull));
      if (slot < ha.cand_cap) cands[slot] = key;
      const Cand me{ia, tx, ty};
      atomicMax(&bins[bin_of(me, a, ha)], key);
    }
  }
}

__device__ __forceinline__ bool in_window(const Cand& c, const Cand& o, const HypArgs& ha) {
  const int dx = abs(o.tx - c.tx), dy = abs(o.ty - c.ty);
  int da = abs(o.ia - c.ia);
  if (ha.wrap) da = min(da, ha.NA - da);
  return dx <= ha.sep_cells && dy <= ha.sep_cells && da <= ha.sep_steps;
}

// one lane per listed candidate, in a grid-stride loop
__global__ __launch_bounds__(kThreads) void icp_hyp_knock(SearchArgs a, HypArgs ha, const unsigned long long* __restrict__ cands,
                                                          const unsigned long long* __restrict__ bins, uint8_t* __restrict__ alive,
                                                          const HypRec* __restrict__ hrec) {
  const uint32_t n = min(hrec->ncand, ha.cand_cap);
  for (uint32_t i = blockIdx.x * kThreads + threadIdx.x; i < n; i += gridDim.x * kThreads) {
    const unsigned long long key = cands[i];
    const Cand c = cand_of(key, a.side);
    // the headings of the window, in order from `start`, nh of them
    int start, nh;
    if (ha.wrap) {
      if (2 * ha.sep_steps + 1 >= ha.NA) {
        start = 0; nh = ha.NA;
      } else {
        start = c.ia - ha.sep_steps; nh = 2 * ha.sep_steps + 1;
        if (start < 0) start += ha.NA;
      }
    } else {
      start = max(0, c.ia - ha.sep_steps);
      nh = min(ha.NA - 1, c.ia + ha.sep_steps) - start + 1;
    }
    const int cbx = (c.tx - a.tx0) / ha.B, cby = (c.ty - a.ty0) / ha.B;
    const int x_lo = max(cbx - 1, 0), x_hi = min(cbx + 1, ha.nbbx - 1);
    const int y_lo = max(cby - 1, 0), y_hi = min(cby + 1, ha.nbby - 1);
    for (int j = 0; j < nh;) {
      int iap = start + j;
      if (iap >= ha.NA) iap -= ha.NA;
      const int ba = iap / ha.Ba;
      j += min((ba + 1) * ha.Ba, ha.NA) - iap;                 // on to the next angular bin, or past the last heading
      for (int x = x_lo; x <= x_hi; ++x) {
        for (int y = y_lo; y <= y_hi; ++y) {
          const uint32_t b = (uint32_t)((ba * ha.nbbx + x) * ha.nbby + y);
          const unsigned long long w = bins[b];
          if (w == 0ull || w >= key) continue;
          if (in_window(c, cand_of(w, a.side), ha)) alive[b] = (uint8_t)0;
        }
      }
    }
  }
}

// one workgroup
__global__ __launch_bounds__(kThreads) void icp_hyp_select(SearchArgs a, HypArgs ha, const unsigned long long* __restrict__ cands,
                                                           const unsigned long long* __restrict__ bins, const uint8_t* __restrict__ alive,
                                                           uint8_t* __restrict__ flags, unsigned long long* __restrict__ peaks,
                                                           HypRec* __restrict__ hrec) {
  __shared__ uint32_t s_np;
  __shared__ unsigned long long s_max[kThreads / kLanes];
  const int tid = threadIdx.x, lane = tid & (kLanes - 1);
  const uint32_t n = min(hrec->ncand, ha.cand_cap);
  if (tid == 0) s_np = 0u;
  __syncthreads();
  for (uint32_t base = 0; base < n; base += kThreads) {
    const uint32_t i = base + tid;
    bool peak = false;
    unsigned long long key = 0ull;
    if (i < n) {
      key = cands[i];
      const uint32_t b = bin_of(cand_of(key, a.side), a, ha);
      peak = bins[b] == key && alive[b] != 0;
      flags[i] = (uint8_t)peak;
    }
    const unsigned long long vote = __ballot(peak);
    if (vote == 0ull) continue;
    uint32_t first = 0u;
    if (lane == 0) first = atomicAdd(&s_np, (uint32_t)__popcll(vote));
    first = (uint32_t)__shfl((int)first, 0, kLanes);
    if (peak) peaks[first + (uint32_t)__popcll(vote & ((1ull << lane) - 1ull))] = key;      // a peak is a candidate: np <= n <= cand_cap
  }
  __syncthreads();
  const uint32_t np = s_np;
  if (tid == 0) hrec->npeaks = np;
  unsigned long long prev = ~0ull;
  for (int k = 0; k < ha.K; ++k) {
    unsigned long long m = 0ull;
    for (uint32_t i = tid; i < np; i += kThreads) {
      const unsigned long long v = peaks[i];
      if (v < prev && v > m) m = v;
    }
    m = wave_max_u64(m);
    if (lane == 0) s_max[tid / kLanes] = m;
    __syncthreads();
    m = 0ull;
#pragma unroll
    for (int wv = 0; wv < kThreads / kLanes; ++wv) m = s_max[wv] > m ? s_max[wv] : m;
    __syncthreads();
    if (m == 0ull) break;                                         // (the workgroup's: every thread holds the same m)
    if (tid == 0) hrec->keys[k] = m;
    prev = m;
  }
}

}  // namespace

namespace tbnav_icpdev {

int hyp_enqueue(hipStream_t stream, const SearchArgs& a, const HypArgs& ha, int threads, const uint8_t* lik, const uint32_t* off,
                const uint32_t* cnt, const uint32_t* list, const GlobalRec* rec, unsigned long long* cands, uint8_t* flags,
                unsigned long long* peaks, unsigned long long* bins, uint8_t* alive, HypRec* hrec) {
  const size_t nbins = (size_t)ha.nba * ha.nbbx * ha.nbby;
  TBNAV_HIP(hipMemsetAsync(bins, 0, sizeof(unsigned long long) * nbins, stream));
  TBNAV_HIP(hipMemsetAsync(alive, 1, nbins, stream));
  TBNAV_HIP(hipMemsetAsync(hrec, 0, sizeof(HypRec), stream));
  hipLaunchKernelGGL(icp_hyp_collect, dim3(ha.list_cap), dim3(threads), 0, stream, a, ha, lik, off, cnt, list, rec, cands, bins, hrec);
  const uint32_t want = (ha.cand_cap + kThreads - 1) / kThreads;
  hipLaunchKernelGGL(icp_hyp_knock, dim3(want < 1024u ? want : 1024u), dim3(kThreads), 0, stream, a, ha, cands, bins, alive, hrec);
  hipLaunchKernelGGL(icp_hyp_select, dim3(1), dim3(kThreads), 0, stream, a, ha, cands, bins, alive, flags, peaks, hrec);
  TBNAV_HIP(hipGetLastError());
  return TBNAV_OK;
}

}  // namespace tbnav_icpdev

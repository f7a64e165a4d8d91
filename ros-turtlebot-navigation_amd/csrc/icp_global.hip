// icp_global.hip — where the robot is in a filter particle's map, with no guess (include/tbnav_icp.h, GLOBAL SEARCH, items L1-L10;
// an addition with no counterpart in the reference; restated in tests/icp_global_restatement.py).  Every heading at every cell is a
// candidate; blocks of s x s cells are pruned with the exact bound of a max-pooled copy of the likelihood map.  Integers only but
// for L3's offsets (fp64, this file is compiled with contraction off).
//   icp_global_field    one workgroup per 32 x 32 map tile: lik (L2) by icp_search_table_from_occ's nearest-set-bit search, into a
//                       byte map with a zero margin; occupied, one atomic add per tile
//   icp_global_pool     the s x s forward sliding maximum (L5's pool), rows then columns through LDS
//   icp_global_offsets  one workgroup per heading: L3's (ox, oy) of the points that can add anything, compacted in no order; points
//   icp_global_bound    one workgroup per (heading, 4 x 64 blocks): L5's bound, lanes along ty; the largest bound
//   icp_global_hist     1024 bins of the bounds, for the host to choose the seeds' least bound
//   icp_global_list     the blocks with lo <= bound < hi, through one slot counter
//   icp_global_refine   one workgroup per listed block: its candidates' scores, one 64-bit atomicMax of (score << 32 | ~index) per wave
// No workgroup waits for another; every loop is bounded by the points, the tile or s.
// The host half of HYPOTHESES (H1-H10, tbnav_icp_localize_map_hyp) lives here too, behind the same prepare and run: it lists the blocks
// whose bound reaches the floor with icp_global_list and hands them to icp_hyp.hip's kernels (icp_global_device.hpp: hyp_enqueue).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "icp_device.hpp"
#include "icp_global_device.hpp"
#include "icp_search_device.hpp"
#include "nav_host.hpp"
#include "tbnav_icp.h"

namespace {

using namespace tbnav_icpdev;

constexpr int kLanes = tbnav_icpdev::kWave;
constexpr int kMargin = kGlobalMargin;   // zero cells before cell 0 of the byte maps (icp_global_device.hpp)
constexpr int kHistBins = 1024;
constexpr int kSeeds = 16;           // round 1 refines at least this many blocks, those with the largest bounds
constexpr int kPoolI = 32, kPoolJ = 64, kPoolMaxS = 32;
constexpr int kBoundBx = kThreads / kLanes;   // 4 x 64 blocks per workgroup of icp_global_bound
static_assert(kOccTile == tbnav_rk::kTS, "a field tile is a tile of the filter's pool");
static_assert(kMargin >= kPoolMaxS && (1 << 5) == kPoolMaxS, "q <= 5");

struct FieldArgs {
  const unsigned int* bm;      // TilePool::bm
  const unsigned int* table;   // [N][TT] the particles' tile tables
  const int* best;             // the filter's arg-max on the device, read where particle < 0
  int particle, TW, TT, side, P, k;
};

// blockIdx.x: the tile along ci (the map's rows), blockIdx.y: along cj (the bits of a word)
__global__ __launch_bounds__(kThreads) void icp_global_field(FieldArgs a, const uint8_t* __restrict__ value, uint8_t* __restrict__ lik,
                                                             GlobalRec* __restrict__ rec) {
  __shared__ unsigned long long s_occ[kOccRows];   // row r: map row X0 - kOccHalo + r; bit b: map column Y0 - kOccHalo + b
  __shared__ uint8_t s_val[kMapValues];
  const int tid = threadIdx.x;
  const int X0 = (int)blockIdx.x * kOccTile, Y0 = (int)blockIdx.y * kOccTile;
  const unsigned int* __restrict__ ids = a.table + (size_t)(a.particle < 0 ? *a.best : a.particle) * a.TT;
  int any = 0;
  if (tid < kLanes) {
    unsigned long long win = 0ull;
    if (tid < kOccRows) {
      win = occ_row_window(a.bm, ids, a.TW, a.side, X0 - kOccHalo + tid, Y0 - kOccHalo);
      s_occ[tid] = win;
      any = win != 0ull;
    }
    // the tile's own cells (rows and columns outside the map are empty in the window already)
    uint32_t cnt = 0u;
    if (tid >= kOccHalo && tid < kOccHalo + kOccTile) cnt = (uint32_t)__popcll(win & (0xffffffffull << kOccHalo));
    cnt = wave_sum_u32(cnt);
    if (tid == 0 && cnt) atomicAdd(&rec->occupied, cnt);
  }
  if (tid < kMapValues) s_val[tid] = value[tid];
  any = __syncthreads_or(any);
  if (!any) return;                                 // (the map was zeroed before the launch)
  const int k = a.k, c_max = 2 * k * k;
  const int ly = tid & (kOccTile - 1), cj = Y0 + ly;
#pragma unroll
  for (int j = 0; j < kOccTile * kOccTile / kThreads; ++j) {
    const int lx = (tid >> 5) + j * (kThreads / kOccTile), ci = X0 + lx;
    if (ci >= a.side || cj >= a.side) continue;     // a ragged tile
    const int d2 = nearest_occ_d2(s_occ, lx, ly + kOccHalo, k);
    lik[(size_t)(ci + kMargin) * a.P + (cj + kMargin)] = d2 <= c_max ? s_val[d2] : (uint8_t)0;
  }
}

// out[pi][pj] = max over a, b < s of in[pi + a][pj + b] over the whole padded map (beyond it: 0); one workgroup per kPoolI x kPoolJ
__global__ __launch_bounds__(kThreads) void icp_global_pool(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int P, int s) {
  constexpr int kW = kPoolJ + kPoolMaxS - 1, kH = kPoolI + kPoolMaxS - 1, kStride = kW + 1;
  __shared__ uint8_t s_in[kH * kStride];
  __shared__ uint8_t s_row[kH * kPoolJ];
  const int tid = threadIdx.x;
  const int I0 = (int)blockIdx.x * kPoolI, J0 = (int)blockIdx.y * kPoolJ;
  const int w = kPoolJ + s - 1, hgt = kPoolI + s - 1;
  for (int idx = tid; idx < hgt * w; idx += kThreads) {
    const int r = idx / w, c = idx - r * w;
    const int gi = I0 + r, gj = J0 + c;
    s_in[r * kStride + c] = gi < P && gj < P ? in[(size_t)gi * P + gj] : (uint8_t)0;
  }
  __syncthreads();
  for (int idx = tid; idx < hgt * kPoolJ; idx += kThreads) {
    const int r = idx / kPoolJ, c = idx - r * kPoolJ;
    unsigned int m = 0u;
    for (int b = 0; b < s; ++b) m = max(m, (unsigned int)s_in[r * kStride + c + b]);
    s_row[idx] = (uint8_t)m;
  }
  __syncthreads();
  for (int idx = tid; idx < kPoolI * kPoolJ; idx += kThreads) {
    const int r = idx / kPoolJ, c = idx - r * kPoolJ;
    unsigned int m = 0u;
    for (int b = 0; b < s; ++b) m = max(m, (unsigned int)s_row[(r + b) * kPoolJ + c]);
    if (I0 + r < P && J0 + c < P) out[(size_t)(I0 + r) * P + (J0 + c)] = (uint8_t)m;
  }
}

// blockIdx.x: the heading.  off [NA][n_beams], cnt [NA]
__global__ __launch_bounds__(kThreads) void icp_global_offsets(const float* __restrict__ scan, const float2* __restrict__ beams, int n_beams,
                                                               IcpConst k, const double2* __restrict__ rot, double inv, int side,
                                                               uint32_t* __restrict__ off, uint32_t* __restrict__ cnt,
                                                               GlobalRec* __restrict__ rec) {
  __shared__ uint32_t s_n, s_valid;
  const int tid = threadIdx.x, ia = blockIdx.x;
  if (tid == 0) { s_n = 0u; s_valid = 0u; }
  __syncthreads();
  const double2 cs = rot[ia];
  const int lim = side + kMargin;                    // an offset this far out reads zero from every cell of the map, in lik and in pool
  uint32_t valid = 0u;
  for (int i = tid; i < n_beams; i += kThreads) {
    float2 p;
    if (!cloud_point(scan[i], beams[i], k, p)) continue;
    ++valid;
    const double sx = (double)p.x, sy = (double)p.y;
    const double vx = ((((cs.x * sx) - (cs.y * sy))) * inv) + 0.5;
    const double vy = ((((cs.y * sx) + (cs.x * sy))) * inv) + 0.5;
    if (!(vx >= -65536.0 && vx <= 65536.0 && vy >= -65536.0 && vy <= 65536.0)) continue;
    const int ox = (int)floor(vx), oy = (int)floor(vy);
    if (ox <= -lim || ox >= lim || oy <= -lim || oy >= lim) continue;
    off[(size_t)ia * n_beams + atomicAdd(&s_n, 1u)] = ((uint32_t)ox & 0xffffu) | ((uint32_t)oy << 16);
  }
  if (ia == 0) {
    valid = wave_sum_u32(valid);
    if ((tid & (kLanes - 1)) == 0 && valid) atomicAdd(&s_valid, valid);
  }
  __syncthreads();
  if (tid == 0) {
    cnt[ia] = s_n;
    if (ia == 0) rec->points = s_valid;
  }
}

// blockIdx.x: the tile of blocks, tile_x * tiles_y + tile_y; blockIdx.y: the heading.  A wave is one Bx, its lanes 64 By.
__global__ __launch_bounds__(kThreads) void icp_global_bound(SearchArgs a, int tiles_y, const uint8_t* __restrict__ pool,
                                                             const uint32_t* __restrict__ off, const uint32_t* __restrict__ cnt,
                                                             uint32_t* __restrict__ bounds, GlobalRec* __restrict__ rec) {
  __shared__ uint32_t s_off[TBNAV_ICP_MAX_BEAMS];
  const int tid = threadIdx.x, ia = blockIdx.y;
  const int tile_x = (int)blockIdx.x / tiles_y, tile_y = (int)blockIdx.x - tile_x * tiles_y;
  const int n = (int)min(cnt[ia], (uint32_t)a.n_beams);
  for (int i = tid; i < n; i += kThreads) s_off[i] = off[(size_t)ia * a.n_beams + i];
  __syncthreads();
  const int Bx = tile_x * kBoundBx + (tid >> 6), By = tile_y * kLanes + (tid & (kLanes - 1));
  const bool live = Bx < a.nbx && By < a.nby;
  uint32_t sum = 0u;
  if (live) {
    const int bx = a.tx0 + (Bx << a.q), by = a.ty0 + (By << a.q);
    for (int p = 0; p < n; ++p) {
      const uint32_t o = s_off[p];
      const int x = clamp_cell(bx + off_x(o), a.side), y = clamp_cell(by + off_y(o), a.side);
      sum += pool[(size_t)(x + kMargin) * a.P + (y + kMargin)];
    }
    bounds[((size_t)ia * a.nbx + Bx) * a.nby + By] = sum;
  }
  uint32_t m = sum;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o, 64));
  if ((tid & (kLanes - 1)) == 0 && m) atomicMax(&rec->maxb, m);
}

// the bin of a bound: its leading bits below the largest bound's highest
__host__ __device__ inline int hist_shift(uint32_t maxb) {
  int bits = 0;
  while (bits < 32 && (maxb >> bits) != 0u) ++bits;
  return bits > 10 ? bits - 10 : 0;
}

__global__ __launch_bounds__(kThreads) void icp_global_hist(const uint32_t* __restrict__ bounds, long long blocks,
                                                            const GlobalRec* __restrict__ rec, uint32_t* __restrict__ hist) {
  __shared__ uint32_t s_hist[kHistBins];
  const int tid = threadIdx.x;
  for (int i = tid; i < kHistBins; i += kThreads) s_hist[i] = 0u;
  __syncthreads();
  const int shift = hist_shift(rec->maxb);
  for (long long i = (long long)blockIdx.x * kThreads + tid; i < blocks; i += (long long)gridDim.x * kThreads)
    atomicAdd(&s_hist[bounds[i] >> shift], 1u);
  __syncthreads();
  for (int i = tid; i < kHistBins; i += kThreads)
    if (s_hist[i]) atomicAdd(&hist[i], s_hist[i]);
}

__global__ __launch_bounds__(kThreads) void icp_global_list(const uint32_t* __restrict__ bounds, long long blocks, unsigned long long lo,
                                                            unsigned long long hi, uint32_t* __restrict__ list, uint32_t cap,
                                                            GlobalRec* __restrict__ rec) {
  for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < blocks; i += (long long)gridDim.x * kThreads) {
    const unsigned long long b = bounds[i];
    if (b >= lo && b < hi) {
      const uint32_t slot = atomicAdd(&rec->nlist, 1u);
      if (slot < cap) list[slot] = (uint32_t)i;
    }
  }
}

// blockIdx.x: the place in the list (list == nullptr: the block itself).  scores: [NA][w][h], or nullptr
__global__ __launch_bounds__(kThreads) void icp_global_refine(SearchArgs a, const uint8_t* __restrict__ lik, const uint32_t* __restrict__ off,
                                                              const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ bounds,
                                                              const uint32_t* __restrict__ list, uint32_t cap, GlobalRec* __restrict__ rec,
                                                              uint32_t* __restrict__ scores) {
  __shared__ uint32_t s_off[TBNAV_ICP_MAX_BEAMS];
  const int tid = threadIdx.x;
  uint32_t blk = blockIdx.x;
  if (list) {
    if (blk >= min(rec->nlist, cap)) return;
    blk = list[blk];
  }
  const int per = a.nbx * a.nby;
  const int ia = (int)(blk / (uint32_t)per), r = (int)(blk - (uint32_t)ia * (uint32_t)per);
  const int Bx = r / a.nby, By = r - Bx * a.nby;
  const int bx = a.tx0 + (Bx << a.q), by = a.ty0 + (By << a.q);
  if (bounds[blk] == 0u) {
    // every score of the block is 0: its first candidate holds its key (a hook's volume was zeroed before the launch)
    if (tid == 0) atomicMax(&rec->key, (unsigned long long)(~(uint32_t)(((uint32_t)ia * a.side + bx) * a.side + by)));
    return;
  }
  const int n = (int)min(cnt[ia], (uint32_t)a.n_beams);
  for (int i = tid; i < n; i += blockDim.x) s_off[i] = off[(size_t)ia * a.n_beams + i];
  __syncthreads();
  unsigned long long key = 0ull;
  for (int c = tid; c < a.s * a.s; c += blockDim.x) {
    const int tx = bx + (c >> a.q), ty = by + (c & (a.s - 1));
    if (tx >= a.tx0 + a.w || ty >= a.ty0 + a.h) continue;          // a ragged block
    uint32_t sum = 0u;
    for (int p = 0; p < n; ++p) {
      const uint32_t o = s_off[p];
      const int x = clamp_cell(tx + off_x(o), a.side), y = clamp_cell(ty + off_y(o), a.side);
      sum += lik[(size_t)(x + kMargin) * a.P + (y + kMargin)];
    }
    if (scores) scores[((size_t)ia * a.w + (tx - a.tx0)) * a.h + (ty - a.ty0)] = sum;
    const unsigned long long cand = ((unsigned long long)sum << 32) | (uint32_t)~(((uint32_t)ia * a.side + tx) * a.side + ty);
    key = cand > key ? cand : key;
  }
  key = wave_max_u64(key);
  if ((tid & (kLanes - 1)) == 0 && key) atomicMax(&rec->key, key);
}

// ---- the host ----
struct Plan {
  tbnav_icp_global_params gp;
  tbnav_icp_search_params sp;
  SearchArgs a;
  int NA;
  long long blocks;
  uint8_t value[kMapValues];
};

bool global_params_ok(const tbnav_icp_global_params& p) {
  if (p.ang_count < 1 || p.ang_count > TBNAV_ICP_GLOBAL_MAX_ANG || !std::isfinite(p.ang_step) || !std::isfinite(p.min_quality)) return false;
  return p.pool_log2 >= 1 && p.pool_log2 <= 5 && p.reserved == 0;
}

// L1.  with_scan: the entry takes a scan.  Nothing is changed.
int prepare(const tbnav_icp* h, const tbnav_rbpf* pf, int32_t particle, bool with_scan, const float* scan, int32_t n_beams,
            const tbnav_icp_global_params* params, Plan& pl) {
  if (!h || !pf) return TBNAV_ERR_INVALID_ARG;
  if (with_scan && (!scan || n_beams <= 0 || n_beams > TBNAV_ICP_MAX_BEAMS)) return TBNAV_ERR_INVALID_ARG;
  if (params) pl.gp = *params; else tbnav_icp_default_global_params(&pl.gp);
  if (!global_params_ok(pl.gp)) return TBNAV_ERR_INVALID_ARG;
  pl.sp = h->search.p;
  if (!search_params_ok(pl.sp) || pl.sp.resolution != pf->p.resolution) return TBNAV_ERR_INVALID_ARG;
  if (!tbnav_nk::particle_ok(pf, particle)) return TBNAV_ERR_INVALID_ARG;
  const int side = pf->xsize;
  const int32_t* rg = pl.gp.region;
  int tx0 = 0, ty0 = 0, tx1 = side - 1, ty1 = side - 1;
  if (!(rg[0] == -1 && rg[1] == -1 && rg[2] == -1 && rg[3] == -1)) {
    if (!(0 <= rg[0] && rg[0] <= rg[2] && rg[2] < side && 0 <= rg[1] && rg[1] <= rg[3] && rg[3] < side)) return TBNAV_ERR_INVALID_ARG;
    tx0 = rg[0]; ty0 = rg[1]; tx1 = rg[2]; ty1 = rg[3];
  }
  if (h->device != pf->device || pf->comm) return TBNAV_ERR_UNSUPPORTED;
  if (side > TBNAV_ICP_GLOBAL_MAX_SIDE || pf->ysize != side) return TBNAV_ERR_UNSUPPORTED;
  SearchArgs& a = pl.a;
  a.side = side;
  a.P = (side + 2 * kMargin + 63) & ~63;
  a.q = pl.gp.pool_log2;
  a.s = 1 << a.q;
  a.tx0 = tx0; a.ty0 = ty0; a.w = tx1 - tx0 + 1; a.h = ty1 - ty0 + 1;
  a.nbx = (a.w + a.s - 1) >> a.q;
  a.nby = (a.h + a.s - 1) >> a.q;
  a.n_beams = with_scan ? n_beams : 0;
  pl.NA = pl.gp.ang_count;
  pl.blocks = (long long)pl.NA * a.nbx * a.nby;
  if (pl.blocks > (long long)TBNAV_ICP_GLOBAL_MAX_BLOCKS) return TBNAV_ERR_UNSUPPORTED;
  return map_value_table(pl.sp, pl.value);
}

enum Stage { kField, kBounds, kScores, kFull };

struct Run {
  GlobalRec rec{};
  long long refined = 0;
  int rounds = 0;
  float* ms = nullptr;      // tbnav_icp_localize_map_timed: the stages' times, or null
  uint32_t hist[kHistBins] = {};   // a full search's seeding histogram, for the hypotheses behind it
};

// Optional event timing of a timed call's stages: stage i lies between stamps i and i + 1 (stamps 5 / 6 and 8 / 9 have the host's
// reads between them: no stage).  Where no times are asked for no event exists and every call does nothing.
struct Stamps {
  static constexpr int kN = 12;
  hipEvent_t ev[kN] = {};
  hipStream_t stream;
  bool on;
  bool set[kN] = {};
  Stamps(bool on_, hipStream_t st) : stream(st), on(on_) {}
  ~Stamps() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
  hipError_t stamp(int i) {
    if (!on) return hipSuccess;
    if (!ev[i]) { const hipError_t e = hipEventCreate(&ev[i]); if (e != hipSuccess) return e; }
    set[i] = true;
    return hipEventRecord(ev[i], stream);
  }
  // (once the stream has been waited for) 0 where either stamp was not taken
  float between(int i, int j) const {
    float ms = 0.0f;
    if (on && set[i] && set[j] && hipEventElapsedTime(&ms, ev[i], ev[j]) != hipSuccess) ms = 0.0f;
    return ms;
  }
};

int read_rec(tbnav_icp* h, GlobalRec* rec, uint32_t* hist) {
  IcpGlobal& G = h->global;
  TBNAV_HIP(hipMemcpyAsync(rec, G.d_rec.ptr, sizeof(GlobalRec), hipMemcpyDeviceToHost, h->stream));
  if (hist) TBNAV_HIP(hipMemcpyAsync(hist, G.d_rec.as<unsigned char>() + sizeof(GlobalRec), sizeof(uint32_t) * kHistBins, hipMemcpyDeviceToHost, h->stream));
  TBNAV_HIP(hipStreamSynchronize(h->stream));
  return TBNAV_OK;
}

// one round: the blocks with lo <= bound < hi (at most cap of them) listed and refined
int refine_round(tbnav_icp* h, const Plan& pl, unsigned long long lo, unsigned long long hi, long long cap, uint32_t* scores, Stamps& st,
                 int first_stamp) {
  IcpGlobal& G = h->global;
  GlobalRec* rec = G.d_rec.as<GlobalRec>();
  if (int rc = G.d_list.reserve(sizeof(uint32_t) * (size_t)cap)) return rc;
  TBNAV_HIP(hipMemsetAsync(&rec->nlist, 0, sizeof(uint32_t), h->stream));
  TBNAV_HIP(st.stamp(first_stamp));
  const long long want = (pl.blocks + kThreads - 1) / kThreads;
  hipLaunchKernelGGL(icp_global_list, dim3((unsigned)(want < 4096 ? want : 4096)), dim3(kThreads), 0, h->stream, G.d_bounds.as<uint32_t>(),
                     pl.blocks, lo, hi, G.d_list.as<uint32_t>(), (uint32_t)cap, rec);
  TBNAV_HIP(st.stamp(first_stamp + 1));
  const int threads = pl.a.s * pl.a.s >= kThreads ? kThreads : (pl.a.s * pl.a.s > kLanes ? pl.a.s * pl.a.s : kLanes);
  hipLaunchKernelGGL(icp_global_refine, dim3((unsigned)cap), dim3(threads), 0, h->stream, pl.a, G.d_lik.as<uint8_t>(), G.d_off.as<uint32_t>(),
                     G.d_cnt.as<uint32_t>(), G.d_bounds.as<uint32_t>(), G.d_list.as<uint32_t>(), (uint32_t)cap, rec, scores);
  TBNAV_HIP(hipGetLastError());
  TBNAV_HIP(st.stamp(first_stamp + 2));
  return TBNAV_OK;
}

int run(tbnav_icp* h, tbnav_rbpf* pf, int32_t particle, const float* scan, int32_t n_beams, const Plan& pl, Stage stage, Run& out) {
  IcpGlobal& G = h->global;
  IcpSearch& S = h->search;
  const SearchArgs& a = pl.a;
  const size_t map_bytes = (size_t)a.P * a.P;
  if (int rc = G.d_lik.reserve(map_bytes)) return rc;
  if (int rc = G.d_pool.reserve(map_bytes)) return rc;
  if (int rc = G.d_rec.reserve(sizeof(GlobalRec) + sizeof(uint32_t) * kHistBins)) return rc;
  const size_t in_bytes = (size_t)kMapValues + sizeof(double2) * (size_t)pl.NA;
  if (int rc = G.d_in.reserve(in_bytes)) return rc;
  G.h_in.resize(in_bytes);
  std::memcpy(G.h_in.data(), pl.value, (size_t)kMapValues);
  double2* rot = reinterpret_cast<double2*>(G.h_in.data() + kMapValues);
  for (int ia = 0; ia < pl.NA; ++ia) {
    const double th = (double)ia * pl.gp.ang_step;
    rot[ia] = make_double2(std::cos(th), std::sin(th));
  }
  if (stage != kField) {
    if (int rc = ensure_table(h, n_beams)) return rc;
    if (int rc = G.d_scan.reserve(sizeof(float) * (size_t)n_beams)) return rc;
    if (int rc = G.d_off.reserve(sizeof(uint32_t) * (size_t)pl.NA * (size_t)n_beams)) return rc;
    if (int rc = G.d_cnt.reserve(sizeof(uint32_t) * (size_t)pl.NA)) return rc;
    if (int rc = G.d_bounds.reserve(sizeof(uint32_t) * (size_t)pl.blocks)) return rc;
    TBNAV_HIP(hipMemcpyAsync(G.d_scan.ptr, scan, sizeof(float) * (size_t)n_beams, hipMemcpyHostToDevice, h->stream));
  }
  TBNAV_HIP(hipMemcpyAsync(G.d_in.ptr, G.h_in.data(), in_bytes, hipMemcpyHostToDevice, h->stream));
  // L8: behind whatever the filter has in flight, the arg-max of its weights included where it is asked for
  if (int rc = tbnav_nk::enqueue_best(pf, particle)) return rc;
  if (!S.map_ev) TBNAV_HIP(hipEventCreateWithFlags(&S.map_ev, hipEventDisableTiming));
  TBNAV_HIP(hipEventRecord(S.map_ev, pf->stream));
  TBNAV_HIP(hipStreamWaitEvent(h->stream, S.map_ev, 0));

  GlobalRec* rec = G.d_rec.as<GlobalRec>();
  uint32_t* d_hist = reinterpret_cast<uint32_t*>(G.d_rec.as<unsigned char>() + sizeof(GlobalRec));
  TBNAV_HIP(hipMemsetAsync(G.d_rec.ptr, 0, sizeof(GlobalRec) + sizeof(uint32_t) * kHistBins, h->stream));
  Stamps st(out.ms != nullptr, h->stream);
  TBNAV_HIP(st.stamp(0));
  TBNAV_HIP(hipMemsetAsync(G.d_lik.ptr, 0, map_bytes, h->stream));
  const FieldArgs fa{pf->pool.bm, pf->d_table[pf->cur], pf->d_best, particle, pf->TW, pf->TT, a.side, a.P, pl.sp.stamp_cells};
  hipLaunchKernelGGL(icp_global_field, dim3(pf->TW, pf->TW), dim3(kThreads), 0, h->stream, fa, G.d_in.as<uint8_t>(), G.d_lik.as<uint8_t>(), rec);
  TBNAV_HIP(st.stamp(1));
  hipLaunchKernelGGL(icp_global_pool, dim3((a.P + kPoolI - 1) / kPoolI, (a.P + kPoolJ - 1) / kPoolJ), dim3(kThreads), 0, h->stream,
                     G.d_lik.as<uint8_t>(), G.d_pool.as<uint8_t>(), a.P, a.s);
  TBNAV_HIP(hipGetLastError());
  TBNAV_HIP(st.stamp(2));
  if (stage == kField) return read_rec(h, &out.rec, nullptr);

  const double2* d_rot = reinterpret_cast<const double2*>(G.d_in.as<unsigned char>() + kMapValues);
  hipLaunchKernelGGL(icp_global_offsets, dim3(pl.NA), dim3(kThreads), 0, h->stream, G.d_scan.as<float>(), h->d_table, n_beams, h->k, d_rot,
                     1.0 / pl.sp.resolution, a.side, G.d_off.as<uint32_t>(), G.d_cnt.as<uint32_t>(), rec);
  TBNAV_HIP(st.stamp(3));
  const int tiles_x = (a.nbx + kBoundBx - 1) / kBoundBx, tiles_y = (a.nby + kLanes - 1) / kLanes;
  hipLaunchKernelGGL(icp_global_bound, dim3(tiles_x * tiles_y, pl.NA), dim3(kThreads), 0, h->stream, a, tiles_y, G.d_pool.as<uint8_t>(),
                     G.d_off.as<uint32_t>(), G.d_cnt.as<uint32_t>(), G.d_bounds.as<uint32_t>(), rec);
  TBNAV_HIP(hipGetLastError());
  TBNAV_HIP(st.stamp(4));
  if (stage == kBounds) return read_rec(h, &out.rec, nullptr);

  if (stage == kScores) {
    // the refinement kernel over all blocks, unlisted
    uint32_t* d_scores = G.d_scores.as<uint32_t>();
    TBNAV_HIP(hipMemsetAsync(d_scores, 0, sizeof(uint32_t) * (size_t)pl.NA * a.w * a.h, h->stream));
    const int threads = a.s * a.s >= kThreads ? kThreads : (a.s * a.s > kLanes ? a.s * a.s : kLanes);
    hipLaunchKernelGGL(icp_global_refine, dim3((unsigned)pl.blocks), dim3(threads), 0, h->stream, a, G.d_lik.as<uint8_t>(), G.d_off.as<uint32_t>(),
                       G.d_cnt.as<uint32_t>(), G.d_bounds.as<uint32_t>(), (const uint32_t*)nullptr, 0u, rec, d_scores);
    TBNAV_HIP(hipGetLastError());
    return read_rec(h, &out.rec, nullptr);
  }

  const long long want = (pl.blocks + kThreads - 1) / kThreads;
  hipLaunchKernelGGL(icp_global_hist, dim3((unsigned)(want < 2048 ? want : 2048)), dim3(kThreads), 0, h->stream, G.d_bounds.as<uint32_t>(), pl.blocks,
                     rec, d_hist);
  TBNAV_HIP(hipGetLastError());
  TBNAV_HIP(st.stamp(5));
  uint32_t* hist = out.hist;
  if (int rc = read_rec(h, &out.rec, hist)) return rc;
  // round 1, the seeds: every block of the highest bins that together hold kSeeds blocks
  const int shift = hist_shift(out.rec.maxb);
  const long long need = pl.blocks < kSeeds ? pl.blocks : kSeeds;
  long long seeds = 0;
  int b0 = kHistBins;
  while (b0 > 0 && seeds < need) seeds += hist[--b0];
  const unsigned long long seed_lo = (unsigned long long)b0 << shift;
  if (int rc = refine_round(h, pl, seed_lo, 1ull << 32, seeds, nullptr, st, 6)) return rc;
  if (int rc = read_rec(h, &out.rec, nullptr)) return rc;
  out.rounds = 1;
  out.refined = seeds;
  // round 2, the survivors: what the seeds' best score does not rule out (L6: a bound that equals it is refined)
  const unsigned long long best = out.rec.key >> 32;
  if (best < seed_lo) {
    long long cap = 0;
    for (int b = (int)(best >> shift); b < b0; ++b) cap += hist[b];
    if (cap > 0) {
      if (int rc = refine_round(h, pl, best, seed_lo, cap, nullptr, st, 9)) return rc;
      if (int rc = read_rec(h, &out.rec, nullptr)) return rc;
      if (out.rec.nlist > 0) {
        out.rounds = 2;
        out.refined += out.rec.nlist;
      }
    }
  }
  if (out.ms) {
    const int from[TBNAV_ICP_GLOBAL_STAGES] = {0, 1, 2, 3, 4, 6, 7, 9, 10};
    for (int i = 0; i < TBNAV_ICP_GLOBAL_STAGES; ++i) out.ms[i] = st.between(from[i], from[i] + 1);
  }
  return TBNAV_OK;
}

const char* const kAllKernels =
    "icp_global_field;icp_global_pool;icp_global_offsets;icp_global_bound;icp_global_hist;icp_global_list;icp_global_refine";
const char* const kHypKernels =
    "icp_global_field;icp_global_pool;icp_global_offsets;icp_global_bound;icp_global_hist;icp_global_list;icp_global_refine;"
    "icp_hyp_collect;icp_hyp_knock;icp_hyp_select";

// ---- HYPOTHESES (H1-H10): the global search above, then icp_hyp.hip's launches behind one more list ----
bool hyp_params_ok(const tbnav_icp_hyp_params& p) {
  return p.max_hyp >= 1 && p.max_hyp <= TBNAV_ICP_HYP_MAX && p.floor_q10 >= 1 && p.floor_q10 <= 1024 && p.sep_cells >= 0 && p.sep_cells <= 64 &&
         p.sep_steps >= 0 && p.sep_steps <= TBNAV_ICP_GLOBAL_MAX_ANG && (p.wrap == 0 || p.wrap == 1) && p.reserved == 0;
}

struct HypOut {
  tbnav_icp_hyp_info info{};
  std::vector<unsigned long long> keys;      // the first n peaks, in order
  std::vector<unsigned long long> cands;     // the hook's: every candidate's key, and its peak flag
  std::vector<uint8_t> flags;
  const char* kernels = kAllKernels;
};

// H1-H7 for one call; nothing of the handle but its buffers is changed
int hyp_run(tbnav_icp* h, tbnav_rbpf* pf, int32_t particle, const float* scan, int32_t n_beams, const tbnav_icp_global_params* gparams,
            const tbnav_icp_hyp_params* hparams, bool want_cands, Plan& pl, HypOut& out) {
  tbnav_icp_hyp_params hp;
  if (hparams) hp = *hparams; else tbnav_icp_default_hyp_params(&hp);
  if (!hyp_params_ok(hp)) return TBNAV_ERR_INVALID_ARG;
  if (int rc = prepare(h, pf, particle, true, scan, n_beams, gparams, pl)) return rc;
  const SearchArgs& a = pl.a;
  HypArgs ha{};
  ha.NA = pl.NA; ha.Ba = hp.sep_steps + 1; ha.B = hp.sep_cells + 1;
  ha.nba = (pl.NA + ha.Ba - 1) / ha.Ba; ha.nbbx = (a.w + ha.B - 1) / ha.B; ha.nbby = (a.h + ha.B - 1) / ha.B;
  ha.sep_cells = hp.sep_cells; ha.sep_steps = hp.sep_steps; ha.wrap = hp.wrap; ha.K = hp.max_hyp;
  const long long bins = (long long)ha.nba * ha.nbbx * ha.nbby;
  if (bins > (long long)TBNAV_ICP_HYP_MAX_BINS) return TBNAV_ERR_UNSUPPORTED;
  DeviceGuard guard(h->device);
  if (!guard.ok) return TBNAV_ERR_NO_DEVICE;
  Run r;
  if (int rc = run(h, pf, particle, scan, n_beams, pl, kFull, r)) return rc;
  tbnav_icp_hyp_info& info = out.info;
  info.searched = 1;
  info.best_score = (uint32_t)(r.rec.key >> 32);
  info.points = (int32_t)r.rec.points;
  info.occupied = (int32_t)r.rec.occupied;
  info.blocks = pl.blocks;
  info.refined_blocks = r.refined;
  info.rounds = r.rounds;
  if (info.best_score == 0u) return TBNAV_OK;                        // H2: empty
  const unsigned long long t = ((unsigned long long)info.best_score * (unsigned long long)hp.floor_q10 + 1023ull) >> 10;
  ha.t = (uint32_t)t;
  // the histogram's bins from t's upwards hold every block with bound >= t: what the list and the launch are sized by
  const int shift = hist_shift(r.rec.maxb);
  long long ub = 0;
  for (int b = (int)(t >> shift); b < kHistBins; ++b) ub += r.hist[b];
  if (ub < 1) ub = 1;
  ha.list_cap = (uint32_t)(ub < (long long)TBNAV_ICP_HYP_MAX_REFINE ? ub : (long long)TBNAV_ICP_HYP_MAX_REFINE);
  const unsigned long long cc = (unsigned long long)ha.list_cap * (unsigned long long)(a.s * a.s);
  ha.cand_cap = (uint32_t)(cc < (unsigned long long)TBNAV_ICP_HYP_MAX_CANDIDATES ? cc : (unsigned long long)TBNAV_ICP_HYP_MAX_CANDIDATES);
  IcpGlobal& G = h->global;
  IcpHyp& Y = h->hyp;
  if (int rc = G.d_list.reserve(sizeof(uint32_t) * (size_t)ha.list_cap)) return rc;
  if (int rc = Y.d_cands.reserve(sizeof(unsigned long long) * (size_t)ha.cand_cap)) return rc;
  if (int rc = Y.d_peaks.reserve(sizeof(unsigned long long) * (size_t)ha.cand_cap)) return rc;
  if (int rc = Y.d_flags.reserve((size_t)ha.cand_cap)) return rc;
  if (int rc = Y.d_bins.reserve(sizeof(unsigned long long) * (size_t)bins)) return rc;
  if (int rc = Y.d_alive.reserve((size_t)bins)) return rc;
  if (int rc = Y.d_rec.reserve(sizeof(HypRec))) return rc;
  GlobalRec* rec = G.d_rec.as<GlobalRec>();
  TBNAV_HIP(hipMemsetAsync(&rec->nlist, 0, sizeof(uint32_t), h->stream));
  const long long want = (pl.blocks + kThreads - 1) / kThreads;
  hipLaunchKernelGGL(icp_global_list, dim3((unsigned)(want < 4096 ? want : 4096)), dim3(kThreads), 0, h->stream, G.d_bounds.as<uint32_t>(),
                     pl.blocks, t, 1ull << 32, G.d_list.as<uint32_t>(), ha.list_cap, rec);
  TBNAV_HIP(hipGetLastError());
  const int threads = a.s * a.s >= kThreads ? kThreads : (a.s * a.s > kLanes ? a.s * a.s : kLanes);
  if (int rc = hyp_enqueue(h->stream, a, ha, threads, G.d_lik.as<uint8_t>(), G.d_off.as<uint32_t>(), G.d_cnt.as<uint32_t>(),
                           G.d_list.as<uint32_t>(), rec, Y.d_cands.as<unsigned long long>(), Y.d_flags.as<uint8_t>(),
                           Y.d_peaks.as<unsigned long long>(), Y.d_bins.as<unsigned long long>(), Y.d_alive.as<uint8_t>(), Y.d_rec.as<HypRec>()))
    return rc;
  HypRec hr;
  GlobalRec gr;
  TBNAV_HIP(hipMemcpyAsync(&gr, rec, sizeof gr, hipMemcpyDeviceToHost, h->stream));
  TBNAV_HIP(hipMemcpyAsync(&hr, Y.d_rec.ptr, sizeof hr, hipMemcpyDeviceToHost, h->stream));
  TBNAV_HIP(hipStreamSynchronize(h->stream));
  if (gr.nlist > (uint32_t)TBNAV_ICP_HYP_MAX_REFINE) return TBNAV_ERR_UNSUPPORTED;          // H6, in this order
  if (hr.ncand > (uint32_t)TBNAV_ICP_HYP_MAX_CANDIDATES) return TBNAV_ERR_UNSUPPORTED;
  if (gr.nlist > ha.list_cap || hr.ncand > ha.cand_cap || hr.npeaks > hr.ncand) return TBNAV_ERR_HIP;   // (the sizes above hold them)
  info.floor_score = ha.t;
  info.floor_blocks = gr.nlist;
  // the blocks the rounds refined and the floor's blocks are both "every block with a bound of at least ...": one holds the other
  if (info.floor_blocks > info.refined_blocks) info.refined_blocks = info.floor_blocks;
  info.rounds = r.rounds + 1;
  info.candidates = hr.ncand;
  info.n_peaks = (int32_t)hr.npeaks;
  info.n = info.n_peaks < hp.max_hyp ? info.n_peaks : hp.max_hyp;
  out.keys.assign(hr.keys, hr.keys + info.n);
  out.kernels = kHypKernels;
  if (want_cands) {
    out.cands.resize(hr.ncand);
    out.flags.resize(hr.ncand);
    TBNAV_HIP(hipMemcpy(out.cands.data(), Y.d_cands.ptr, sizeof(unsigned long long) * (size_t)hr.ncand, hipMemcpyDeviceToHost));
    TBNAV_HIP(hipMemcpy(out.flags.data(), Y.d_flags.ptr, (size_t)hr.ncand, hipMemcpyDeviceToHost));
  }
  return TBNAV_OK;
}

}  // namespace

namespace tbnav_icpdev {

void global_free(tbnav_icp* h) {
  IcpGlobal& G = h->global;
  for (DevBuf* b : {&G.d_lik, &G.d_pool, &G.d_in, &G.d_scan, &G.d_off, &G.d_cnt, &G.d_bounds, &G.d_list, &G.d_scores, &G.d_rec}) b->release();
  IcpHyp& Y = h->hyp;
  for (DevBuf* b : {&Y.d_cands, &Y.d_flags, &Y.d_peaks, &Y.d_bins, &Y.d_alive, &Y.d_rec}) b->release();
}

}  // namespace tbnav_icpdev

extern "C" {

void tbnav_icp_default_global_params(tbnav_icp_global_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof *p);
  p->ang_step = 3.14159265358979323846 / 180.0;
  p->min_quality = 0.5;
  p->ang_count = 360;
  p->pool_log2 = 3;
  for (int i = 0; i < 4; ++i) p->region[i] = -1;
}

int tbnav_icp_localize_map(tbnav_icp* h, tbnav_rbpf* pf, int32_t particle, const float* scan, int32_t n_beams,
                           const tbnav_icp_global_params* params, tbnav_icp_global_info* info) {
  return tbnav_icp_localize_map_timed(h, pf, particle, scan, n_beams, params, info, nullptr);
}

int tbnav_icp_localize_map_timed(tbnav_icp* h, tbnav_rbpf* pf, int32_t particle, const float* scan, int32_t n_beams,
                                 const tbnav_icp_global_params* params, tbnav_icp_global_info* info, float* stage_ms) {
  if (!info) return TBNAV_ERR_INVALID_ARG;
  Plan pl;
  if (int rc = prepare(h, pf, particle, true, scan, n_beams, params, pl)) return rc;
  DeviceGuard guard(h->device);
  if (!guard.ok) return TBNAV_ERR_NO_DEVICE;
  Run r;
  r.ms = stage_ms;
  if (int rc = run(h, pf, particle, scan, n_beams, pl, kFull, r)) return rc;
  const SearchArgs& a = pl.a;
  tbnav_icp_global_info out{};
  const uint32_t lin = ~(uint32_t)r.rec.key;
  out.score = (uint32_t)(r.rec.key >> 32);
  out.ia = (int32_t)(lin / ((uint32_t)a.side * (uint32_t)a.side));
  out.tx = (int32_t)((lin / (uint32_t)a.side) % (uint32_t)a.side);
  out.ty = (int32_t)(lin % (uint32_t)a.side);
  out.points = (int32_t)r.rec.points;
  out.occupied = (int32_t)r.rec.occupied;
  out.T[0] = (double)out.ia * pl.gp.ang_step;
  out.T[1] = pf->p.xmin + ((double)out.tx + 0.5) * pl.sp.resolution;
  out.T[2] = pf->p.ymin + ((double)out.ty + 0.5) * pl.sp.resolution;
  out.quality = out.points > 0 ? (double)out.score / (255.0 * (double)out.points) : 0.0;
  out.accepted = out.quality >= pl.gp.min_quality && out.points > 0 && out.occupied > 0;
  out.blocks = pl.blocks;
  out.refined_blocks = r.refined;
  out.rounds = r.rounds;
  out.searched = 1;
  *info = out;
  h->global.last = out;
  h->global.kernels = kAllKernels;
  return TBNAV_OK;
}

int tbnav_icp_last_global(const tbnav_icp* h, tbnav_icp_global_info* info) {
  if (!h || !info) return TBNAV_ERR_INVALID_ARG;
  *info = h->global.last;
  return TBNAV_OK;
}

int tbnav_icp_last_global_kernels(const tbnav_icp* h, char* buf, int32_t cap) {
  if (!h || !buf || cap <= 0) return TBNAV_ERR_INVALID_ARG;
  std::snprintf(buf, (size_t)cap, "%s", h->global.kernels);
  return TBNAV_OK;
}

int tbnav_icp_localize_map_field(tbnav_icp* h, tbnav_rbpf* pf, int32_t particle, const tbnav_icp_global_params* params, uint8_t* lik,
                                 uint8_t* pool, int32_t* occupied) {
  if (!lik || !pool || !occupied) return TBNAV_ERR_INVALID_ARG;
  Plan pl;
  if (int rc = prepare(h, pf, particle, false, nullptr, 0, params, pl)) return rc;
  DeviceGuard guard(h->device);
  if (!guard.ok) return TBNAV_ERR_NO_DEVICE;
  Run r;
  if (int rc = run(h, pf, particle, nullptr, 0, pl, kField, r)) return rc;
  const SearchArgs& a = pl.a;
  std::vector<uint8_t> m((size_t)a.P * a.P);
  TBNAV_HIP(hipMemcpy(m.data(), h->global.d_lik.ptr, m.size(), hipMemcpyDeviceToHost));
  for (int ci = 0; ci < a.side; ++ci) std::memcpy(lik + (size_t)ci * a.side, m.data() + (size_t)(ci + kMargin) * a.P + kMargin, (size_t)a.side);
  // the margin is part of what the field kernel owes the gathers: all zero
  for (int pi = 0; pi < a.P; ++pi)
    for (int pj = 0; pj < a.P; ++pj) {
      const bool in = pi >= kMargin && pi < kMargin + a.side && pj >= kMargin && pj < kMargin + a.side;
      if (!in && m[(size_t)pi * a.P + pj] != 0) return TBNAV_ERR_HIP;
    }
  TBNAV_HIP(hipMemcpy(m.data(), h->global.d_pool.ptr, m.size(), hipMemcpyDeviceToHost));
  const int e = a.s - 1, ps = a.side + e;
  for (int i = 0; i < ps; ++i) std::memcpy(pool + (size_t)i * ps, m.data() + (size_t)(i - e + kMargin) * a.P + (kMargin - e), (size_t)ps);
  *occupied = (int32_t)r.rec.occupied;
  return TBNAV_OK;
}

int tbnav_icp_localize_map_bounds(tbnav_icp* h, tbnav_rbpf* pf, int32_t particle, const float* scan, int32_t n_beams,
                                  const tbnav_icp_global_params* params, uint32_t* bounds) {
  if (!bounds) return TBNAV_ERR_INVALID_ARG;
  Plan pl;
  if (int rc = prepare(h, pf, particle, true, scan, n_beams, params, pl)) return rc;
  DeviceGuard guard(h->device);
  if (!guard.ok) return TBNAV_ERR_NO_DEVICE;
  Run r;
  if (int rc = run(h, pf, particle, scan, n_beams, pl, kBounds, r)) return rc;
  TBNAV_HIP(hipMemcpy(bounds, h->global.d_bounds.ptr, sizeof(uint32_t) * (size_t)pl.blocks, hipMemcpyDeviceToHost));
  return TBNAV_OK;
}

int tbnav_icp_localize_map_scores(tbnav_icp* h, tbnav_rbpf* pf, int32_t particle, const float* scan, int32_t n_beams,
                                  const tbnav_icp_global_params* params, uint32_t* scores) {
  if (!scores) return TBNAV_ERR_INVALID_ARG;
  Plan pl;
  if (int rc = prepare(h, pf, particle, true, scan, n_beams, params, pl)) return rc;
  const long long cands = (long long)pl.NA * pl.a.w * pl.a.h;
  if (cands > (long long)TBNAV_ICP_GLOBAL_MAX_HOOK_SCORES) return TBNAV_ERR_UNSUPPORTED;
  DeviceGuard guard(h->device);
  if (!guard.ok) return TBNAV_ERR_NO_DEVICE;
  if (int rc = h->global.d_scores.reserve(sizeof(uint32_t) * (size_t)cands)) return rc;
  Run r;
  if (int rc = run(h, pf, particle, scan, n_beams, pl, kScores, r)) return rc;
  TBNAV_HIP(hipMemcpy(scores, h->global.d_scores.ptr, sizeof(uint32_t) * (size_t)cands, hipMemcpyDeviceToHost));
  return TBNAV_OK;
}

void tbnav_icp_default_hyp_params(tbnav_icp_hyp_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof *p);
  p->max_hyp = 8;
  p->floor_q10 = 768;
  p->sep_cells = 8;
  p->sep_steps = 10;
  p->wrap = 1;
}

int tbnav_icp_localize_map_hyp(tbnav_icp* h, tbnav_rbpf* pf, int32_t particle, const float* scan, int32_t n_beams,
                               const tbnav_icp_global_params* gparams, const tbnav_icp_hyp_params* hparams, tbnav_icp_hypothesis* hyps,
                               int32_t cap, tbnav_icp_hyp_info* info) {
  if (!hyps || !info || cap < 1) return TBNAV_ERR_INVALID_ARG;
  Plan pl;
  HypOut out;
  if (int rc = hyp_run(h, pf, particle, scan, n_beams, gparams, hparams, false, pl, out)) return rc;
  const uint32_t side = (uint32_t)pl.a.side;
  for (int i = 0; i < out.info.n && i < cap; ++i) {
    tbnav_icp_hypothesis y{};
    const uint32_t lin = ~(uint32_t)out.keys[i];
    y.score = (uint32_t)(out.keys[i] >> 32);
    y.ia = (int32_t)(lin / (side * side));
    y.tx = (int32_t)((lin / side) % side);
    y.ty = (int32_t)(lin % side);
    y.T[0] = (double)y.ia * pl.gp.ang_step;
    y.T[1] = pf->p.xmin + ((double)y.tx + 0.5) * pl.sp.resolution;
    y.T[2] = pf->p.ymin + ((double)y.ty + 0.5) * pl.sp.resolution;
    y.quality = out.info.points > 0 ? (double)y.score / (255.0 * (double)out.info.points) : 0.0;
    y.accepted = y.quality >= pl.gp.min_quality && out.info.points > 0 && out.info.occupied > 0;
    hyps[i] = y;
  }
  *info = out.info;
  h->hyp.last = out.info;
  h->hyp.kernels = out.kernels;
  return TBNAV_OK;
}

int tbnav_icp_last_hyp(const tbnav_icp* h, tbnav_icp_hyp_info* info) {
  if (!h || !info) return TBNAV_ERR_INVALID_ARG;
  *info = h->hyp.last;
  return TBNAV_OK;
}

int tbnav_icp_last_hyp_kernels(const tbnav_icp* h, char* buf, int32_t cap) {
  if (!h || !buf || cap <= 0) return TBNAV_ERR_INVALID_ARG;
  std::snprintf(buf, (size_t)cap, "%s", h->hyp.kernels);
  return TBNAV_OK;
}

int tbnav_icp_localize_map_hyp_candidates(tbnav_icp* h, tbnav_rbpf* pf, int32_t particle, const float* scan, int32_t n_beams,
                                          const tbnav_icp_global_params* gparams, const tbnav_icp_hyp_params* hparams, uint32_t* index,
                                          uint32_t* score, uint8_t* peak, int64_t cap, int64_t* count) {
  if (!count || cap < 0 || (cap > 0 && (!index || !score || !peak))) return TBNAV_ERR_INVALID_ARG;
  Plan pl;
  HypOut out;
  if (int rc = hyp_run(h, pf, particle, scan, n_beams, gparams, hparams, true, pl, out)) return rc;
  const size_t n = out.cands.size();
  std::vector<uint32_t> order(n);
  for (size_t i = 0; i < n; ++i) order[i] = (uint32_t)i;
  std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return (uint32_t)~out.cands[x] < (uint32_t)~out.cands[y]; });
  for (size_t i = 0; i < n && (int64_t)i < cap; ++i) {
    index[i] = ~(uint32_t)out.cands[order[i]];
    score[i] = (uint32_t)(out.cands[order[i]] >> 32);
    peak[i] = out.flags[order[i]];
  }
  *count = (int64_t)n;
  return TBNAV_OK;
}

}  // extern "C"

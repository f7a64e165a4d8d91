// icp_search_wide.hip — the wide second stage of the correlative search (include/tbnav_icp.h, WIDE WINDOW, items W1-W8; an
// addition with no counterpart in the reference).  The first stage keeps the whole table, padded by its window, in LDS and so
// stops at +-16 cells; a window of up to +-64 cells and +-180 steps is TILED instead: brute force, exact by construction, all
// integer or fp64 without contraction (-ffp-contract=off, csrc/Makefile), restated in tests/icp_search_wide_restatement.py.
//   icp_search_wide_score   one workgroup of 256 threads per (translation tile, angle, pair).  A tile is up to 33 x 33
//                           translations (kTile); shifting every base cell by the tile's first offset turns the tile into a
//                           window 0 .. ts-1, so the workgroup needs the table with ts-1 zero cells on its HIGH side only: a
//                           slice of side n + ts - 1 <= 208 in LDS, read from the first stage's padded table in global memory
//                           (icp_search_table wrote it: there is no second table kernel).  A shifted base cell inside the
//                           table goes to the fast list; one up to ts-1 cells below it, whose tile is only partly inside, to a
//                           bounds-tested slow list as its shifted coordinates + (ts-1), 0 .. 207 each: 8 bits hold them
//                           because they are relative to the TILE, not to the window (by + W would reach 303).  One
//                           translation at a time, the points innermost (icp_search_shape's loop).  mode 0 / 1 reduce one
//                           64-bit key per workgroup (S6; pass 1 against thr), mode 2 the integers of F3 for the chosen angle's
//                           tiles, one partial record per tile that the host adds (integers have no order).
//   icp_search_wide_select  one workgroup per pair: the maximum of its tiles x angles keys, the candidate count and thr.
// Key (S6 in one max-reduction): a score is below 2^20, D <= 180^2 + 2 * 64^2 below 2^16, the linear index below 361 * 129^2,
// so below 2^23: rank = D << 23 | lin has 39 bits.  Pass 0: score << 39 | ~rank.  Pass 1: ~rank << 25 | score.
// On the host wide_stage runs the escalated pairs of one chunk of search_pairs (icp_search.hip) in sub-launches of at most
// kWideGroups workgroups and synchronises once.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "icp_device.hpp"
#include "icp_search_device.hpp"
#include "tbnav_icp.h"

namespace {

using namespace tbnav_icpdev;

constexpr int kTile = 33;           // translations per axis and tile: the first stage's largest window, 5 per thread
constexpr int kWideGroups = 16384;  // workgroups of one scoring launch at the most (the chunk bound)
constexpr int kRankBits = 39, kLinBits = 23, kScoreBits = 25;
constexpr int kSums = 7;            // S0, Sx, Sy, Sxx, Sxy, Syy, cells
static_assert(TBNAV_ICP_SEARCH_WIDE_MAX_TABLE + kTile - 1 <= TBNAV_ICP_SEARCH_MAX_SIDE, "the slice does not fit where the first stage's table does");
static_assert(TBNAV_ICP_SEARCH_WIDE_MAX_TABLE + kTile - 1 <= 256, "a slow-list coordinate does not fit in 8 bits");
static_assert((TBNAV_ICP_SEARCH_WIDE_MAX_TABLE - 1) * TBNAV_ICP_SEARCH_MAX_SIDE + TBNAV_ICP_SEARCH_WIDE_MAX_TABLE <= 65536, "a fast-list cell does not fit in 16 bits");
static_assert((2 * TBNAV_ICP_SEARCH_WIDE_MAX_ANG + 1) * (2 * TBNAV_ICP_SEARCH_WIDE_MAX_LIN + 1) * (2 * TBNAV_ICP_SEARCH_WIDE_MAX_LIN + 1) < (1 << kLinBits), "the linear index does not fit");
static_assert(TBNAV_ICP_SEARCH_WIDE_MAX_ANG * TBNAV_ICP_SEARCH_WIDE_MAX_ANG + 2 * TBNAV_ICP_SEARCH_WIDE_MAX_LIN * TBNAV_ICP_SEARCH_WIDE_MAX_LIN < (1 << (kRankBits - kLinBits)), "D does not fit");
static_assert(TBNAV_ICP_MAX_BEAMS * 255 < (1 << 20), "a score does not fit");

struct WideConst {
  double E, inv;
  int n;                 // the table's side
  int side0, pad0;       // the first stage's padded table in global memory: its side and its border (the first stage's lin_cells)
  int tab_stride;        // bytes of one of those
  int W, A, nl, na;      // nl = 2W + 1, na = 2A + 1
  int nt, ts;            // tiles per axis, translations per axis and tile (<= kTile)
  int stride, rows;      // the LDS slice: rows = n + ts - 1, each stride = rows rounded up to 4 bytes long
  int slice_bytes;       // stride * rows rounded up to 16
  unsigned slack;
};

// what one (pair, angle, tile) workgroup leaves
struct WideRec {
  unsigned long long key;
  uint32_t count, points;
};

// blockIdx.x: the tile; blockIdx.y: the angle (mode 2: the chosen one, from sel); blockIdx.z: the pair of this launch, w0 + z of
// the chunk's escalated pairs, whose place in the chunk (pairs, tables) is idx[w0 + z].
// mode 0: key = (score, inverted rank), count = the candidates at this workgroup's best score.  mode 1: among score >= thr,
// key = (inverted rank, score), count = how many they are.  mode 2: the tile's part of F3's integers -> shape.
__global__ __launch_bounds__(kThreads) void icp_search_wide_score(const float* __restrict__ scans, const float* __restrict__ stored,
                                                                  const float2* __restrict__ beams, int n_beams,
                                                                  const SearchPair* __restrict__ pairs, const int* __restrict__ idx,
                                                                  const double2* __restrict__ rot, const uint8_t* __restrict__ tables,
                                                                  const SearchSel* __restrict__ sel, WideRec* __restrict__ rec,
                                                                  uint32_t* __restrict__ scores, ShapeRec* __restrict__ shape, IcpConst k,
                                                                  WideConst wc, int w0, int mode, unsigned drop) {
  extern __shared__ uint4 lds_tab[];                                    // the slice, then the cells
  uint32_t* words = reinterpret_cast<uint32_t*>(lds_tab);
  const uint8_t* tab = reinterpret_cast<const uint8_t*>(lds_tab);
  uint16_t* cells = reinterpret_cast<uint16_t*>(lds_tab + wc.slice_bytes / 16);  // [n_beams]: fast list up from 0, slow list down from the end
  __shared__ uint32_t n_fast, n_slow, n_valid;
  __shared__ unsigned long long red_key[kThreads / kWave];
  __shared__ uint32_t red_cnt[kThreads / kWave];
  __shared__ long long red_sum[kThreads / kWave][kSums + 1];
  const int t = threadIdx.x;
  const int tile = blockIdx.x, z = blockIdx.z, wi = w0 + z;
  const int pi = idx[wi];
  const int n_win = wc.nl * wc.nl;
  // the slice: table rows 0 .. n-1 from the first stage's padded table, zero to the right of and below them
  {
    const uint8_t* g = tables + (size_t)pi * (size_t)wc.tab_stride + (size_t)(wc.pad0 * wc.side0 + wc.pad0);
    const int wpr = wc.stride / 4;
    for (int i = t; i < wc.slice_bytes / 4; i += kThreads) {
      const int row = i / wpr, c = (i - row * wpr) * 4;
      uint32_t v = 0u;
      if (row < wc.n && c < wc.n) {
        const uint8_t* s = g + row * wc.side0 + c;
        if (c + 4 <= wc.n) {
          __builtin_memcpy(&v, s, 4);
        } else {
          for (int b = 0; c + b < wc.n; ++b) v |= (uint32_t)s[b] << (8 * b);
        }
      }
      words[i] = v;
    }
  }
  if (t == 0) { n_fast = 0u; n_slow = 0u; n_valid = 0u; }
  __syncthreads();
  const SearchSel choice = mode ? sel[wi] : SearchSel{};
  int ia = blockIdx.y;
  if (mode == 2) {
    ia = (int)(choice.lin / (uint32_t)n_win);
    ia = ia < wc.na ? ia : wc.na - 1;                                   // lin < na * nl^2 by construction; never index past rot
  }
  const int ty = tile / wc.nt, tx = tile - ty * wc.nt;
  const int iy0 = ty * wc.ts, ix0 = tx * wc.ts;                         // the tile's first translation in the window
  const int th = wc.nl - iy0 < wc.ts ? wc.nl - iy0 : wc.ts;
  const int tw = wc.nl - ix0 < wc.ts ? wc.nl - ix0 : wc.ts;
  const SearchPair pr = pairs[pi];
  const double2 cs = rot[(size_t)wi * wc.na + ia];
  const float* ss = pr.src < 0 ? stored : scans + (size_t)pr.src * n_beams;
  // base cells, shifted by the tile's first offset: the tile reads rows by .. by + th - 1, columns bx .. bx + tw - 1
  uint32_t valid = 0u;
  const int reach = wc.ts - 1;
  for (int i = t; i < n_beams; i += kThreads) {
    float2 p;
    if (!cloud_point(ss[i], beams[i], k, p)) continue;
    ++valid;
    const double sx = (double)p.x, sy = (double)p.y;
    const double ax = (((cs.x * sx) - (cs.y * sy)) + pr.x0);
    const double ay = (((cs.y * sx) + (cs.x * sy)) + pr.y0);
    int bx, by;
    if (!cell_of(ax, wc.E, wc.inv, bx) || !cell_of(ay, wc.E, wc.inv, by)) continue;
    bx += ix0 - wc.W;
    by += iy0 - wc.W;
    if (bx >= 0 && bx < wc.n && by >= 0 && by < wc.n) {
      cells[atomicAdd(&n_fast, 1u)] = (uint16_t)(by * wc.stride + bx);
    } else if (bx >= -reach && bx < wc.n && by >= -reach && by < wc.n) {
      cells[n_beams - 1 - (int)atomicAdd(&n_slow, 1u)] = (uint16_t)(((by + reach) << 8) | (bx + reach));
    }
  }
  if (valid) atomicAdd(&n_valid, valid);
  __syncthreads();
  const int nf = (int)n_fast, ns = (int)n_slow;
  const int n_cand = th * tw;
  const int per = (n_cand + kThreads - 1) / kThreads;                   // 1 .. 5, the same for every thread
  const uint32_t best_sel = choice.score;
  const uint32_t thr = mode == 1 ? choice.thr : 0u;
  const uint32_t floor_ = best_sel - (uint32_t)(((unsigned long long)best_sel * drop) >> 10);
  unsigned long long key = 0ull;
  uint32_t top = 0u, cnt = 0u;                                          // mode 0: this thread's best score and how often it has it
  long long s[kSums] = {0, 0, 0, 0, 0, 0, 0};
  for (int j = 0; j < per; ++j) {
    const int q = t + j * kThreads;
    const bool in = q < n_cand;
    const int ly = in ? q / tw : 0;
    const int lx = in ? q - ly * tw : 0;
    const int off = ly * wc.stride + lx;                                // a slot past the tile reads translation 0's cells and is dropped
    uint32_t acc = 0u;
#pragma unroll 8
    for (int p = 0; p < nf; ++p) acc += tab[(int)cells[p] + off];
    for (int p = 0; p < ns; ++p) {
      const int v = cells[n_beams - 1 - p];
      const int ry = (v >> 8) - reach + ly, rx = (v & 0xff) - reach + lx;
      if (ry >= 0 && ry < wc.n && rx >= 0 && rx < wc.n) acc += tab[ry * wc.stride + rx];
    }
    if (!in) continue;
    const int iy = iy0 + ly, ix = ix0 + lx;
    const int dy = iy - wc.W, dx = ix - wc.W;
    if (mode == 2) {
      if (acc <= floor_) continue;
      const long long w = (long long)(acc - floor_);
      s[0] += w;
      s[1] += w * dx;
      s[2] += w * dy;
      s[3] += w * dx * dx;
      s[4] += w * dx * dy;
      s[5] += w * dy * dy;
      s[6] += 1;
      continue;
    }
    const uint32_t lin = (uint32_t)((ia * wc.nl + iy) * wc.nl + ix);
    if (scores && mode == 0) scores[(size_t)z * wc.na * n_win + lin] = acc;
    const int da = ia - wc.A;
    const unsigned long long rank = ((unsigned long long)(uint32_t)(da * da + dy * dy + dx * dx) << kLinBits) | lin;
    const unsigned long long inv_rank = (~rank) & ((1ull << kRankBits) - 1ull);
    unsigned long long kj;
    if (mode == 1) {
      if (acc < thr) continue;
      ++cnt;
      kj = (inv_rank << kScoreBits) | acc;
    } else {
      kj = ((unsigned long long)acc << kRankBits) | inv_rank;
      if (cnt == 0u || acc > top) { top = acc; cnt = 1u; }
      else if (acc == top) ++cnt;
    }
    key = kj > key ? kj : key;
  }
  if (mode == 2) {
#pragma unroll
    for (int i = 0; i < kSums; ++i) {
      s[i] = wave_sum_i64(s[i]);
      if ((t & (kWave - 1)) == 0) red_sum[t / kWave][i] = s[i];
    }
    __syncthreads();
    if (t == 0) {
#pragma unroll
      for (int i = 0; i < kSums; ++i) {
        s[i] = red_sum[0][i];
#pragma unroll
        for (int w = 1; w < kThreads / kWave; ++w) s[i] += red_sum[w][i];
      }
      ShapeRec r;
      r.S0 = s[0]; r.Sx = s[1]; r.Sy = s[2]; r.Sxx = s[3]; r.Sxy = s[4]; r.Syy = s[5];
      r.cells = (uint32_t)s[6];
      r.pad0 = 0u;
      r.pad1 = 0;
      shape[(size_t)z * gridDim.x + tile] = r;
    }
    return;
  }
  // the workgroup's maximum, then (mode 0) how many of its candidates reach that score
  key = wave_max_u64(key);
  if ((t & (kWave - 1)) == 0) red_key[t / kWave] = key;
  __syncthreads();
  key = red_key[0];
#pragma unroll
  for (int w = 1; w < kThreads / kWave; ++w) key = red_key[w] > key ? red_key[w] : key;
  if (mode == 0 && top != (uint32_t)(key >> kRankBits)) cnt = 0u;
  cnt = wave_sum_u32(cnt);
  if ((t & (kWave - 1)) == 0) red_cnt[t / kWave] = cnt;
  __syncthreads();
  if (t == 0) {
    WideRec r;
    r.key = key;
    r.count = 0u;
#pragma unroll
    for (int w = 0; w < kThreads / kWave; ++w) r.count += red_cnt[w];
    r.points = n_valid;
    rec[((size_t)z * gridDim.y + blockIdx.y) * gridDim.x + tile] = r;
  }
}

// one workgroup per pair of the launch: its n_rec = tiles * na records -> the chosen candidate, sel[w0 + blockIdx.x]
__global__ __launch_bounds__(kThreads) void icp_search_wide_select(const WideRec* __restrict__ rec, int n_rec, const int* __restrict__ idx,
                                                                   const uint32_t* __restrict__ tgt_points, SearchSel* __restrict__ sel,
                                                                   WideConst wc, int w0, int pass) {
  __shared__ unsigned long long red_key[kThreads / kWave];
  __shared__ uint32_t red_cnt[kThreads / kWave];
  const int t = threadIdx.x, wi = w0 + blockIdx.x;
  const WideRec* r = rec + (size_t)blockIdx.x * n_rec;
  unsigned long long key = 0ull;
  for (int a = t; a < n_rec; a += kThreads) key = r[a].key > key ? r[a].key : key;
  key = wave_max_u64(key);
  if ((t & (kWave - 1)) == 0) red_key[t / kWave] = key;
  __syncthreads();
  key = red_key[0];
#pragma unroll
  for (int w = 1; w < kThreads / kWave; ++w) key = red_key[w] > key ? red_key[w] : key;
  uint32_t cnt = 0u;
  for (int a = t; a < n_rec; a += kThreads)
    if (pass || (r[a].key >> kRankBits) == (key >> kRankBits)) cnt += r[a].count;
  cnt = wave_sum_u32(cnt);
  if ((t & (kWave - 1)) == 0) red_cnt[t / kWave] = cnt;
  __syncthreads();
  if (t == 0) {
    SearchSel s;
    // pass 1 with nothing at or above thr cannot happen: the best candidate itself is
    const unsigned long long inv_rank = pass ? key >> kScoreBits : key & ((1ull << kRankBits) - 1ull);
    s.score = pass ? (uint32_t)(key & ((1ull << kScoreBits) - 1ull)) : (uint32_t)(key >> kRankBits);
    s.lin = (uint32_t)((~inv_rank) & ((1ull << kLinBits) - 1ull));
    s.count = 0u;
#pragma unroll
    for (int w = 0; w < kThreads / kWave; ++w) s.count += red_cnt[w];
    s.points = r[0].points;
    s.tgt_points = tgt_points[idx[wi]];
    s.thr = pass ? sel[wi].thr : s.score - (uint32_t)(((unsigned long long)s.score * wc.slack) >> 10);
    sel[wi] = s;
  }
}

WideConst make_wide(const SearchConst& sc, const tbnav_icp_search_wide_params& wp) {
  WideConst wc;
  wc.E = sc.E; wc.inv = sc.inv;
  wc.n = sc.n; wc.side0 = sc.side; wc.pad0 = sc.wl; wc.tab_stride = sc.tab_stride;
  wc.W = wp.lin_cells; wc.A = wp.ang_steps;
  wc.nl = 2 * wc.W + 1; wc.na = 2 * wc.A + 1;
  wc.nt = (wc.nl + kTile - 1) / kTile;
  wc.ts = (wc.nl + wc.nt - 1) / wc.nt;
  wc.rows = wc.n + wc.ts - 1;
  wc.stride = (wc.rows + 3) & ~3;
  wc.slice_bytes = (wc.stride * wc.rows + 15) & ~15;
  wc.slack = sc.slack;
  return wc;
}

size_t wide_lds_bytes(const WideConst& wc, int n_beams) {
  return (size_t)wc.slice_bytes + ((sizeof(uint16_t) * (size_t)n_beams + 15) & ~(size_t)15);
}

}  // namespace

namespace tbnav_icpdev {

bool wide_params_ok(const tbnav_icp_search_wide_params& wp, const tbnav_icp_search_params& sp) {
  if (wp.lin_cells < 1 || wp.lin_cells > TBNAV_ICP_SEARCH_WIDE_MAX_LIN || wp.ang_steps < 0 || wp.ang_steps > TBNAV_ICP_SEARCH_WIDE_MAX_ANG ||
      wp.when < TBNAV_ICP_WIDE_ON_REJECT || wp.when > TBNAV_ICP_WIDE_ALWAYS)
    return false;
  if (wp.lin_cells < sp.lin_cells || wp.ang_steps < sp.ang_steps) return false;
  const double cells = std::ceil(sp.half_extent / sp.resolution);
  return cells >= 1.0 && 2.0 * cells <= (double)TBNAV_ICP_SEARCH_WIDE_MAX_TABLE;
}

int wide_stage(tbnav_icp* h, int first, const std::vector<int>& esc, int n_beams, const tbnav_icp_search_params& sp,
               const SearchConst& sc, const SearchPair* d_pairs, const tbnav_icp_search_wide_params& wp, uint32_t* scores,
               const tbnav_icp_search_shape_params* shp) {
  IcpSearch& S = h->search;
  const int m = (int)esc.size();
  if (m == 0) return TBNAV_OK;
  if (!wide_params_ok(wp, sp) || (scores && m != 1)) return TBNAV_ERR_INVALID_ARG;
  const WideConst wc = make_wide(sc, wp);
  const int tiles = wc.nt * wc.nt, n_rec = tiles * wc.na;
  const int per_launch = kWideGroups / n_rec > 0 ? kWideGroups / n_rec : 1;   // pairs of one scoring launch
  const int lm = m < per_launch ? m : per_launch;
  const size_t vol = (size_t)wc.na * wc.nl * wc.nl;
  // one upload: the escalated pairs' places in the chunk, then (16-byte aligned) their rotations over the wide angles
  const size_t rot_at = (sizeof(int) * (size_t)m + 15) & ~(size_t)15;
  S.h_win.resize(rot_at + sizeof(double2) * (size_t)m * wc.na);
  int* hi = reinterpret_cast<int*>(S.h_win.data());
  double2* hr = reinterpret_cast<double2*>(S.h_win.data() + rot_at);
  for (int j = 0; j < m; ++j) {
    hi[j] = esc[(size_t)j];
    const std::array<double, 3>& T = h->h_init[(size_t)(first + esc[(size_t)j])];
    for (int ia = 0; ia < wc.na; ++ia) {
      const double th = T[0] + (double)(ia - wc.A) * sp.ang_step;
      hr[(size_t)j * wc.na + ia] = make_double2(std::cos(th), std::sin(th));
    }
  }
  const std::pair<DevBuf*, size_t> want[] = {{&S.d_win, S.h_win.size()},
                                             {&S.d_wrec, sizeof(WideRec) * (size_t)lm * n_rec},
                                             {&S.d_wsel, sizeof(SearchSel) * (size_t)m},
                                             {&S.d_wshape, shp ? sizeof(ShapeRec) * (size_t)m * tiles : 0},
                                             {&S.d_wscores, scores ? sizeof(uint32_t) * vol : 0}};
  for (const auto& w : want)
    if (int rc = w.first->reserve(w.second)) return rc;
  TBNAV_HIP(hipMemcpyAsync(S.d_win.ptr, S.h_win.data(), S.h_win.size(), hipMemcpyHostToDevice, h->stream));
  const int* d_idx = S.d_win.as<int>();
  const double2* d_rot = reinterpret_cast<const double2*>(S.d_win.as<unsigned char>() + rot_at);
  const size_t lds = wide_lds_bytes(wc, n_beams);
  const unsigned drop = shp ? (unsigned)shp->drop_q10 : 0u;
  auto score = [&](int w0, int cnt, int mode) {
    hipLaunchKernelGGL(icp_search_wide_score, dim3(tiles, mode == 2 ? 1 : wc.na, cnt), dim3(kThreads), lds, h->stream,
                       h->d_scans.as<float>(), h->d_stored.as<float>(), h->d_table, n_beams, d_pairs, d_idx, d_rot,
                       S.d_tables.as<uint8_t>(), S.d_wsel.as<SearchSel>(), S.d_wrec.as<WideRec>(),
                       scores && mode == 0 ? S.d_wscores.as<uint32_t>() : nullptr,
                       S.d_wshape.as<ShapeRec>() + (size_t)w0 * tiles, h->k, wc, w0, mode, drop);
  };
  for (int w0 = 0; w0 < m; w0 += per_launch) {
    const int cnt = m - w0 < per_launch ? m - w0 : per_launch;
    for (int pass = 0; pass < (wc.slack ? 2 : 1); ++pass) {
      score(w0, cnt, pass);
      TBNAV_HIP(hipGetLastError());
      hipLaunchKernelGGL(icp_search_wide_select, dim3(cnt), dim3(kThreads), 0, h->stream, S.d_wrec.as<WideRec>(), n_rec, d_idx,
                         S.d_tgt_points.as<uint32_t>(), S.d_wsel.as<SearchSel>(), wc, w0, pass);
      TBNAV_HIP(hipGetLastError());
    }
    if (shp) {
      score(w0, cnt, 2);
      TBNAV_HIP(hipGetLastError());
    }
  }
  S.h_wsel.resize(sizeof(SearchSel) * (size_t)m);
  TBNAV_HIP(hipMemcpyAsync(S.h_wsel.data(), S.d_wsel.ptr, S.h_wsel.size(), hipMemcpyDeviceToHost, h->stream));
  if (shp) {
    S.h_wshape.resize(sizeof(ShapeRec) * (size_t)m * tiles);
    TBNAV_HIP(hipMemcpyAsync(S.h_wshape.data(), S.d_wshape.ptr, S.h_wshape.size(), hipMemcpyDeviceToHost, h->stream));
  }
  if (scores) TBNAV_HIP(hipMemcpyAsync(scores, S.d_wscores.ptr, sizeof(uint32_t) * vol, hipMemcpyDeviceToHost, h->stream));
  TBNAV_HIP(hipStreamSynchronize(h->stream));
  // S7 (and F4 / F5) over the wide window: the first stage's host code with wl := W, wa := A
  tbnav_icp_search_params spw = sp;
  spw.lin_cells = wp.lin_cells;
  spw.ang_steps = wp.ang_steps;
  SearchConst scw = sc;
  scw.wl = wc.W; scw.wa = wc.A; scw.nl = wc.nl; scw.na = wc.na;
  for (int j = 0; j < m; ++j) {
    const size_t at = (size_t)(first + esc[(size_t)j]);
    const double* T_init = h->h_init[at].data();
    tbnav_icp_search_info* info = &h->h_sinfo[at];
    search_finish(reinterpret_cast<const SearchSel*>(S.h_wsel.data())[j], scw, spw, T_init, info);
    h->h_sshape[at] = tbnav_icp_search_shape{};
    if (shp) {
      const ShapeRec* part = reinterpret_cast<const ShapeRec*>(S.h_wshape.data()) + (size_t)j * tiles;
      ShapeRec r{};
      for (int q = 0; q < tiles; ++q) {
        r.S0 += part[q].S0; r.Sx += part[q].Sx; r.Sy += part[q].Sy;
        r.Sxx += part[q].Sxx; r.Sxy += part[q].Sxy; r.Syy += part[q].Syy;
        r.cells += part[q].cells;
      }
      shape_finish(r, spw, *shp, T_init, info, &h->h_sshape[at]);
    }
  }
  return TBNAV_OK;
}

}  // namespace tbnav_icpdev

extern "C" {

void tbnav_icp_default_search_wide_params(tbnav_icp_search_wide_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof *p);
  p->lin_cells = 48;
  p->ang_steps = 45;
  p->when = TBNAV_ICP_WIDE_ON_REJECT;
}

int tbnav_icp_set_search_wide(tbnav_icp* h, const tbnav_icp_search_wide_params* params) {
  if (!h) return TBNAV_ERR_INVALID_ARG;
  if (!params) {
    h->search.wide_on = false;
    tbnav_icp_default_search_wide_params(&h->search.wide_p);
    return TBNAV_OK;
  }
  if (!tbnav_icpdev::wide_params_ok(*params, h->search.p)) return TBNAV_ERR_INVALID_ARG;
  h->search.wide_p = *params;
  h->search.wide_p.reserved = 0;
  h->search.wide_on = true;
  return TBNAV_OK;
}

int tbnav_icp_get_search_wide(const tbnav_icp* h, int32_t* on, tbnav_icp_search_wide_params* params) {
  if (!h) return TBNAV_ERR_INVALID_ARG;
  if (on) *on = h->search.wide_on ? 1 : 0;
  if (params) *params = h->search.wide_p;
  return TBNAV_OK;
}

int tbnav_icp_last_search_wide(const tbnav_icp* h, tbnav_icp_search_wide_info* info) {
  if (!h || !info) return TBNAV_ERR_INVALID_ARG;
  *info = h->search.last_wide;
  return TBNAV_OK;
}

}  // extern "C"

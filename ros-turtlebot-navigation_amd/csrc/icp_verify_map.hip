// icp_verify_map.hip — the check of a pose against the walls and the free space of a filter particle's MAP (include/tbnav_icp.h, MAP
// CHECK, items V1-V10; an addition with no counterpart in the reference; restated in tests/icp_verify_map_restatement.py and reproduced
// bit for bit).  What the searches and the alignment do not ask: does a beam pass through a wall the map holds, does it end in space
// the map knows to be empty?
//   icp_verify_map<P>  one workgroup of 256 threads per pair, in icp_align_map's shape.
//     Staging: three bitmaps of the window's 2H x 2H cells into LDS — OCCUPIED, FREE, UNKNOWN — row r = map row sx - H + r, one zero
//     word in front of and one behind each row's ceil(2H / 32) words (icp_align_map's layout: at most 3 x 256 x 10 words, 30 KB).
//     OCCUPIED comes through occ_row_window.  FREE and UNKNOWN come from the log-odds, read through the particle's tile table a map
//     word (32 cells of one tile row, contiguous) at a time: a wave64 takes two such words, classifies against the cuts and packs with
//     two ballots (nav_gain_classes' way), four pairs of words in flight; a tile with id 0 is all-UNKNOWN without a read; tiles and
//     rows outside the map and the columns of a ragged last tile are in neither.  The map-aligned words land in the rows' own slots
//     and are then shifted to the window's origin in place, a row per thread.
//     Walk: thread t takes beams t, t + 256, ... (P of them): the end cell, G17's steps by a carried remainder (the integers of the
//     closed form), G18's corner rule, V6's counts, then V5's D by rows outwards (clz / ffs on a masked 64-bit look).
//     Counts: wave sums (wave.hpp), four partial rows in LDS, thread 0 adds them and writes the record.  No atomics.
// Compiled with -ffp-contract=off (csrc/Makefile).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "icp_device.hpp"
#include "icp_search_device.hpp"
#include "nav_host.hpp"
#include "tbnav_icp.h"

namespace {

using namespace tbnav_icpdev;

constexpr int kCounts = 9;     // points, outside, hit, through, missing, unseen, undecided, free_cells, unknown_cells
constexpr int kLanes = tbnav_icpdev::kWave, kWaves = kThreads / kLanes;
constexpr int kInFlight = 4;   // pairs of map words a wave has loads out for at once (16 was measured and was slower: DESIGN.md §4)

struct VerifyMapArgs {
  const double* lo;            // TilePool::lo
  const unsigned int* bm;      // TilePool::bm
  const unsigned int* table;   // [N][TT] the particles' tile tables
  const int* best;             // the filter's arg-max on the device (rbpf_argmax), read where a pair asks for it
  int TW, TT, side;            // tiles per side and per map, cells per side
  double xmin, ymin, inv;      // A2
  double half_lo, half_hi, free_cut;   // ExportCuts (G10)
  int H, k;                    // V1a
  int max_through, max_missing, min_hit;
};

struct VerifyMapPair {
  int32_t particle;            // a slot, or TBNAV_ICP_MAP_BEST_PARTICLE
  int32_t sx, sy;              // the sensor cell (V3)
  int32_t pad;
  double c, s, x, y;           // item 2's float-rounded pose
};

// 64 bits of window row `row` (its first pad word included) from bit position p
__device__ __forceinline__ unsigned long long look(const uint32_t* row, int p) {
  const int w = p >> 5, o = p & 31;
  return ((((unsigned long long)row[w + 1]) << 32) | row[w]) >> o;
}

// bit of local cell (r, c) in a staged bitmap
__device__ __forceinline__ bool bit_at(const uint32_t* map, int W, int r, int c) { return (map[r * W + 1 + (c >> 5)] >> (c & 31)) & 1u; }

// V5: the least D over the occupied cells of the window within +-k rows and columns of local cell (er, ec); -1: none
__device__ __forceinline__ int nearest_d(const uint32_t* occ, int W, int rows, int er, int ec, int k) {
  const uint32_t m = (1u << (k + 1)) - 1u;
  int best = 1 << 20;
  for (int dr = 0; dr <= k && dr * dr < best; ++dr) {
    for (int s = 0; s < (dr == 0 ? 1 : 2); ++s) {
      const int r = s ? er + dr : er - dr;
      if (r < 0 || r >= rows) continue;
      const unsigned long long v = look(occ + r * W, ec + 32 - k);   // bit q: column offset q - k
      const uint32_t left = (uint32_t)v & m;                         // offsets -k .. 0
      const uint32_t right = (uint32_t)(v >> k) & m;                 // offsets 0 .. k
      if (left) {
        const int dc = k - (31 - __clz((int)left));
        const int d = dr * dr + dc * dc;
        best = d < best ? d : best;
      }
      if (right) {
        const int dc = __ffs((int)right) - 1;
        const int d = dr * dr + dc * dc;
        best = d < best ? d : best;
      }
    }
  }
  return best == (1 << 20) ? -1 : best;
}

// blockIdx.x: the pair.  recs: the test hook's per-beam record [n_beams] (one pair), or null
template <int P>
__global__ __launch_bounds__(kThreads) void icp_verify_map(VerifyMapArgs a, const VerifyMapPair* __restrict__ pairs, const float* __restrict__ scan,
                                                            const float2* __restrict__ beams, int n_beams, tbnav_icp_verify_map_info* __restrict__ out,
                                                            IcpConst k, tbnav_icp_verify_map_beam* __restrict__ recs) {
  extern __shared__ uint32_t win[];          // [3][rows][W]: OCCUPIED, FREE, UNKNOWN
  __shared__ uint32_t part[kWaves][kCounts];
  const int t = threadIdx.x, lane = t & (kLanes - 1), wave = t / kLanes;
  const VerifyMapPair pr = pairs[blockIdx.x];
  const int rows = 2 * a.H, nw = (rows + 31) >> 5, W = nw + 2;
  const int wx0 = pr.sx - a.H, wy0 = pr.sy - a.H;   // the map cell of the window's cell (0, 0)
  uint32_t* const occ = win;
  uint32_t* const fre = win + rows * W;
  uint32_t* const unk = win + 2 * rows * W;
  const unsigned int* __restrict__ ids = a.table + (size_t)(pr.particle < 0 ? *a.best : pr.particle) * a.TT;
  // OCCUPIED, as icp_align_map stages it
  for (int idx = t; idx < rows * W; idx += kThreads) {
    const int r = idx / W, q = idx - r * W - 1;     // word q of the row's bits; -1 and nw: the zero words either side
    uint32_t v = 0u;
    if (q >= 0 && q < nw) {
      v = (uint32_t)occ_row_window(a.bm, ids, a.TW, a.side, wx0 + r, wy0 + 32 * q);
      const int rem = rows - 32 * q;                // columns of this word that are cells of the window (>= 1)
      if (rem < 32) v &= (1u << rem) - 1u;
    }
    occ[idx] = v;
  }
  // FREE and UNKNOWN, map-aligned: word j = 0 .. nw of row r is map word w0 + j, into slot 1 + j of the row
  {
    const int w0 = wy0 >> 5;                        // (an arithmetic shift: floor for a window that starts left of the map)
    const int nm = nw + 1, n_items = rows * nm, n_pairs = (n_items + 1) >> 1;
    const int half = lane >> 5, l5 = lane & 31;
    for (int base = wave * kInFlight; base < n_pairs; base += kWaves * kInFlight) {   // (the same trip count for a wave's lanes)
      double l[kInFlight];
      int slot[kInFlight];
      bool in[kInFlight], zero[kInFlight];
#pragma unroll
      for (int u = 0; u < kInFlight; ++u) {
        const int it = 2 * (base + u) + half;
        const int r = it / nm, j = it - r * nm;
        const int mx = wx0 + r, wy = w0 + j;
        slot[u] = it < n_items ? r * W + 1 + j : -1;
        in[u] = it < n_items && mx >= 0 && mx < a.side && wy >= 0 && wy < a.TW && wy * kOccTile + l5 < a.side;
        const unsigned int id = in[u] ? ids[(mx >> 5) * a.TW + wy] : 0u;
        zero[u] = id == 0u;
        l[u] = (in[u] && !zero[u]) ? a.lo[(size_t)id * (kOccTile * kOccTile) + (mx & (kOccTile - 1)) * kOccTile + l5] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < kInFlight; ++u) {
        const unsigned long long bu = __ballot(in[u] && (zero[u] || (l[u] >= a.half_lo && l[u] <= a.half_hi)));
        const unsigned long long bf = __ballot(in[u] && !zero[u] && l[u] <= a.free_cut);
        if (l5 == 0 && slot[u] >= 0) {
          unk[slot[u]] = (uint32_t)(bu >> (32 * half));
          fre[slot[u]] = (uint32_t)(bf >> (32 * half));
        }
      }
    }
  }
  __syncthreads();
  // ... shifted to the window's origin in place, a row per thread: word q reads slots 1 + q and 2 + q, written in ascending q
  {
    const int o = wy0 & 31;
    for (int r = t; r < rows; r += kThreads) {
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        uint32_t* row = (m ? unk : fre) + r * W;
        for (int q = 0; q < nw; ++q) {
          uint32_t v = o ? (row[1 + q] >> o) | (row[2 + q] << (32 - o)) : row[1 + q];
          const int rem = rows - 32 * q;
          if (rem < 32) v &= (1u << rem) - 1u;
          row[1 + q] = v;
        }
        row[0] = 0u;
        row[nw + 1] = 0u;
      }
    }
  }
  __syncthreads();

  const double fx0 = (double)(wx0 > 0 ? wx0 : 0), fx1 = (double)(wx0 + rows < a.side ? wx0 + rows : a.side);
  const double fy0 = (double)(wy0 > 0 ? wy0 : 0), fy1 = (double)(wy0 + rows < a.side ? wy0 + rows : a.side);
  uint32_t cnt[kCounts];
#pragma unroll
  for (int q = 0; q < kCounts; ++q) cnt[q] = 0u;
#pragma unroll
  for (int j = 0; j < P; ++j) {
    const int i = t + j * kThreads;
    if (i >= n_beams) continue;
    tbnav_icp_verify_map_beam rec{};
    float2 src;
    if (cloud_point(scan[i], beams[i], k, src)) {
      ++cnt[0];
      const float ax = (float)(((pr.c * (double)src.x) + ((-pr.s) * (double)src.y)) + pr.x);
      const float ay = (float)(((pr.s * (double)src.x) + (pr.c * (double)src.y)) + pr.y);
      const double fi = floor(((double)ax - a.xmin) * a.inv), fj = floor(((double)ay - a.ymin) * a.inv);
      if (!(fi >= fx0 && fi < fx1 && fj >= fy0 && fj < fy1)) {   // (a NaN is outside)
        ++cnt[1];
        rec.cls = TBNAV_ICP_VERIFY_OUTSIDE;
      } else {
        const int ei = (int)fi, ej = (int)fj;
        const int er = ei - wx0, ec = ej - wy0;
        const int di = ei - pr.sx, dj = ej - pr.sy;
        const int ai = di < 0 ? -di : di, aj = dj < 0 ? -dj : dj, si = di < 0 ? -1 : 1, sj = dj < 0 ? -1 : 1;
        const int n = ai > aj ? ai : aj;     // <= H
        // G17's quotients with the remainder carried: 2*t*|d| + n = q * 2n + rem, 0 <= rem < 2n — the integers of the closed form
        int qi = 0, remi = n, qj = 0, remj = n, pi = a.H, pj = a.H, b = n + 1;
        uint32_t nf = 0u, nu = 0u;
        for (int s = 1; s <= n; ++s) {
          remi += 2 * ai; if (remi >= 2 * n) { remi -= 2 * n; ++qi; }
          remj += 2 * aj; if (remj >= 2 * n) { remj -= 2 * n; ++qj; }
          const int ci = a.H + si * qi, cj = a.H + sj * qj;
          if (bit_at(occ, W, ci, cj) || (ci != pi && cj != pj && bit_at(occ, W, pi, cj) && bit_at(occ, W, ci, pj))) { b = s; break; }
          if (s < n) {
            nf += bit_at(fre, W, ci, cj) ? 1u : 0u;
            nu += bit_at(unk, W, ci, cj) ? 1u : 0u;
          }
          pi = ci; pj = cj;
        }
        int cls, D = -1;
        if (b + a.k < n) {
          cls = TBNAV_ICP_VERIFY_THROUGH;
        } else {
          D = nearest_d(occ, W, rows, er, ec, a.k);
          if (D >= 0 && D <= a.k * a.k) cls = TBNAV_ICP_VERIFY_HIT;     // (an OCCUPIED end cell has D = 0: OCCUPIED wins)
          else if (bit_at(fre, W, er, ec)) cls = TBNAV_ICP_VERIFY_MISSING;
          else if (bit_at(unk, W, er, ec)) cls = TBNAV_ICP_VERIFY_UNSEEN;
          else cls = TBNAV_ICP_VERIFY_UNDECIDED;
        }
#pragma unroll
        for (int q = TBNAV_ICP_VERIFY_HIT; q <= TBNAV_ICP_VERIFY_UNDECIDED; ++q) cnt[q] += cls == q ? 1u : 0u;   // counts 2 .. 6 are the classes' own numbers
        cnt[7] += nf; cnt[8] += nu;
        rec.cls = cls; rec.e[0] = ei; rec.e[1] = ej; rec.n = n; rec.b = b <= n ? b : -1; rec.D = D;
        rec.free_cells = (int32_t)nf; rec.unknown_cells = (int32_t)nu;
      }
    }
    if (recs) recs[i] = rec;
  }
#pragma unroll
  for (int q = 0; q < kCounts; ++q) {
    const uint32_t v = wave_sum_u32(cnt[q]);
    if (lane == 0) part[wave][q] = v;
  }
  __syncthreads();
  if (t == 0) {
    uint32_t tot[kCounts];
#pragma unroll
    for (int q = 0; q < kCounts; ++q) {
      tot[q] = 0u;
      for (int w = 0; w < kWaves; ++w) tot[q] += part[w][q];
    }
    tbnav_icp_verify_map_info o{};
    o.free_cells = (int64_t)tot[7]; o.unknown_cells = (int64_t)tot[8];
    o.points = (int32_t)tot[0]; o.outside = (int32_t)tot[1]; o.walked = o.points - o.outside;
    o.hit = (int32_t)tot[2]; o.through = (int32_t)tot[3]; o.missing = (int32_t)tot[4]; o.unseen = (int32_t)tot[5]; o.undecided = (int32_t)tot[6];
    o.sensor_cell[0] = pr.sx; o.sensor_cell[1] = pr.sy;
    o.sensor_class = bit_at(occ, W, a.H, a.H) ? 2 : bit_at(unk, W, a.H, a.H) ? 0 : bit_at(fre, W, a.H, a.H) ? 1 : 3;
    o.accepted = (o.walked >= 1 && (long long)o.through * 1024 <= (long long)a.max_through * o.walked &&
                  (long long)o.missing * 1024 <= (long long)a.max_missing * o.walked && (long long)o.hit * 1024 >= (long long)a.min_hit * o.walked)
                     ? 1 : 0;
    out[blockIdx.x] = o;
  }
}

bool params_ok(const tbnav_icp_verify_map_params& p) {
  const auto q10 = [](int32_t v) { return v >= 0 && v <= 1024; };
  return p.half_cells >= 8 && p.half_cells <= TBNAV_ICP_VERIFY_MAP_MAX_HALF && p.slack_cells >= 0 && p.slack_cells <= TBNAV_ICP_VERIFY_MAP_MAX_SLACK &&
         q10(p.max_through_q10) && q10(p.max_missing_q10) && q10(p.min_hit_q10) && p.reserved == 0;
}

template <int P>
void launch(tbnav_icp* h, const VerifyMapArgs& a, int n, int n_beams, tbnav_icp_verify_map_beam* recs) {
  const int rows = 2 * a.H;
  const size_t lds = 3 * sizeof(uint32_t) * (size_t)rows * (size_t)(((rows + 31) >> 5) + 2);
  hipLaunchKernelGGL((icp_verify_map<P>), dim3(n), dim3(kThreads), lds, h->stream, a, h->d_verify_in.as<VerifyMapPair>(), h->d_scans.as<float>(),
                     h->d_table, n_beams, h->d_verify_out.as<tbnav_icp_verify_map_info>(), h->k, recs);
  h->verify_map_p = P;
}

// the entries' common body.  recs: the test hook (n == 1): its per-beam record [n_beams]; infos may then be null
int verify_map(tbnav_icp* h, tbnav_rbpf* pf, const float* scan, int32_t n_beams, int32_t n, const int32_t* particles, const double* Ts,
               const tbnav_icp_verify_map_params* params, tbnav_icp_verify_map_info* infos, tbnav_icp_verify_map_beam* recs) {
  // V1: arguments, parameters and particles; then device and group; then the poses (V3).  Nothing is changed before the last passes.
  if (!h || !pf || !scan || !particles || !Ts || n < 1 || n_beams <= 0 || n_beams > TBNAV_ICP_MAX_BEAMS) return TBNAV_ERR_INVALID_ARG;
  if (!recs && !infos) return TBNAV_ERR_INVALID_ARG;
  tbnav_icp_verify_map_params p;
  tbnav_icp_default_verify_map_params(&p);
  if (params) p = *params;
  if (!params_ok(p)) return TBNAV_ERR_INVALID_ARG;
  for (int i = 0; i < n; ++i)
    if (!tbnav_nk::particle_ok(pf, particles[i])) return TBNAV_ERR_INVALID_ARG;
  if (h->device != pf->device || pf->comm) return TBNAV_ERR_UNSUPPORTED;
  const double inv = 1.0 / pf->p.resolution;
  const double p0x = (double)(float)h->k.trs_x, p0y = (double)(float)h->k.trs_y;   // item 1's point of a zero range
  std::vector<VerifyMapPair> pairs((size_t)n);
  bool best = false;
  for (int i = 0; i < n; ++i) {
    const double* T = Ts + 3 * (size_t)i;
    if (!std::isfinite(T[0]) || !std::isfinite(T[1]) || !std::isfinite(T[2])) return TBNAV_ERR_OUT_OF_WORLD;
    VerifyMapPair& q = pairs[(size_t)i];
    q.c = (double)(float)std::cos(T[0]);   // item 2
    q.s = (double)(float)std::sin(T[0]);
    q.x = (double)(float)T[1];
    q.y = (double)(float)T[2];
    const float ax = (float)(((q.c * p0x) + ((-q.s) * p0y)) + q.x);   // item 3
    const float ay = (float)(((q.s * p0x) + (q.c * p0y)) + q.y);
    const double fx = std::floor(((double)ax - pf->p.xmin) * inv), fy = std::floor(((double)ay - pf->p.ymin) * inv);
    if (!(fx >= 0.0 && fx < (double)pf->xsize && fy >= 0.0 && fy < (double)pf->xsize)) return TBNAV_ERR_OUT_OF_WORLD;
    q.particle = particles[i]; q.sx = (int)fx; q.sy = (int)fy; q.pad = 0;
    best = best || particles[i] == TBNAV_ICP_MAP_BEST_PARTICLE;
  }
  DeviceGuard guard(h->device);
  if (!guard.ok) return TBNAV_ERR_NO_DEVICE;
  if (int rc = ensure_table(h, n_beams)) return rc;
  if (int rc = h->d_scans.reserve(sizeof(float) * (size_t)n_beams)) return rc;
  if (int rc = h->d_verify_in.reserve(sizeof(VerifyMapPair) * (size_t)n)) return rc;
  if (int rc = h->d_verify_out.reserve(sizeof(tbnav_icp_verify_map_info) * (size_t)n)) return rc;
  if (recs)
    if (int rc = h->d_verify_rec.reserve(sizeof(tbnav_icp_verify_map_beam) * (size_t)n_beams)) return rc;
  TBNAV_HIP(hipMemcpyAsync(h->d_scans.ptr, scan, sizeof(float) * (size_t)n_beams, hipMemcpyHostToDevice, h->stream));
  TBNAV_HIP(hipMemcpyAsync(h->d_verify_in.ptr, pairs.data(), sizeof(VerifyMapPair) * (size_t)n, hipMemcpyHostToDevice, h->stream));
  // A9: behind whatever the filter's stream has in flight, the arg-max of its weights included where a pair asks for it
  if (best)
    if (int rc = tbnav_nk::enqueue_best(pf, TBNAV_NAV_BEST_PARTICLE)) return rc;
  IcpSearch& S = h->search;
  if (!S.map_ev) TBNAV_HIP(hipEventCreateWithFlags(&S.map_ev, hipEventDisableTiming));
  TBNAV_HIP(hipEventRecord(S.map_ev, pf->stream));
  TBNAV_HIP(hipStreamWaitEvent(h->stream, S.map_ev, 0));
  const VerifyMapArgs a{pf->pool.lo, pf->pool.bm, pf->d_table[pf->cur], pf->d_best, pf->TW, pf->TT, pf->xsize, pf->p.xmin, pf->p.ymin, inv,
                        pf->cuts.half_lo, pf->cuts.half_hi, pf->cuts.free_cut, p.half_cells, p.slack_cells,
                        p.max_through_q10, p.max_missing_q10, p.min_hit_q10};
  tbnav_icp_verify_map_beam* d_recs = recs ? h->d_verify_rec.as<tbnav_icp_verify_map_beam>() : nullptr;
  const int per = (n_beams + kThreads - 1) / kThreads;
  static_assert(TBNAV_ICP_MAX_BEAMS <= 16 * kThreads, "no instantiation holds TBNAV_ICP_MAX_BEAMS");
  if (per <= 1) launch<1>(h, a, n, n_beams, d_recs);
  else if (per <= 2) launch<2>(h, a, n, n_beams, d_recs);
  else if (per <= 4) launch<4>(h, a, n, n_beams, d_recs);
  else if (per <= 6) launch<6>(h, a, n, n_beams, d_recs);
  else if (per <= 8) launch<8>(h, a, n, n_beams, d_recs);
  else launch<16>(h, a, n, n_beams, d_recs);
  TBNAV_HIP(hipGetLastError());
  std::vector<tbnav_icp_verify_map_info> outs((size_t)n);
  TBNAV_HIP(hipMemcpyAsync(outs.data(), h->d_verify_out.ptr, sizeof(tbnav_icp_verify_map_info) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
  if (recs) TBNAV_HIP(hipMemcpyAsync(recs, d_recs, sizeof(tbnav_icp_verify_map_beam) * (size_t)n_beams, hipMemcpyDeviceToHost, h->stream));
  TBNAV_HIP(hipStreamSynchronize(h->stream));
  if (infos)
    for (int i = 0; i < n; ++i) infos[i] = outs[(size_t)i];
  return TBNAV_OK;
}

}  // namespace

extern "C" {

void tbnav_icp_default_verify_map_params(tbnav_icp_verify_map_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof *p);
  p->half_cells = 96;
  p->slack_cells = 2;
  p->max_through_q10 = 102;
  p->max_missing_q10 = 102;
  p->min_hit_q10 = 512;
}

int tbnav_icp_verify_map(tbnav_icp* h, tbnav_rbpf* pf, int32_t particle, const float* scan, int32_t n_beams, const double T[3],
                         const tbnav_icp_verify_map_params* params, tbnav_icp_verify_map_info* info) {
  if (!info) return TBNAV_ERR_INVALID_ARG;
  return verify_map(h, pf, scan, n_beams, 1, &particle, T, params, info, nullptr);
}

int tbnav_icp_verify_map_batch(tbnav_icp* h, tbnav_rbpf* pf, const float* scan, int32_t n_beams, int32_t n, const int32_t* particles,
                               const double* T, const tbnav_icp_verify_map_params* params, tbnav_icp_verify_map_info* infos) {
  if (!infos) return TBNAV_ERR_INVALID_ARG;
  return verify_map(h, pf, scan, n_beams, n, particles, T, params, infos, nullptr);
}

int tbnav_icp_verify_map_beams(tbnav_icp* h, tbnav_rbpf* pf, int32_t particle, const float* scan, int32_t n_beams, const double T[3],
                               const tbnav_icp_verify_map_params* params, tbnav_icp_verify_map_info* info, tbnav_icp_verify_map_beam* beams) {
  if (!beams) return TBNAV_ERR_INVALID_ARG;
  return verify_map(h, pf, scan, n_beams, 1, &particle, T, params, info, beams);
}

int tbnav_icp_last_verify_map_kernel(const tbnav_icp* h, char* kernel, int32_t kernel_cap) {
  if (!h || !kernel || kernel_cap <= 0) return TBNAV_ERR_INVALID_ARG;
  if (h->verify_map_p) std::snprintf(kernel, (size_t)kernel_cap, "icp_verify_map<%d>", h->verify_map_p);
  else kernel[0] = '\0';
  return TBNAV_OK;
}

}  // extern "C"

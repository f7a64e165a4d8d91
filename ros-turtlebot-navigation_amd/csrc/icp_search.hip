// icp_search.hip — the correlative scan search in front of the device ICP (include/tbnav_icp.h, CORRELATIVE SEARCH; an addition
// with no counterpart in the reference).  Three kernels, all integer or fp64 without contraction (-ffp-contract=off,
// csrc/Makefile), so that tests/icp_search_restatement.py reproduces them exactly:
//   icp_search_table   one workgroup per pair: the target's likelihood table as bytes in LDS.  Every valid target point stamps
//                      its (2k+1)^2 Gaussian by a MAXIMUM; the hardware has no byte maximum, so it is a compare-and-swap on the
//                      byte's dword, entered only where the byte would grow.  The table goes to global memory PADDED with wl
//                      zero cells on every side: the scoring loop below then needs no bounds test.
//   icp_search_score   one workgroup per (pair, angle): the padded table (<= 43 KB, copied with 16-byte loads) and the base
//                      cells of this angle's source points (uint16, compacted: a sum of integers has no order) in LDS.  A
//                      thread owns J = ceil(nl^2 / 256) translations and walks the points: the base cell is a broadcast read,
//                      the table byte a strided one.  Points whose base cell lies outside the table but whose window reaches
//                      into it go to a second list with a bounds test (they exist only where half_extent is smaller than the
//                      laser's range).  The workgroup reduces one 64-bit key, score high and inverted rank low.
//   icp_search_select  one wave per pair: the maximum of the na keys, the candidate count and thr.
// slack_q10 > 0 scores a second time against thr (pass 1: the key is the inverted rank alone, among score >= thr).
// The score volume itself is written only for the test hook.  The shape of the score volume (F1-F6) is icp_search_shape.hip's:
// its kernel is launched here behind the final icp_search_select and its record comes back with the selection.
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

constexpr int kMaxStampSide = 2 * TBNAV_ICP_SEARCH_MAX_STAMP + 1;
constexpr int kChunk = 1024;      // pairs per launch: bounds the table memory (43 KB a pair at the largest table)
constexpr int kRankLinBits = 18;  // the linear index (< 181 * 33 * 33 = 197109) below D (<= 90^2 + 2 * 16^2) in the rank

// what one (pair, angle) workgroup leaves
struct SearchRec {
  unsigned long long key;
  uint32_t count, points;
};

// table byte idx <- max(itself, v) by compare-and-swap on its dword
__device__ __forceinline__ void byte_max(uint32_t* words, int idx, uint32_t v) {
  uint32_t* w = words + (idx >> 2);
  const int sh = (idx & 3) * 8;
  uint32_t old = *reinterpret_cast<volatile uint32_t*>(w);
  while (((old >> sh) & 0xffu) < v) {
    const uint32_t want = (old & ~(0xffu << sh)) | (v << sh);
    const uint32_t seen = atomicCAS(w, old, want);
    if (seen == old) break;
    old = seen;
  }
}

__global__ __launch_bounds__(kThreads) void icp_search_table(const float* __restrict__ scans, const float* __restrict__ stored,
                                                             const float2* __restrict__ beams, int n_beams,
                                                             const SearchPair* __restrict__ pairs, const uint8_t* __restrict__ stamp,
                                                             uint8_t* __restrict__ tables, uint32_t* __restrict__ tgt_points, IcpConst k,
                                                             SearchConst sc) {
  extern __shared__ uint4 lds_tab[];                     // [tab_stride / 16]
  uint32_t* words = reinterpret_cast<uint32_t*>(lds_tab);
  __shared__ uint8_t st[kMaxStampSide * kMaxStampSide];
  __shared__ uint32_t n_points;
  const int t = threadIdx.x;
  const int w = 2 * sc.k + 1;
  for (int i = t; i < sc.tab_stride / 16; i += kThreads) lds_tab[i] = make_uint4(0u, 0u, 0u, 0u);
  for (int i = t; i < w * w; i += kThreads) st[i] = stamp[i];
  if (t == 0) n_points = 0u;
  __syncthreads();
  const SearchPair pr = pairs[blockIdx.x];
  const float* ts = pr.tgt < 0 ? stored : scans + (size_t)pr.tgt * n_beams;
  uint32_t cnt = 0u;
  for (int i = t; i < n_beams; i += kThreads) {
    float2 p;
    if (!cloud_point(ts[i], beams[i], k, p)) continue;
    ++cnt;
    int ix, iy;
    if (!cell_of((double)p.x, sc.E, sc.inv, ix) || !cell_of((double)p.y, sc.E, sc.inv, iy)) continue;
    if (ix < -sc.k || ix >= sc.n + sc.k || iy < -sc.k || iy >= sc.n + sc.k) continue;
    for (int oy = -sc.k; oy <= sc.k; ++oy) {
      const int cy = iy + oy;
      if (cy < 0 || cy >= sc.n) continue;
      for (int ox = -sc.k; ox <= sc.k; ++ox) {
        const int cx = ix + ox;
        if (cx < 0 || cx >= sc.n) continue;
        const uint32_t v = st[(oy + sc.k) * w + (ox + sc.k)];
        if (v != 0u) byte_max(words, (cy + sc.wl) * sc.side + (cx + sc.wl), v);
      }
    }
  }
  if (cnt) atomicAdd(&n_points, cnt);
  __syncthreads();
  uint4* out = reinterpret_cast<uint4*>(tables + (size_t)blockIdx.x * (size_t)sc.tab_stride);
  for (int i = t; i < sc.tab_stride / 16; i += kThreads) out[i] = lds_tab[i];
  if (t == 0) tgt_points[blockIdx.x] = n_points;
}

// blockIdx.x: the angle ia; blockIdx.y: the pair.  pass 0: the key is (score, inverted rank), count = the candidates at this
// workgroup's best score.  pass 1: among score >= sel[pair].thr the key is (inverted rank, score), count = how many they are.
template <int J>
__global__ __launch_bounds__(kThreads) void icp_search_score(const float* __restrict__ scans, const float* __restrict__ stored,
                                                             const float2* __restrict__ beams, int n_beams,
                                                             const SearchPair* __restrict__ pairs, const double2* __restrict__ rot,
                                                             const uint8_t* __restrict__ tables, const SearchSel* __restrict__ sel,
                                                             SearchRec* __restrict__ rec, uint32_t* __restrict__ scores, IcpConst k,
                                                             SearchConst sc, int pass) {
  extern __shared__ uint4 lds_tab[];                                    // the padded table, then the cells
  const uint8_t* tab = reinterpret_cast<const uint8_t*>(lds_tab);
  uint16_t* cells = reinterpret_cast<uint16_t*>(lds_tab + sc.tab_stride / 16);  // [n_beams]: fast list up from 0, slow list down from the end
  __shared__ uint32_t n_fast, n_slow, n_valid;
  __shared__ unsigned long long red_key[kThreads / kWave];
  __shared__ uint32_t red_cnt[kThreads / kWave];
  const int t = threadIdx.x;
  const int ia = blockIdx.x, pair = blockIdx.y;
  {
    const uint4* src = reinterpret_cast<const uint4*>(tables + (size_t)pair * (size_t)sc.tab_stride);
    for (int i = t; i < sc.tab_stride / 16; i += kThreads) lds_tab[i] = src[i];
  }
  if (t == 0) { n_fast = 0u; n_slow = 0u; n_valid = 0u; }
  __syncthreads();
  const SearchPair pr = pairs[pair];
  const double2 cs = rot[(size_t)pair * sc.na + ia];
  const float* ss = pr.src < 0 ? stored : scans + (size_t)pr.src * n_beams;
  uint32_t valid = 0u;
  for (int i = t; i < n_beams; i += kThreads) {
    float2 p;
    if (!cloud_point(ss[i], beams[i], k, p)) continue;
    ++valid;
    const double sx = (double)p.x, sy = (double)p.y;
    const double ax = (((cs.x * sx) - (cs.y * sy)) + pr.x0);
    const double ay = (((cs.y * sx) + (cs.x * sy)) + pr.y0);
    int bx, by;
    if (!cell_of(ax, sc.E, sc.inv, bx) || !cell_of(ay, sc.E, sc.inv, by)) continue;
    if (bx >= 0 && bx < sc.n && by >= 0 && by < sc.n) {
      // the window's first cell in the padded table: rows by .. by + 2*wl, columns bx .. bx + 2*wl, all inside it
      cells[atomicAdd(&n_fast, 1u)] = (uint16_t)(by * sc.side + bx);
    } else if (bx >= -sc.wl && bx < sc.n + sc.wl && by >= -sc.wl && by < sc.n + sc.wl) {
      // outside the table, the window reaches in: padded coordinates, 0 .. side - 1 <= 207 each
      cells[n_beams - 1 - (int)atomicAdd(&n_slow, 1u)] = (uint16_t)(((by + sc.wl) << 8) | (bx + sc.wl));
    }
  }
  if (valid) atomicAdd(&n_valid, valid);
  __syncthreads();
  const int nf = (int)n_fast, ns = (int)n_slow;
  const int n_cand = sc.nl * sc.nl;
  int off[J], iy[J], ix[J];
  uint32_t acc[J];
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int q = t + j * kThreads;
    const bool in = q < n_cand;
    iy[j] = in ? q / sc.nl : 0;
    ix[j] = in ? q - iy[j] * sc.nl : 0;
    off[j] = iy[j] * sc.side + ix[j];
    acc[j] = 0u;
  }
  for (int p = 0; p < nf; ++p) {
    const int cell = cells[p];
#pragma unroll
    for (int j = 0; j < J; ++j) acc[j] += tab[cell + off[j]];
  }
  for (int p = 0; p < ns; ++p) {
    const int v = cells[n_beams - 1 - p];
    const int py = v >> 8, px = v & 0xff;
#pragma unroll
    for (int j = 0; j < J; ++j) {
      const int ry = py + iy[j] - sc.wl, rx = px + ix[j] - sc.wl;   // padded coordinates of the cell this candidate reads
      if (ry >= sc.wl && ry < sc.n + sc.wl && rx >= sc.wl && rx < sc.n + sc.wl) acc[j] += tab[ry * sc.side + rx];
    }
  }
  const uint32_t thr = pass ? sel[pair].thr : 0u;
  unsigned long long key = 0ull;
  uint32_t cnt = 0u;
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int q = t + j * kThreads;
    if (q >= n_cand) continue;
    const int lin = (ia * sc.nl + iy[j]) * sc.nl + ix[j];
    if (scores) scores[(size_t)pair * sc.na * n_cand + lin] = acc[j];
    const int da = ia - sc.wa, dy = iy[j] - sc.wl, dx = ix[j] - sc.wl;
    const uint32_t rank = ((uint32_t)(da * da + dy * dy + dx * dx) << kRankLinBits) | (uint32_t)lin;
    unsigned long long kj;
    if (pass) {
      if (acc[j] < thr) continue;
      ++cnt;
      kj = ((unsigned long long)(~rank) << 32) | acc[j];
    } else {
      kj = ((unsigned long long)acc[j] << 32) | (~rank);
    }
    key = kj > key ? kj : key;
  }
  // the workgroup's maximum, then (pass 0) how many of its candidates reach that score
  key = wave_max_u64(key);
  if ((t & (kWave - 1)) == 0) red_key[t / kWave] = key;
  __syncthreads();
  key = red_key[0];
#pragma unroll
  for (int w = 1; w < kThreads / kWave; ++w) key = red_key[w] > key ? red_key[w] : key;
  if (!pass) {
    const uint32_t best = (uint32_t)(key >> 32);
#pragma unroll
    for (int j = 0; j < J; ++j)
      if (t + j * kThreads < n_cand && acc[j] == best) ++cnt;
  }
  cnt = wave_sum_u32(cnt);
  if ((t & (kWave - 1)) == 0) red_cnt[t / kWave] = cnt;
  __syncthreads();
  if (t == 0) {
    SearchRec r;
    r.key = key;
    r.count = 0u;
#pragma unroll
    for (int w = 0; w < kThreads / kWave; ++w) r.count += red_cnt[w];
    r.points = n_valid;
    rec[(size_t)pair * sc.na + ia] = r;
  }
}

// one wave per pair: the na records -> the chosen candidate
__global__ __launch_bounds__(kWave) void icp_search_select(const SearchRec* __restrict__ rec, const uint32_t* __restrict__ tgt_points,
                                                           SearchSel* __restrict__ sel, SearchConst sc, int pass) {
  const int t = threadIdx.x, pair = blockIdx.x;
  const SearchRec* r = rec + (size_t)pair * sc.na;
  unsigned long long key = 0ull;
  for (int a = t; a < sc.na; a += kWave) key = r[a].key > key ? r[a].key : key;
  key = wave_max_u64(key);
  uint32_t cnt = 0u;
  for (int a = t; a < sc.na; a += kWave)
    if (pass || (uint32_t)(r[a].key >> 32) == (uint32_t)(key >> 32)) cnt += r[a].count;
  cnt = wave_sum_u32(cnt);
  if (t == 0) {
    SearchSel s;
    // pass 1 with nothing at or above thr cannot happen: the best candidate itself is
    const uint32_t hi = (uint32_t)(key >> 32), lo = (uint32_t)key;
    s.score = pass ? lo : hi;
    s.lin = (~(pass ? hi : lo)) & ((1u << kRankLinBits) - 1u);
    s.count = cnt;
    s.points = r[0].points;
    s.tgt_points = tgt_points[pair];
    s.thr = s.score - (uint32_t)(((unsigned long long)s.score * sc.slack) >> 10);
    if (pass) s.thr = sel[pair].thr;
    sel[pair] = s;
  }
}

template <class T>
int ensure(T*& ptr, size_t& cap, size_t want) {
  if (want <= cap) return TBNAV_OK;
  if (ptr) TBNAV_HIP(hipFree(ptr));
  ptr = nullptr; cap = 0;
  void* p = nullptr;
  TBNAV_HIP(hipMalloc(&p, want));
  ptr = static_cast<T*>(p);
  cap = want;
  return TBNAV_OK;
}

int table_side(const tbnav_icp_search_params& p) { return 2 * (int)std::ceil(p.half_extent / p.resolution); }

bool params_ok(const tbnav_icp_search_params& p) {
  if (!(p.resolution > 0.0) || !std::isfinite(p.resolution) || !(p.half_extent > 0.0) || !std::isfinite(p.half_extent) ||
      !(p.sigma > 0.0) || !std::isfinite(p.sigma) || !std::isfinite(p.ang_step) || !std::isfinite(p.min_quality))
    return false;
  if (p.stamp_cells < 1 || p.stamp_cells > TBNAV_ICP_SEARCH_MAX_STAMP || p.lin_cells < 0 || p.lin_cells > TBNAV_ICP_SEARCH_MAX_LIN ||
      p.ang_steps < 0 || p.ang_steps > TBNAV_ICP_SEARCH_MAX_ANG || p.slack_q10 < 0 || p.slack_q10 > 1023)
    return false;
  const double cells = std::ceil(p.half_extent / p.resolution);
  if (!(cells >= 1.0 && cells <= (double)TBNAV_ICP_SEARCH_MAX_SIDE)) return false;
  return table_side(p) + 2 * p.lin_cells <= TBNAV_ICP_SEARCH_MAX_SIDE;
}

SearchConst make_const(const tbnav_icp_search_params& p) {
  SearchConst sc;
  sc.E = p.half_extent;
  sc.inv = 1.0 / p.resolution;
  sc.n = table_side(p);
  sc.wl = p.lin_cells; sc.wa = p.ang_steps; sc.k = p.stamp_cells;
  sc.side = sc.n + 2 * sc.wl;
  sc.nl = 2 * sc.wl + 1; sc.na = 2 * sc.wa + 1;
  sc.tab_stride = (sc.side * sc.side + 15) & ~15;
  sc.slack = (unsigned)p.slack_q10;
  return sc;
}

// the stamp of S3 on the device, rebuilt when the parameters it depends on change
int ensure_stamp(tbnav_icp* h, const tbnav_icp_search_params& p) {
  IcpSearch& S = h->search;
  if (S.have_stamp && S.stamp_of.resolution == p.resolution && S.stamp_of.sigma == p.sigma && S.stamp_of.stamp_cells == p.stamp_cells)
    return TBNAV_OK;
  if (!S.d_stamp) TBNAV_HIP(hipMalloc(&S.d_stamp, kMaxStampSide * kMaxStampSide));
  const int k = p.stamp_cells, w = 2 * k + 1;
  std::vector<uint8_t> st((size_t)(w * w));
  for (int oy = -k; oy <= k; ++oy)
    for (int ox = -k; ox <= k; ++ox) {
      const double d2 = (double)(ox * ox + oy * oy) * (p.resolution * p.resolution);
      st[(size_t)((oy + k) * w + (ox + k))] = (uint8_t)std::floor(255.0 * std::exp(-(d2 / (2.0 * (p.sigma * p.sigma)))) + 0.5);
    }
  S.have_stamp = false;
  TBNAV_HIP(hipMemcpyAsync(S.d_stamp, st.data(), st.size(), hipMemcpyHostToDevice, h->stream));
  TBNAV_HIP(hipStreamSynchronize(h->stream));  // st is about to go out of scope
  S.stamp_of = p;
  S.have_stamp = true;
  return TBNAV_OK;
}

template <int J>
void launch_score(tbnav_icp* h, int n, int n_beams, const SearchConst& sc, const SearchPair* d_pairs, const double2* d_rot,
                  uint32_t* d_scores, int pass) {
  IcpSearch& S = h->search;
  const size_t lds = (size_t)sc.tab_stride + ((sizeof(uint16_t) * (size_t)n_beams + 15) & ~(size_t)15);
  hipLaunchKernelGGL((icp_search_score<J>), dim3(sc.na, n), dim3(kThreads), lds, h->stream, h->d_scans, h->d_stored, h->d_table, n_beams,
                     d_pairs, d_rot, S.d_tables, static_cast<const SearchSel*>(S.d_sel), static_cast<SearchRec*>(S.d_rec), d_scores,
                     h->k, sc, pass);
}

// translations per thread -> J (nl^2 <= 33^2 = 1089 <= 5 * 256)
void dispatch_score(tbnav_icp* h, int n, int n_beams, const SearchConst& sc, const SearchPair* d_pairs, const double2* d_rot,
                    uint32_t* d_scores, int pass) {
  static_assert((2 * TBNAV_ICP_SEARCH_MAX_LIN + 1) * (2 * TBNAV_ICP_SEARCH_MAX_LIN + 1) <= 5 * kThreads, "no instantiation holds the window");
  const int per = (sc.nl * sc.nl + kThreads - 1) / kThreads;
  if (per <= 1) launch_score<1>(h, n, n_beams, sc, d_pairs, d_rot, d_scores, pass);
  else if (per <= 2) launch_score<2>(h, n, n_beams, sc, d_pairs, d_rot, d_scores, pass);
  else if (per <= 3) launch_score<3>(h, n, n_beams, sc, d_pairs, d_rot, d_scores, pass);
  else if (per <= 4) launch_score<4>(h, n, n_beams, sc, d_pairs, d_rot, d_scores, pass);
  else launch_score<5>(h, n, n_beams, sc, d_pairs, d_rot, d_scores, pass);
}

}  // namespace

namespace tbnav_icpdev {

void search_free(tbnav_icp* h) {
  IcpSearch& S = h->search;
  (void)hipFree(S.d_stamp);
  (void)hipFree(S.d_tables);
  (void)hipFree(S.d_in);
  (void)hipFree(S.d_rec);
  (void)hipFree(S.d_sel);
  (void)hipFree(S.d_tgt_points);
  (void)hipFree(S.d_scores);
  (void)hipFree(S.d_shape);
  S = IcpSearch{};
}

int search_pairs(tbnav_icp* h, int n_pairs, int n_beams, const tbnav_icp_search_params& sp, uint32_t* scores,
                 const tbnav_icp_search_shape_params* shp) {
  if (!params_ok(sp) || (shp && !shape_params_ok(*shp)) || n_beams <= 0 || n_beams > TBNAV_ICP_MAX_BEAMS || (scores && n_pairs != 1)) return TBNAV_ERR_INVALID_ARG;
  IcpSearch& S = h->search;
  const SearchConst sc = make_const(sp);
  if (int rc = ensure_stamp(h, sp)) return rc;
  h->h_sinfo.assign((size_t)n_pairs, tbnav_icp_search_info{});
  h->h_sshape.assign((size_t)n_pairs, tbnav_icp_search_shape{});
  const size_t vol = (size_t)sc.na * sc.nl * sc.nl;
  if (scores)
    if (int rc = ensure(S.d_scores, S.scores_cap, sizeof(uint32_t) * vol)) return rc;
  for (int first = 0; first < n_pairs; first += kChunk) {
    const int n = n_pairs - first < kChunk ? n_pairs - first : kChunk;
    // the chunk's pairs, then their rotations (cos, sin of theta_a in double, glibc), in one upload
    const size_t rot_at = (sizeof(SearchPair) * (size_t)n + 15) & ~(size_t)15;
    const size_t in_bytes = rot_at + sizeof(double2) * (size_t)n * sc.na;
    S.h_in.resize(in_bytes);
    SearchPair* hp = reinterpret_cast<SearchPair*>(S.h_in.data());
    double2* hr = reinterpret_cast<double2*>(S.h_in.data() + rot_at);
    for (int i = 0; i < n; ++i) {
      const IcpPair& pr = h->h_pairs[(size_t)(first + i)];
      const std::array<double, 3>& T = h->h_init[(size_t)(first + i)];
      hp[i].tgt = pr.tgt; hp[i].src = pr.src; hp[i].x0 = T[1]; hp[i].y0 = T[2];
      for (int ia = 0; ia < sc.na; ++ia) {
        const double th = T[0] + (double)(ia - sc.wa) * sp.ang_step;
        hr[(size_t)i * sc.na + ia] = make_double2(std::cos(th), std::sin(th));
      }
    }
    if (int rc = ensure(S.d_in, S.in_cap, in_bytes)) return rc;
    if (int rc = ensure(S.d_tables, S.tables_cap, (size_t)sc.tab_stride * (size_t)n)) return rc;
    if (int rc = ensure(S.d_rec, S.rec_cap, sizeof(SearchRec) * (size_t)n * sc.na)) return rc;
    if (int rc = ensure(S.d_sel, S.sel_cap, sizeof(SearchSel) * (size_t)n)) return rc;
    if (int rc = ensure(S.d_tgt_points, S.tgt_cap, sizeof(uint32_t) * (size_t)n)) return rc;
    TBNAV_HIP(hipMemcpyAsync(S.d_in, S.h_in.data(), in_bytes, hipMemcpyHostToDevice, h->stream));
    const SearchPair* d_pairs = static_cast<const SearchPair*>(S.d_in);
    const double2* d_rot = reinterpret_cast<const double2*>(static_cast<const unsigned char*>(S.d_in) + rot_at);
    hipLaunchKernelGGL(icp_search_table, dim3(n), dim3(kThreads), (size_t)sc.tab_stride, h->stream, h->d_scans, h->d_stored, h->d_table,
                       n_beams, d_pairs, S.d_stamp, S.d_tables, S.d_tgt_points, h->k, sc);
    TBNAV_HIP(hipGetLastError());
    dispatch_score(h, n, n_beams, sc, d_pairs, d_rot, scores ? S.d_scores : nullptr, 0);
    TBNAV_HIP(hipGetLastError());
    hipLaunchKernelGGL(icp_search_select, dim3(n), dim3(kWave), 0, h->stream, static_cast<const SearchRec*>(S.d_rec), S.d_tgt_points,
                       static_cast<SearchSel*>(S.d_sel), sc, 0);
    TBNAV_HIP(hipGetLastError());
    if (sc.slack) {
      dispatch_score(h, n, n_beams, sc, d_pairs, d_rot, nullptr, 1);
      TBNAV_HIP(hipGetLastError());
      hipLaunchKernelGGL(icp_search_select, dim3(n), dim3(kWave), 0, h->stream, static_cast<const SearchRec*>(S.d_rec), S.d_tgt_points,
                         static_cast<SearchSel*>(S.d_sel), sc, 1);
      TBNAV_HIP(hipGetLastError());
    }
    if (shp) {
      if (int rc = ensure(S.d_shape, S.shape_cap, sizeof(ShapeRec) * (size_t)n)) return rc;
      if (int rc = launch_shape(h, n, n_beams, sc, d_pairs, d_rot, *shp)) return rc;
      S.h_shape.resize(sizeof(ShapeRec) * (size_t)n);
      TBNAV_HIP(hipMemcpyAsync(S.h_shape.data(), S.d_shape, sizeof(ShapeRec) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
    }
    S.h_sel.resize(sizeof(SearchSel) * (size_t)n);
    TBNAV_HIP(hipMemcpyAsync(S.h_sel.data(), S.d_sel, sizeof(SearchSel) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
    if (scores) TBNAV_HIP(hipMemcpyAsync(scores, S.d_scores, sizeof(uint32_t) * vol, hipMemcpyDeviceToHost, h->stream));
    TBNAV_HIP(hipStreamSynchronize(h->stream));
    const SearchSel* hs = reinterpret_cast<const SearchSel*>(S.h_sel.data());
    for (int i = 0; i < n; ++i) {
      const SearchSel& s = hs[i];
      const std::array<double, 3>& T = h->h_init[(size_t)(first + i)];
      tbnav_icp_search_info& o = h->h_sinfo[(size_t)(first + i)];
      o.ia = (int32_t)(s.lin / (uint32_t)(sc.nl * sc.nl));
      o.iy = (int32_t)((s.lin / (uint32_t)sc.nl) % (uint32_t)sc.nl);
      o.ix = (int32_t)(s.lin % (uint32_t)sc.nl);
      o.T[0] = T[0] + (double)(o.ia - sc.wa) * sp.ang_step;
      o.T[1] = T[1] + (double)(o.ix - sc.wl) * sp.resolution;
      o.T[2] = T[2] + (double)(o.iy - sc.wl) * sp.resolution;
      o.score = s.score;
      o.points = (int32_t)s.points;
      o.candidates = (int32_t)s.count;
      o.quality = s.points ? (double)s.score / (255.0 * (double)s.points) : 0.0;
      o.at_edge = ((sc.wa > 0 && (o.ia == 0 || o.ia == sc.na - 1)) ||
                   (sc.wl > 0 && (o.iy == 0 || o.iy == sc.nl - 1 || o.ix == 0 || o.ix == sc.nl - 1))) ? 1 : 0;
      o.accepted = (o.quality >= sp.min_quality && s.points > 0u && s.tgt_points > 0u) ? 1 : 0;
      o.searched = 1;
      o.reserved = 0;
      if (shp)
        shape_finish(reinterpret_cast<const ShapeRec*>(S.h_shape.data())[i], sp, *shp, T.data(), &o, &h->h_sshape[(size_t)(first + i)]);
    }
  }
  return TBNAV_OK;
}

}  // namespace tbnav_icpdev

extern "C" {

void tbnav_icp_default_search_params(tbnav_icp_search_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof *p);
  p->resolution = 0.05;
  p->half_extent = 4.0;
  p->sigma = 0.05;
  p->ang_step = 3.14159265358979323846 / 180.0;
  p->min_quality = 0.5;
  p->stamp_cells = 3;
  p->lin_cells = 6;
  p->ang_steps = 20;
  p->slack_q10 = 0;
}

int tbnav_icp_set_search(tbnav_icp* h, const tbnav_icp_search_params* params) {
  if (!h) return TBNAV_ERR_INVALID_ARG;
  if (!params) {
    h->search.on = false;
    tbnav_icp_default_search_params(&h->search.p);
    return TBNAV_OK;
  }
  if (!params_ok(*params)) return TBNAV_ERR_INVALID_ARG;
  h->search.p = *params;
  h->search.on = true;
  return TBNAV_OK;
}

int tbnav_icp_get_search(const tbnav_icp* h, int32_t* on, tbnav_icp_search_params* params) {
  if (!h) return TBNAV_ERR_INVALID_ARG;
  if (on) *on = h->search.on ? 1 : 0;
  if (params) *params = h->search.p;
  return TBNAV_OK;
}

int tbnav_icp_last_search(const tbnav_icp* h, tbnav_icp_search_info* info) {
  if (!h || !info) return TBNAV_ERR_INVALID_ARG;
  *info = h->search.last;
  return TBNAV_OK;
}

namespace {

// the stateless entries: the search of one pair with the handle's parameters; the shape when the handle has it on, or when
// shape_out asks for it
int search_one(tbnav_icp* h, const float* target_scan, const float* source_scan, int32_t n_beams, const double T_init[3], double T_out[3],
               tbnav_icp_search_info* info, uint32_t* scores, tbnav_icp_search_shape* shape_out) {
  if (!h || !target_scan || !source_scan || !T_init || !T_out || !info || n_beams <= 0 || n_beams > TBNAV_ICP_MAX_BEAMS)
    return TBNAV_ERR_INVALID_ARG;
  DevGuard guard(h->device);
  if (!guard.ok) return TBNAV_ERR_NO_DEVICE;
  if (int rc = ensure_table(h, n_beams)) return rc;
  if (int rc = ensure_scans(h, 2 * (size_t)n_beams)) return rc;
  TBNAV_HIP(hipMemcpyAsync(h->d_scans, target_scan, sizeof(float) * (size_t)n_beams, hipMemcpyHostToDevice, h->stream));
  TBNAV_HIP(hipMemcpyAsync(h->d_scans + n_beams, source_scan, sizeof(float) * (size_t)n_beams, hipMemcpyHostToDevice, h->stream));
  IcpPair pr{};
  pr.tgt = 0; pr.src = 1;
  h->h_pairs.assign(1, pr);
  h->h_init.assign(1, {T_init[0], T_init[1], T_init[2]});
  const bool shape = h->search.shape_on || shape_out;
  if (int rc = search_pairs(h, 1, n_beams, h->search.p, scores, shape ? &h->search.shape_p : nullptr)) return rc;
  *info = h->h_sinfo[0];
  if (shape_out) *shape_out = h->h_sshape[0];
  T_out[0] = info->T[0]; T_out[1] = info->T[1]; T_out[2] = info->T[2];
  return TBNAV_OK;
}

}  // namespace

int tbnav_icp_search_scores(tbnav_icp* h, const float* target_scan, const float* source_scan, int32_t n_beams, const double T_init[3],
                            double T_out[3], tbnav_icp_search_info* info, uint32_t* scores) {
  return search_one(h, target_scan, source_scan, n_beams, T_init, T_out, info, scores, nullptr);
}

int tbnav_icp_search(tbnav_icp* h, const float* target_scan, const float* source_scan, int32_t n_beams, const double T_init[3],
                     double T_out[3], tbnav_icp_search_info* info) {
  return search_one(h, target_scan, source_scan, n_beams, T_init, T_out, info, nullptr, nullptr);
}

int tbnav_icp_search_with_shape(tbnav_icp* h, const float* target_scan, const float* source_scan, int32_t n_beams,
                                const double T_init[3], double T_out[3], tbnav_icp_search_info* info, tbnav_icp_search_shape* shape) {
  if (!shape) return TBNAV_ERR_INVALID_ARG;
  return search_one(h, target_scan, source_scan, n_beams, T_init, T_out, info, nullptr, shape);
}

int tbnav_icp_search_table(tbnav_icp* h, const float* scan, int32_t n_beams, uint8_t* table) {
  if (!h || !scan || !table || n_beams <= 0 || n_beams > TBNAV_ICP_MAX_BEAMS) return TBNAV_ERR_INVALID_ARG;
  DevGuard guard(h->device);
  if (!guard.ok) return TBNAV_ERR_NO_DEVICE;
  IcpSearch& S = h->search;
  const SearchConst sc = make_const(S.p);
  if (int rc = ensure_table(h, n_beams)) return rc;
  if (int rc = ensure_scans(h, (size_t)n_beams)) return rc;
  if (int rc = ensure_stamp(h, S.p)) return rc;
  if (int rc = ensure(S.d_in, S.in_cap, sizeof(SearchPair))) return rc;
  if (int rc = ensure(S.d_tables, S.tables_cap, (size_t)sc.tab_stride)) return rc;
  if (int rc = ensure(S.d_sel, S.sel_cap, sizeof(SearchSel))) return rc;
  if (int rc = ensure(S.d_tgt_points, S.tgt_cap, sizeof(uint32_t))) return rc;
  TBNAV_HIP(hipMemcpyAsync(h->d_scans, scan, sizeof(float) * (size_t)n_beams, hipMemcpyHostToDevice, h->stream));
  SearchPair pr{};
  pr.tgt = 0; pr.src = 0;
  TBNAV_HIP(hipMemcpyAsync(S.d_in, &pr, sizeof pr, hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(icp_search_table, dim3(1), dim3(kThreads), (size_t)sc.tab_stride, h->stream, h->d_scans, h->d_stored, h->d_table,
                     (int)n_beams, static_cast<const SearchPair*>(S.d_in), S.d_stamp, S.d_tables, S.d_tgt_points, h->k, sc);
  TBNAV_HIP(hipGetLastError());
  std::vector<uint8_t> padded((size_t)sc.tab_stride);
  TBNAV_HIP(hipMemcpyAsync(padded.data(), S.d_tables, padded.size(), hipMemcpyDeviceToHost, h->stream));
  TBNAV_HIP(hipStreamSynchronize(h->stream));
  for (int iy = 0; iy < sc.n; ++iy)
    std::memcpy(table + (size_t)iy * sc.n, padded.data() + (size_t)(iy + sc.wl) * sc.side + sc.wl, (size_t)sc.n);
  return TBNAV_OK;
}

}  // extern "C"

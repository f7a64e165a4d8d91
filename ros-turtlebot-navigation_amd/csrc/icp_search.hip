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
// its kernel is launched here behind the final icp_search_select and its record comes back with the selection.  What
// icp_search_score does before it scores (load_table, base_cells) and its read for a slow-list point (slow_read) are
// icp_search_device.hpp's scoring front, shared with that kernel.  On the host search_pairs walks the chunks in named steps
// (pack_chunk, reserve_chunk, launch_table, score_pass, launch_shape) and search_finish forms S7's record, as shape_finish
// forms F4 / F5's; every device buffer is a DevBuf (icp_device.hpp).  The wide second stage (W1-W8) is icp_search_wide.hip's:
// search_pairs collects the pairs W3 names behind a chunk's synchronisation and hands them to wide_stage.  The tables have one of
// two sources: target scans (launch_table, here) or the occupancy bits of a filter particle's map (MAP SEARCH, M1-M9:
// launch_table_from_occ, icp_search_map.hip, which writes the same padded layout); search_pairs is told which by its MapSource and
// shares everything else between them.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <utility>
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
  load_table(lds_tab, tables, pair, sc, t);
  if (t == 0) { n_fast = 0u; n_slow = 0u; n_valid = 0u; }
  __syncthreads();
  const SearchPair pr = pairs[pair];
  const double2 cs = rot[(size_t)pair * sc.na + ia];
  const float* ss = pr.src < 0 ? stored : scans + (size_t)pr.src * n_beams;
  const uint32_t valid = base_cells(ss, beams, n_beams, k, sc, cs, pr, cells, &n_fast, &n_slow, t);
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
#pragma unroll
    for (int j = 0; j < J; ++j) acc[j] += slow_read(tab, sc, v, iy[j], ix[j]);
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

// the device buffers of a chunk of n pairs whose upload is in_bytes long (d_shape: only where the shape runs)
int reserve_chunk(IcpSearch& S, int n, const SearchConst& sc, size_t in_bytes, bool shape) {
  const size_t m = (size_t)n;
  const std::pair<DevBuf*, size_t> want[] = {{&S.d_in, in_bytes},
                                             {&S.d_tables, (size_t)sc.tab_stride * m},
                                             {&S.d_rec, sizeof(SearchRec) * m * sc.na},
                                             {&S.d_sel, sizeof(SearchSel) * m},
                                             {&S.d_tgt_points, sizeof(uint32_t) * m},
                                             {&S.d_shape, shape ? sizeof(ShapeRec) * m : 0}};
  for (const auto& w : want)
    if (int rc = w.first->reserve(w.second)) return rc;
  return TBNAV_OK;
}

// icp_search_table over the n pairs at d_pairs -> d_tables, d_tgt_points
int launch_table(tbnav_icp* h, int n, int n_beams, const SearchConst& sc, const SearchPair* d_pairs) {
  IcpSearch& S = h->search;
  hipLaunchKernelGGL(icp_search_table, dim3(n), dim3(kThreads), (size_t)sc.tab_stride, h->stream, h->d_scans.as<float>(),
                     h->d_stored.as<float>(), h->d_table, n_beams, d_pairs, S.d_stamp, S.d_tables.as<uint8_t>(),
                     S.d_tgt_points.as<uint32_t>(), h->k, sc);
  TBNAV_HIP(hipGetLastError());
  return TBNAV_OK;
}

template <int J>
void launch_score(tbnav_icp* h, int n, int n_beams, const SearchConst& sc, const SearchPair* d_pairs, const double2* d_rot,
                  uint32_t* d_scores, int pass) {
  IcpSearch& S = h->search;
  hipLaunchKernelGGL((icp_search_score<J>), dim3(sc.na, n), dim3(kThreads), score_lds_bytes(sc, n_beams), h->stream,
                     h->d_scans.as<float>(), h->d_stored.as<float>(), h->d_table, n_beams, d_pairs, d_rot, S.d_tables.as<uint8_t>(),
                     S.d_sel.as<SearchSel>(), S.d_rec.as<SearchRec>(), d_scores, h->k, sc, pass);
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

// one pass over the chunk: every (pair, angle) scored, then the selection per pair
int score_pass(tbnav_icp* h, int n, int n_beams, const SearchConst& sc, const SearchPair* d_pairs, const double2* d_rot,
               uint32_t* d_scores, int pass) {
  IcpSearch& S = h->search;
  dispatch_score(h, n, n_beams, sc, d_pairs, d_rot, d_scores, pass);
  TBNAV_HIP(hipGetLastError());
  hipLaunchKernelGGL(icp_search_select, dim3(n), dim3(kWave), 0, h->stream, S.d_rec.as<SearchRec>(), S.d_tgt_points.as<uint32_t>(),
                     S.d_sel.as<SearchSel>(), sc, pass);
  TBNAV_HIP(hipGetLastError());
  return TBNAV_OK;
}

// h_in <- pairs [first, first + n) of h->h_pairs with their guesses h->h_init, then (at the offset returned, 16-byte aligned)
// their rotations (cos, sin of theta_a in double, glibc): one upload.  map (M5): the translation is the local guess, the angle stays
size_t pack_chunk(tbnav_icp* h, int first, int n, const SearchConst& sc, const tbnav_icp_search_params& sp, const MapSource* map) {
  IcpSearch& S = h->search;
  const size_t rot_at = (sizeof(SearchPair) * (size_t)n + 15) & ~(size_t)15;
  S.h_in.resize(rot_at + sizeof(double2) * (size_t)n * sc.na);
  SearchPair* hp = reinterpret_cast<SearchPair*>(S.h_in.data());
  double2* hr = reinterpret_cast<double2*>(S.h_in.data() + rot_at);
  for (int i = 0; i < n; ++i) {
    const IcpPair& pr = h->h_pairs[(size_t)(first + i)];
    const std::array<double, 3>& T = h->h_init[(size_t)(first + i)];
    hp[i].tgt = pr.tgt; hp[i].src = pr.src; hp[i].x0 = T[1]; hp[i].y0 = T[2];
    if (map) { hp[i].x0 = map->local[(size_t)(first + i)].x; hp[i].y0 = map->local[(size_t)(first + i)].y; }
    for (int ia = 0; ia < sc.na; ++ia) {
      const double th = T[0] + (double)(ia - sc.wa) * sp.ang_step;
      hr[(size_t)i * sc.na + ia] = make_double2(std::cos(th), std::sin(th));
    }
  }
  return rot_at;
}

}  // namespace

namespace tbnav_icpdev {

// S7 on the host: the record of one pair from its selection (shape_finish's counterpart)
void search_finish(const SearchSel& s, const SearchConst& sc, const tbnav_icp_search_params& sp, const double T_init[3],
                   tbnav_icp_search_info* info) {
  tbnav_icp_search_info& o = *info;
  o.ia = (int32_t)(s.lin / (uint32_t)(sc.nl * sc.nl));
  o.iy = (int32_t)((s.lin / (uint32_t)sc.nl) % (uint32_t)sc.nl);
  o.ix = (int32_t)(s.lin % (uint32_t)sc.nl);
  o.T[0] = T_init[0] + (double)(o.ia - sc.wa) * sp.ang_step;
  o.T[1] = T_init[1] + (double)(o.ix - sc.wl) * sp.resolution;
  o.T[2] = T_init[2] + (double)(o.iy - sc.wl) * sp.resolution;
  o.score = s.score;
  o.points = (int32_t)s.points;
  o.candidates = (int32_t)s.count;
  o.quality = s.points ? (double)s.score / (255.0 * (double)s.points) : 0.0;
  o.at_edge = ((sc.wa > 0 && (o.ia == 0 || o.ia == sc.na - 1)) ||
               (sc.wl > 0 && (o.iy == 0 || o.iy == sc.nl - 1 || o.ix == 0 || o.ix == sc.nl - 1))) ? 1 : 0;
  o.accepted = (o.quality >= sp.min_quality && s.points > 0u && s.tgt_points > 0u) ? 1 : 0;
  o.searched = 1;
  o.reserved = 0;
}

SearchConst search_const(const tbnav_icp_search_params& p) { return make_const(p); }
bool search_params_ok(const tbnav_icp_search_params& p) { return params_ok(p); }

void search_free(tbnav_icp* h) {
  IcpSearch& S = h->search;
  (void)hipFree(S.d_stamp);
  for (DevBuf* b : {&S.d_tables, &S.d_in, &S.d_rec, &S.d_sel, &S.d_tgt_points, &S.d_scores, &S.d_shape, &S.d_win, &S.d_wrec, &S.d_wsel,
                    &S.d_wshape, &S.d_wscores, &S.d_map_in}) b->release();
  if (S.map_ev) (void)hipEventDestroy(S.map_ev);
  S = IcpSearch{};
}

int search_pairs(tbnav_icp* h, int n_pairs, int n_beams, const tbnav_icp_search_params& sp, uint32_t* scores,
                 const tbnav_icp_search_shape_params* shp, const tbnav_icp_search_wide_params* wp, uint32_t* wide_scores,
                 const MapSource* map) {
  if (!params_ok(sp) || (shp && !shape_params_ok(*shp)) || n_beams <= 0 || n_beams > TBNAV_ICP_MAX_BEAMS || (scores && n_pairs != 1)) return TBNAV_ERR_INVALID_ARG;
  if ((wp && !wide_params_ok(*wp, sp)) || (wide_scores && (!wp || n_pairs != 1))) return TBNAV_ERR_INVALID_ARG;
  const bool first_stage = !(wp && wp->when == TBNAV_ICP_WIDE_ALWAYS);   // W2
  IcpSearch& S = h->search;
  SearchConst sc = make_const(sp);
  if (map) sc.E = map->E;                                                // M3: E' in S1's place
  if (!map)
    if (int rc = ensure_stamp(h, sp)) return rc;
  h->h_sinfo.assign((size_t)n_pairs, tbnav_icp_search_info{});
  h->h_sshape.assign((size_t)n_pairs, tbnav_icp_search_shape{});
  h->h_swide.assign((size_t)n_pairs, tbnav_icp_search_wide_info{});
  std::vector<int> esc;                                                  // W3: the chunk's pairs the wide stage runs for
  const size_t vol = (size_t)sc.na * sc.nl * sc.nl;
  if (scores)
    if (int rc = S.d_scores.reserve(sizeof(uint32_t) * vol)) return rc;
  for (int first = 0; first < n_pairs; first += kChunk) {
    const int n = n_pairs - first < kChunk ? n_pairs - first : kChunk;
    const size_t rot_at = pack_chunk(h, first, n, sc, sp, map);
    if (int rc = reserve_chunk(S, n, sc, S.h_in.size(), shp != nullptr)) return rc;
    TBNAV_HIP(hipMemcpyAsync(S.d_in.ptr, S.h_in.data(), S.h_in.size(), hipMemcpyHostToDevice, h->stream));
    const SearchPair* d_pairs = S.d_in.as<SearchPair>();
    const double2* d_rot = reinterpret_cast<const double2*>(S.d_in.as<unsigned char>() + rot_at);
    if (int rc = map ? launch_table_from_occ(h, first, n, sc, *map) : launch_table(h, n, n_beams, sc, d_pairs)) return rc;
    esc.clear();
    if (first_stage) {
      if (int rc = score_pass(h, n, n_beams, sc, d_pairs, d_rot, scores ? S.d_scores.as<uint32_t>() : nullptr, 0)) return rc;
      if (sc.slack)
        if (int rc = score_pass(h, n, n_beams, sc, d_pairs, d_rot, nullptr, 1)) return rc;
      if (shp) {
        if (int rc = launch_shape(h, n, n_beams, sc, d_pairs, d_rot, *shp)) return rc;
        S.h_shape.resize(sizeof(ShapeRec) * (size_t)n);
        TBNAV_HIP(hipMemcpyAsync(S.h_shape.data(), S.d_shape.ptr, S.h_shape.size(), hipMemcpyDeviceToHost, h->stream));
      }
      S.h_sel.resize(sizeof(SearchSel) * (size_t)n);
      TBNAV_HIP(hipMemcpyAsync(S.h_sel.data(), S.d_sel.ptr, S.h_sel.size(), hipMemcpyDeviceToHost, h->stream));
      if (scores) TBNAV_HIP(hipMemcpyAsync(scores, S.d_scores.ptr, sizeof(uint32_t) * vol, hipMemcpyDeviceToHost, h->stream));
      TBNAV_HIP(hipStreamSynchronize(h->stream));
      for (int i = 0; i < n; ++i) {
        const double* T_init = h->h_init[(size_t)(first + i)].data();
        tbnav_icp_search_info* info = &h->h_sinfo[(size_t)(first + i)];
        search_finish(reinterpret_cast<const SearchSel*>(S.h_sel.data())[i], sc, sp, T_init, info);
        if (shp) shape_finish(reinterpret_cast<const ShapeRec*>(S.h_shape.data())[i], sp, *shp, T_init, info, &h->h_sshape[(size_t)(first + i)]);
        if (wp) {
          h->h_swide[(size_t)(first + i)].first = *info;
          if (!info->accepted || (wp->when == TBNAV_ICP_WIDE_ON_REJECT_OR_EDGE && info->at_edge)) esc.push_back(i);
        }
      }
    } else {
      for (int i = 0; i < n; ++i) esc.push_back(i);
    }
    // the wide stage, with the chunk's tables still on the device: further launches and one more synchronisation, and only
    // when a pair escalated
    if (!esc.empty()) {
      if (int rc = wide_stage(h, first, esc, n_beams, sp, sc, d_pairs, *wp, wide_scores, shp)) return rc;
      for (int i : esc) h->h_swide[(size_t)(first + i)].ran = 1;
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
    tbnav_icp_search_params def;
    tbnav_icp_default_search_params(&def);
    if (h->search.wide_on && !wide_params_ok(h->search.wide_p, def)) return TBNAV_ERR_INVALID_ARG;   // W1
    h->search.on = false;
    h->search.p = def;
    return TBNAV_OK;
  }
  if (!params_ok(*params)) return TBNAV_ERR_INVALID_ARG;
  if (h->search.wide_on && !wide_params_ok(h->search.wide_p, *params)) return TBNAV_ERR_INVALID_ARG;     // W1
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
               tbnav_icp_search_info* info, uint32_t* scores, tbnav_icp_search_shape* shape_out, bool wide_hook = false,
               uint32_t* wide_scores = nullptr) {
  if (!h || !target_scan || !source_scan || !T_init || !T_out || !info || n_beams <= 0 || n_beams > TBNAV_ICP_MAX_BEAMS)
    return TBNAV_ERR_INVALID_ARG;
  DeviceGuard guard(h->device);
  if (!guard.ok) return TBNAV_ERR_NO_DEVICE;
  if (int rc = ensure_table(h, n_beams)) return rc;
  if (int rc = h->d_scans.reserve(sizeof(float) * 2 * (size_t)n_beams)) return rc;
  TBNAV_HIP(hipMemcpyAsync(h->d_scans.ptr, target_scan, sizeof(float) * (size_t)n_beams, hipMemcpyHostToDevice, h->stream));
  TBNAV_HIP(hipMemcpyAsync(h->d_scans.as<float>() + n_beams, source_scan, sizeof(float) * (size_t)n_beams, hipMemcpyHostToDevice, h->stream));
  IcpPair pr{};
  pr.tgt = 0; pr.src = 1;
  h->h_pairs.assign(1, pr);
  h->h_init.assign(1, {T_init[0], T_init[1], T_init[2]});
  const bool shape = h->search.shape_on || shape_out;
  // the wide stage: as the handle has it (W7; the first stage's own hook, which asks for its volume, ignores it), or alone (W8)
  tbnav_icp_search_wide_params wp = h->search.wide_p;
  if (wide_hook) wp.when = TBNAV_ICP_WIDE_ALWAYS;
  const bool wide = wide_hook || (h->search.wide_on && !scores);
  if (int rc = search_pairs(h, 1, n_beams, h->search.p, scores, shape ? &h->search.shape_p : nullptr, wide ? &wp : nullptr, wide_scores)) return rc;
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

int tbnav_icp_search_wide_scores(tbnav_icp* h, const float* target_scan, const float* source_scan, int32_t n_beams,
                                 const double T_init[3], double T_out[3], tbnav_icp_search_info* info, uint32_t* scores) {
  return search_one(h, target_scan, source_scan, n_beams, T_init, T_out, info, nullptr, nullptr, true, scores);
}

int tbnav_icp_search_table(tbnav_icp* h, const float* scan, int32_t n_beams, uint8_t* table) {
  if (!h || !scan || !table || n_beams <= 0 || n_beams > TBNAV_ICP_MAX_BEAMS) return TBNAV_ERR_INVALID_ARG;
  DeviceGuard guard(h->device);
  if (!guard.ok) return TBNAV_ERR_NO_DEVICE;
  IcpSearch& S = h->search;
  const SearchConst sc = make_const(S.p);
  if (int rc = ensure_table(h, n_beams)) return rc;
  if (int rc = h->d_scans.reserve(sizeof(float) * (size_t)n_beams)) return rc;
  if (int rc = ensure_stamp(h, S.p)) return rc;
  if (int rc = reserve_chunk(S, 1, sc, sizeof(SearchPair), false)) return rc;
  TBNAV_HIP(hipMemcpyAsync(h->d_scans.ptr, scan, sizeof(float) * (size_t)n_beams, hipMemcpyHostToDevice, h->stream));
  SearchPair pr{};
  pr.tgt = 0; pr.src = 0;
  TBNAV_HIP(hipMemcpyAsync(S.d_in.ptr, &pr, sizeof pr, hipMemcpyHostToDevice, h->stream));
  if (int rc = launch_table(h, 1, n_beams, sc, S.d_in.as<SearchPair>())) return rc;
  std::vector<uint8_t> padded((size_t)sc.tab_stride);
  TBNAV_HIP(hipMemcpyAsync(padded.data(), S.d_tables.ptr, padded.size(), hipMemcpyDeviceToHost, h->stream));
  TBNAV_HIP(hipStreamSynchronize(h->stream));
  for (int iy = 0; iy < sc.n; ++iy)
    std::memcpy(table + (size_t)iy * sc.n, padded.data() + (size_t)(iy + sc.wl) * sc.side + sc.wl, (size_t)sc.n);
  return TBNAV_OK;
}

}  // extern "C"

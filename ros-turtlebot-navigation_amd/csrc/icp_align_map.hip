// icp_align_map.hip — the alignment of one scan to a filter particle's MAP below one cell (include/tbnav_icp.h, MAP ALIGNMENT,
// items A1-A11; an addition with no counterpart in the reference; restated in tests/icp_align_map_restatement.py and reproduced bit
// for bit).  The last link of global search -> window search -> alignment: a point-to-line Gauss-Newton iteration whose lines are
// fitted to the occupied cells round the nearest one.
//   icp_align_map<P>  one workgroup of 256 threads per pair, the whole iteration loop in one launch, in icp_align's shape.
//     Staging: the window's 2H x 2H occupancy bits into LDS, row r = map row cx - H + r, one zero word in front of and one behind
//     each row's ceil(2H / 32) words (a 64-bit look at any column +-16 then needs no bounds test along the row); read through the
//     particle's tile table by occ_row_window (icp_search_device.hpp: tile id 0, tiles outside the map and a ragged last tile
//     read as empty).  At most 512 rows of 18 words: 36 KB, beside 16 KB for the tree.
//     Source: thread t keeps beams t, t + 256, ... (P of them) in registers, untransformed.
//     Iteration: transform, home cell, the nearest occupied cell by rows outwards (clz / ffs on the masked 64-bit look; one
//     integer key D << 20 | row << 10 | column settles A5's tie rule, and the loop goes on while dr^2 <= the best D, since a row at
//     dr^2 == D can still win by its lower index), the cell's feature from its (2w + 1)^2 bits on the fly, the line metric's
//     sums, tree and step (icp_iter_device.hpp, shared with icp_align).  LDS and registers only; no atomics.
// Compiled with -ffp-contract=off (csrc/Makefile).
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "icp_device.hpp"
#include "icp_iter_device.hpp"
#include "icp_search_device.hpp"
#include "nav_host.hpp"
#include "tbnav_icp.h"

namespace {

using namespace tbnav_icpdev;

constexpr int kMaxGate = 16;   // A1a's largest G: a look of 2G + 1 <= 33 bits from a bit offset <= 31 fits in 64

struct AlignMapArgs {
  const unsigned int* bm;      // TilePool::bm
  const unsigned int* table;   // [N][TT] the particles' tile tables
  const int* best;             // the filter's arg-max on the device (rbpf_argmax), read where a pair asks for it
  int TW, TT, side;            // tiles per side and per map, cells per side
  double xmin, ymin, inv, res; // A2
  int H, G, w;                 // A1a
  double f;                    // max_flatness
  double min_cond;             // L4's K
};

struct AlignMapPair {
  int32_t particle;            // a slot, or TBNAV_ICP_MAP_BEST_PARTICLE
  int32_t cx, cy;              // the cell of T_init (A3)
  int32_t pad;
  double c, s, x, y;           // item 2's float-rounded guess
};

// 64 bits of window row `row` (its first pad word included) from bit position p
__device__ __forceinline__ unsigned long long look(const uint32_t* row, int p) {
  const int w = p >> 5, o = p & 31;
  return ((((unsigned long long)row[w + 1]) << 32) | row[w]) >> o;
}

// A5: the occupied cell of the window nearest local cell (hr, hc) within +-G rows and columns, as the key D << 20 | row << 10 |
// column (the least key IS the least D, then the lowest mi, then the lowest mj); 0xffffffff: none
__device__ __forceinline__ uint32_t nearest_cell(const uint32_t* win, int W, int rows, int hr, int hc, int G) {
  const uint32_t m = (1u << (G + 1)) - 1u;
  uint32_t best = 0xffffffffu;
  for (int dr = 0; dr <= G && (uint32_t)(dr * dr) <= (best >> 20); ++dr) {
    for (int s = 0; s < (dr == 0 ? 1 : 2); ++s) {
      const int r = s ? hr + dr : hr - dr;
      if (r < 0 || r >= rows) continue;
      const unsigned long long v = look(win + r * W, hc + 32 - G);   // bit q: column offset q - G
      const uint32_t left = (uint32_t)v & m;                         // offsets -G .. 0
      const uint32_t right = (uint32_t)(v >> G) & m;                 // offsets 0 .. G
      if (left) {
        const int dc = G - (31 - __clz((int)left));
        const uint32_t key = ((uint32_t)(dr * dr + dc * dc) << 20) | ((uint32_t)r << 10) | (uint32_t)(hc - dc);
        best = key < best ? key : best;
      }
      if (right) {
        const int dc = __ffs((int)right) - 1;
        const uint32_t key = ((uint32_t)(dr * dr + dc * dc) << 20) | ((uint32_t)r << 10) | (uint32_t)(hc + dc);
        best = key < best ? key : best;
      }
    }
  }
  return best;
}

// A4: the feature of the occupied local cell (mr, mc): its centroid (bx, by) and, when it has one, its normal; map cell = (wx0 + mr, wy0 + mc)
__device__ __forceinline__ bool cell_feature(const uint32_t* win, int W, int rows, int mr, int mc, int wx0, int wy0, const AlignMapArgs& a,
                                             double& bx, double& by, float2& nrm) {
  const int w = a.w;
  const uint32_t m = (1u << (2 * w + 1)) - 1u;
  int n = 0, sx = 0, sy = 0, sxx = 0, sxy = 0, syy = 0;
  for (int di = -w; di <= w; ++di) {
    const int r = mr + di;
    if (r < 0 || r >= rows) continue;
    uint32_t bits = (uint32_t)look(win + r * W, mc + 32 - w) & m;   // bit q: column offset q - w
    while (bits) {
      const int dj = __ffs((int)bits) - 1 - w;
      bits &= bits - 1u;
      ++n; sx += di; sy += dj; sxx += di * di; sxy += di * dj; syy += dj * dj;
    }
  }
  const int ia = n * sxx - sx * sx, ic = n * syy - sy * sy, ib = n * sxy - sx * sy;
  bx = a.xmin + (((double)(wx0 + mr) + 0.5) + ((double)sx / (double)n)) * a.res;
  by = a.ymin + (((double)(wy0 + mc) + 0.5) + ((double)sy / (double)n)) * a.res;
  const double hd = 0.5 * (double)(ia - ic);
  const double dd = sqrt((hd * hd) + ((double)ib * (double)ib));
  const double lmin = (0.5 * (double)(ia + ic)) - dd;
  const double lmax = (0.5 * (double)(ia + ic)) + dd;
  nrm = make_float2(0.0f, 0.0f);
  if (!(n >= 3 && lmax > 0.0 && lmin <= a.f * lmax)) return false;
  double vx, vy;
  if (ib != 0) { vx = (double)ib; vy = lmin - (double)ia; }
  else if (ia >= ic) { vx = 0.0; vy = 1.0; }
  else { vx = 1.0; vy = 0.0; }
  const double l = sqrt((vx * vx) + (vy * vy));
  nrm = make_float2((float)(vx / l), (float)(vy / l));
  return true;
}

// blockIdx.x: the pair.  recs: the test hook's pairing record of this launch's iterations [n_beams] (one pair, max_iter = 1), or null
template <int P>
__global__ __launch_bounds__(kThreads) void icp_align_map(AlignMapArgs a, const AlignMapPair* __restrict__ pairs, const float* __restrict__ scan,
                                                           const float2* __restrict__ beams, int n_beams, IcpOut* __restrict__ out, IcpConst k,
                                                           tbnav_icp_align_map_pair* __restrict__ recs) {
  extern __shared__ uint32_t win[];          // [rows][W]
  __shared__ TreeLds<kLineSums> tree;
  const int t = threadIdx.x;
  const AlignMapPair pr = pairs[blockIdx.x];
  const int rows = 2 * a.H, nw = (rows + 31) >> 5, W = nw + 2;
  const int wx0 = pr.cx - a.H, wy0 = pr.cy - a.H;   // the map cell of the window's cell (0, 0)
  const unsigned int* __restrict__ ids = a.table + (size_t)(pr.particle < 0 ? *a.best : pr.particle) * a.TT;
  for (int idx = t; idx < rows * W; idx += kThreads) {
    const int r = idx / W, q = idx - r * W - 1;     // word q of the row's bits; -1 and nw: the zero words either side
    uint32_t v = 0u;
    if (q >= 0 && q < nw) {
      v = (uint32_t)occ_row_window(a.bm, ids, a.TW, a.side, wx0 + r, wy0 + 32 * q);
      const int rem = rows - 32 * q;                // columns of this word that are cells of the window (>= 1)
      if (rem < 32) v &= (1u << rem) - 1u;
    }
    win[idx] = v;
  }
  float2 src[P];
  bool valid[P];
#pragma unroll
  for (int j = 0; j < P; ++j) {
    const int i = t + j * kThreads;
    valid[j] = i < n_beams && cloud_point(scan[i], beams[i], k, src[j]);
    if (!valid[j]) src[j] = make_float2(0.0f, 0.0f);
  }
  __syncthreads();

  const double fx0 = (double)wx0, fx1 = (double)(wx0 + rows), fy0 = (double)wy0, fy1 = (double)(wy0 + rows);
  const int gate = a.G * a.G;
  IcpState st{pr.c, -pr.s, pr.s, pr.c, pr.x, pr.y, DBL_MAX};
  double mse = 0.0;
  int iter = 0, n = 0, crit = TBNAV_ICP_NOT_RUN;
  while (true) {
    ++iter;
    double sum[kLineSums];
#pragma unroll
    for (int q = 0; q < kLineSums; ++q) sum[q] = 0.0;
    int cnt = 0;
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const int i = t + j * kThreads;
      tbnav_icp_align_map_pair rec{};
      rec.mi = rec.mj = rec.D = -1;
      if (valid[j]) {
        const float ax = (float)(((st.R00 * (double)src[j].x) + (st.R01 * (double)src[j].y)) + st.tx);
        const float ay = (float)(((st.R10 * (double)src[j].x) + (st.R11 * (double)src[j].y)) + st.ty);
        const double fi = floor(((double)ax - a.xmin) * a.inv), fj = floor(((double)ay - a.ymin) * a.inv);
        if (fi >= fx0 && fi < fx1 && fj >= fy0 && fj < fy1) {   // (a NaN is outside)
          const int hr = (int)fi - wx0, hc = (int)fj - wy0;
          rec.has_home = 1; rec.hi = (int)fi; rec.hj = (int)fj;
          const uint32_t key = nearest_cell(win, W, rows, hr, hc, a.G);
          if (key != 0xffffffffu) {
            const int D = (int)(key >> 20), mr = (int)((key >> 10) & 1023u), mc = (int)(key & 1023u);
            rec.mi = wx0 + mr; rec.mj = wy0 + mc; rec.D = D;
            if (D <= gate || recs) {
              double bx, by;
              float2 nf;
              const bool has = cell_feature(win, W, rows, mr, mc, wx0, wy0, a, bx, by, nf);
              rec.bx = bx; rec.by = by; rec.nx = nf.x; rec.ny = nf.y; rec.has_normal = has ? 1 : 0;
              if (D <= gate && has) {
                line_add(sum, (double)ax, (double)ay, bx, by, (double)nf.x, (double)nf.y);
                ++cnt;
                rec.kept = 1;
              }
            }
          }
        }
      }
      if (recs && i < n_beams) recs[i] = rec;
    }
    tree_totals(tree, sum, cnt, t);
    n = tree.tot_n;
    if (n < 3) { crit = TBNAV_ICP_NO_CORRESPONDENCES; mse = 0.0; break; }
    double c = 0.0, s = 0.0, tix = 0.0, tiy = 0.0;
    if (!line_step(tree.tot, n, a.min_cond, c, s, tix, tiy, mse)) { crit = TBNAV_ICP_DEGENERATE; break; }
    crit = advance(st, c, s, tix, tiy, mse, iter, k);
    if (crit != TBNAV_ICP_NOT_RUN) break;
  }
  if (t == 0) {
    IcpOut o;
    o.R00 = st.R00; o.R10 = st.R10; o.tx = st.tx; o.ty = st.ty; o.mse = mse;
    o.iterations = iter; o.correspondences = n; o.criterion = crit; o.pad = 0;
    out[blockIdx.x] = o;
  }
}

bool params_ok(const tbnav_icp_align_map_params& p) {
  return p.half_cells >= 8 && p.half_cells <= TBNAV_ICP_ALIGN_MAP_MAX_HALF && p.gate_cells >= 1 && p.gate_cells <= kMaxGate &&
         p.feature_cells >= 1 && p.feature_cells <= 4 && std::isfinite(p.max_flatness) && p.max_flatness >= 0.0 && p.max_flatness < 1.0 &&
         p.reserved == 0;
}

template <int P>
void launch(tbnav_icp* h, const AlignMapArgs& a, int n, int n_beams, const IcpConst& k, tbnav_icp_align_map_pair* recs) {
  const int rows = 2 * a.H;
  const size_t lds = sizeof(uint32_t) * (size_t)rows * (size_t)(((rows + 31) >> 5) + 2);
  hipLaunchKernelGGL((icp_align_map<P>), dim3(n), dim3(kThreads), lds, h->stream, a, h->d_align_in.as<AlignMapPair>(), h->d_scans.as<float>(),
                     h->d_table, n_beams, h->d_out.as<IcpOut>(), k, recs);
  h->align_map_p = P;
}

// the entries' common body.  recs: the test hook (n == 1): iteration 1 alone, and its pairing record [n_beams]
int align_map(tbnav_icp* h, tbnav_rbpf* pf, const float* scan, int32_t n_beams, int32_t n, const int32_t* particles, const double* T_init,
              const tbnav_icp_align_map_params* params, double* T_out, int32_t* ok, tbnav_icp_info* infos, tbnav_icp_align_map_pair* recs) {
  // A1: arguments, parameters and particles; then device and group; then the guesses (A3).  Nothing is changed before the last passes.
  if (!h || !pf || !scan || !particles || !T_init || n < 1 || n_beams <= 0 || n_beams > TBNAV_ICP_MAX_BEAMS) return TBNAV_ERR_INVALID_ARG;
  if (recs ? false : (!T_out || !ok || !infos)) return TBNAV_ERR_INVALID_ARG;
  tbnav_icp_align_map_params p;
  tbnav_icp_default_align_map_params(&p);
  if (params) p = *params;
  if (!params_ok(p)) return TBNAV_ERR_INVALID_ARG;
  for (int i = 0; i < n; ++i)
    if (!tbnav_nk::particle_ok(pf, particles[i])) return TBNAV_ERR_INVALID_ARG;
  if (h->device != pf->device || pf->comm) return TBNAV_ERR_UNSUPPORTED;
  const double inv = 1.0 / pf->p.resolution;
  std::vector<AlignMapPair> pairs((size_t)n);
  bool best = false;
  for (int i = 0; i < n; ++i) {
    const double* T = T_init + 3 * (size_t)i;
    if (!std::isfinite(T[0]) || !std::isfinite(T[1]) || !std::isfinite(T[2])) return TBNAV_ERR_OUT_OF_WORLD;
    const double fx = std::floor((T[1] - pf->p.xmin) * inv), fy = std::floor((T[2] - pf->p.ymin) * inv);
    if (!(fx >= 0.0 && fx < (double)pf->xsize && fy >= 0.0 && fy < (double)pf->xsize)) return TBNAV_ERR_OUT_OF_WORLD;
    AlignMapPair& q = pairs[(size_t)i];
    q.particle = particles[i]; q.cx = (int)fx; q.cy = (int)fy; q.pad = 0;
    q.c = (double)(float)std::cos(T[0]);   // item 2
    q.s = (double)(float)std::sin(T[0]);
    q.x = (double)(float)T[1];
    q.y = (double)(float)T[2];
    best = best || particles[i] == TBNAV_ICP_MAP_BEST_PARTICLE;
  }
  DeviceGuard guard(h->device);
  if (!guard.ok) return TBNAV_ERR_NO_DEVICE;
  if (int rc = ensure_table(h, n_beams)) return rc;
  if (int rc = h->d_scans.reserve(sizeof(float) * (size_t)n_beams)) return rc;
  if (int rc = h->d_align_in.reserve(sizeof(AlignMapPair) * (size_t)n)) return rc;
  if (int rc = h->d_out.reserve(sizeof(IcpOut) * (size_t)n)) return rc;
  if (recs)
    if (int rc = h->d_align_rec.reserve(sizeof(tbnav_icp_align_map_pair) * (size_t)n_beams)) return rc;
  TBNAV_HIP(hipMemcpyAsync(h->d_scans.ptr, scan, sizeof(float) * (size_t)n_beams, hipMemcpyHostToDevice, h->stream));
  TBNAV_HIP(hipMemcpyAsync(h->d_align_in.ptr, pairs.data(), sizeof(AlignMapPair) * (size_t)n, hipMemcpyHostToDevice, h->stream));
  // A9: behind whatever the filter's stream has in flight, the arg-max of its weights included where a pair asks for it
  if (best)
    if (int rc = tbnav_nk::enqueue_best(pf, TBNAV_NAV_BEST_PARTICLE)) return rc;
  IcpSearch& S = h->search;
  if (!S.map_ev) TBNAV_HIP(hipEventCreateWithFlags(&S.map_ev, hipEventDisableTiming));
  TBNAV_HIP(hipEventRecord(S.map_ev, pf->stream));
  TBNAV_HIP(hipStreamWaitEvent(h->stream, S.map_ev, 0));
  const AlignMapArgs a{pf->pool.bm, pf->d_table[pf->cur], pf->d_best, pf->TW, pf->TT, pf->xsize, pf->p.xmin, pf->p.ymin, inv, pf->p.resolution,
                       p.half_cells, p.gate_cells, p.feature_cells, p.max_flatness, TBNAV_ICP_LINE_MIN_COND};
  IcpConst k = h->k;
  if (recs) k.max_iter = 1;
  tbnav_icp_align_map_pair* d_recs = recs ? h->d_align_rec.as<tbnav_icp_align_map_pair>() : nullptr;
  const int per = (n_beams + kThreads - 1) / kThreads;
  static_assert(TBNAV_ICP_MAX_BEAMS <= 16 * kThreads, "no instantiation holds TBNAV_ICP_MAX_BEAMS");
  if (per <= 1) launch<1>(h, a, n, n_beams, k, d_recs);
  else if (per <= 2) launch<2>(h, a, n, n_beams, k, d_recs);
  else if (per <= 4) launch<4>(h, a, n, n_beams, k, d_recs);
  else if (per <= 6) launch<6>(h, a, n, n_beams, k, d_recs);
  else if (per <= 8) launch<8>(h, a, n, n_beams, k, d_recs);
  else launch<16>(h, a, n, n_beams, k, d_recs);
  TBNAV_HIP(hipGetLastError());
  std::vector<IcpOut> outs((size_t)n);
  TBNAV_HIP(hipMemcpyAsync(outs.data(), h->d_out.ptr, sizeof(IcpOut) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
  if (recs) TBNAV_HIP(hipMemcpyAsync(recs, d_recs, sizeof(tbnav_icp_align_map_pair) * (size_t)n_beams, hipMemcpyDeviceToHost, h->stream));
  TBNAV_HIP(hipStreamSynchronize(h->stream));
  if (recs) return TBNAV_OK;
  for (int i = 0; i < n; ++i) {
    const IcpOut& o = outs[(size_t)i];
    const bool conv = o.criterion >= TBNAV_ICP_ITERATIONS && o.criterion <= TBNAV_ICP_REL_MSE;
    double* T = T_out + 3 * (size_t)i;
    if (conv) {
      T[0] = std::atan2(o.R10, o.R00);   // item 5
      T[1] = o.tx;
      T[2] = o.ty;
    } else {                             // A7: the guess, unchanged
      for (int q = 0; q < 3; ++q) T[q] = T_init[3 * (size_t)i + q];
    }
    ok[i] = conv ? 1 : 0;
    infos[i] = tbnav_icp_info{o.iterations, o.correspondences, o.mse, o.criterion, 0};
  }
  return TBNAV_OK;
}

}  // namespace

extern "C" {

void tbnav_icp_default_align_map_params(tbnav_icp_align_map_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof *p);
  p->max_flatness = 0.25;
  p->half_cells = 128;
  p->gate_cells = 10;
  p->feature_cells = 2;
}

int tbnav_icp_align_map(tbnav_icp* h, tbnav_rbpf* pf, int32_t particle, const float* scan, int32_t n_beams, const double T_init[3],
                        const tbnav_icp_align_map_params* params, double T_out[3], int32_t* ok, tbnav_icp_info* info) {
  return align_map(h, pf, scan, n_beams, 1, &particle, T_init, params, T_out, ok, info, nullptr);
}

int tbnav_icp_align_map_batch(tbnav_icp* h, tbnav_rbpf* pf, const float* scan, int32_t n_beams, int32_t n, const int32_t* particles,
                              const double* T_init, const tbnav_icp_align_map_params* params, double* T_out, int32_t* ok,
                              tbnav_icp_info* infos) {
  return align_map(h, pf, scan, n_beams, n, particles, T_init, params, T_out, ok, infos, nullptr);
}

int tbnav_icp_align_map_pairs(tbnav_icp* h, tbnav_rbpf* pf, int32_t particle, const float* scan, int32_t n_beams, const double T_init[3],
                              const tbnav_icp_align_map_params* params, tbnav_icp_align_map_pair* pairs) {
  if (!pairs) return TBNAV_ERR_INVALID_ARG;
  return align_map(h, pf, scan, n_beams, 1, &particle, T_init, params, nullptr, nullptr, nullptr, pairs);
}

int tbnav_icp_last_align_map_kernel(const tbnav_icp* h, char* kernel, int32_t kernel_cap) {
  if (!h || !kernel || kernel_cap <= 0) return TBNAV_ERR_INVALID_ARG;
  if (h->align_map_p) std::snprintf(kernel, (size_t)kernel_cap, "icp_align_map<%d>", h->align_map_p);
  else kernel[0] = '\0';
  return TBNAV_OK;
}

}  // extern "C"

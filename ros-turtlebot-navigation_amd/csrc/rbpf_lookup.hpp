// rbpf_lookup.hpp — where a likelihood lookup gets its distance code (device code only): the particle's stored field, or, in
// query mode, the exact nearest-obstacle search on its occupancy bitmap — the 7 x 7 look on the slice of the bitmap a workgroup
// holds in LDS, then the row walks on the slice and on the global bitmap — and the staging of that slice.  Used by the one-pose
// likelihood, the scan matcher and the proposal kernel (rbpf_propose.hip).
#ifndef TBNAV_RBPF_LOOKUP_HPP
#define TBNAV_RBPF_LOOKUP_HPP
#include "rbpf_device.hpp"

namespace tbnav_rk {

// Where a lookup gets its distance code from.
//  field  : the particle's u16 field is authoritative (injected, or whole-field fresh) -> read it
//  window : the field was refreshed inside `win` for this call -> read it, report a lookup outside the window
//  query  : no field refresh at all — the squared distance to the nearest occupied cell is computed from the
//           occupancy bitmap at the looked-up cell: rows i, i+-1, i+-2, ... each contribute (dr^2 + nearest set
//           bit in that row)^2 and the walk stops once dr^2 >= best.  A beam ends on or next to a wall, so this
//           is a handful of rows; the result is the exact transform's value (same integer arithmetic), and a
//           cell with no obstacle within cell_radius keeps its stored code, like the transform.
struct DistSrc {
  const uint16_t* code;             // [G] of the particle; NULL when the handle keeps no stored field (query mode only)
  OccT occ;                         // the particle's occupancy bits (tiled)
  int4 win;
  int mode;                         // 0 field, 1 window, 2 query
  // query mode, optional: the part of the bitmap round the particle held in LDS (rows R0..R1, 64-cell word
  // columns W0..W0+nW-1; any[r] = row r has a set bit inside those columns).  nW == 0: no slice.
  const unsigned long long* tbm;
  const int* tany;
  int R0, R1, W0, nW;
  // optional, with the LDS slice: lut7[m] = least (c - 3)^2 over the set bits c of the 7-bit pattern m (100: none) — lets a
  // lookup read the 7 x 7 cells round it as seven table look-ups instead of seven 64-column bit scans
  const unsigned char* lut7;
  // reference-field mode: where a stored-field lookup that reads kCodePending leaves cell + 1 (NULL: nobody asks)
  int* pend;
};
// a stored code as the lookups read it: a pending cell (the reference-field mode's lazy brushfire has not written it) is reported
__device__ __forceinline__ uint16_t stored_code(const GridC& g, const DistSrc& d, int ci, int cj) {
  const uint16_t v = d.code[(size_t)ci * g.xsize + cj];
  if (v == kCodePending && d.pend) *d.pend = ci * g.xsize + cj + 1;
  return v;
}
// Walk rows i, i+-1, i+-2, ... of an occupancy bitmap (stride `words` u64 per row, rows row_lo..row_hi present,
// cell columns [0, words*64) relative to the bitmap) and return the least squared distance found (INT_MAX: none
// within `radius`).  row_any(r) says whether row r can hold a set bit.
template <class RowWord, class RowAny>
__device__ __forceinline__ int nearest_d2_rows(RowWord row_word, int words, int row_lo, int row_hi, int radius,
                                               int ci, int cj, RowAny row_any) {
  int best = 0x7fffffff;
  for (int dr = 0; dr <= radius; ++dr) {
    if (dr * dr >= best) break;
    if (ci + dr > row_hi && ci - dr < row_lo) break;
    for (int sg = 0; sg < (dr ? 2 : 1); ++sg) {
      const int r = sg ? ci - dr : ci + dr;
      if (r < row_lo || r > row_hi || !row_any(r)) continue;
      int cap = radius;
      if (best != 0x7fffffff) { cap = (int)sqrtf((float)(best - dr * dr)) + 1; cap = cap < radius ? cap : radius; }
      const int f = row_nearest_f([&](int w) { return row_word(r, w); }, words, cj, cap);
      if (f != 255) { const int cand = dr * dr + f * f; best = cand < best ? cand : best; }
    }
  }
  return best;
}

// ---- the query mode's search ----------------------------------------------------------------------------------------------
// How far the nearest cell OUTSIDE the slice is from (ci, cj), a cell of the slice, at least: a side of the slice that is not
// the map's own border is (distance to that side + 1) cells away, and nothing beyond the radius matters.  What the slice shows
// within `clear` cells is the map's answer.
__device__ __forceinline__ int tile_clear(const GridC& g, const DistSrc& d, int radius, int ci, int cj) {
  const int C0 = d.W0 * 64, C1 = (d.W0 + d.nW) * 64 - 1;
  int clear = radius + 1;
  if (d.R0 > 0) clear = min(clear, ci - d.R0 + 1);
  if (d.R1 < g.xsize - 1) clear = min(clear, d.R1 - ci + 1);
  if (C0 > 0) clear = min(clear, cj - C0 + 1);
  if (C1 < g.ysize - 1) clear = min(clear, C1 - cj + 1);
  return clear;
}
// What a lookup returns beside a code (>= 0) and -1 (a windowed lookup outside the refreshed window):
constexpr int kNeedSearch = -2;  // the 7 x 7 look ran and did not settle it: the answer needs the row walks (nearest_code_query_body)
constexpr int kNoLook = -3;      // the 7 x 7 look could not be made: no slice, no table, or its window sticks out of the slice
// A beam ends on or next to a wall: the 7 x 7 cells round the looked-up cell first.  Every cell outside them is >= 4 cells away,
// so a result <= 9 (and <= clear^2) is the map's answer.  Row by row: the seven bits round the column (one v_alignbit on two
// adjacent dwords of the LDS slice) index a 128-entry table of least column offsets.
__device__ __forceinline__ int look7(const GridC& g, const DistSrc& d, int radius, int ci, int cj) {
  if (d.nW == 0 || !d.lut7) return kNoLook;
  const int C0 = d.W0 * 64, C1 = (d.W0 + d.nW) * 64 - 1;
  const int p0 = cj - C0 - 3, wi = p0 >> 5;
  if (!(ci - 3 >= d.R0 && ci + 3 <= d.R1 && p0 >= 0 && wi + 1 < 2 * d.nW && cj <= C1)) return kNoLook;
  const int clear = tile_clear(g, d, radius, ci, cj);
  const unsigned int* t32 = reinterpret_cast<const unsigned int*>(d.tbm) + wi;
  const int sh = p0 & 31, stride = 2 * d.nW;
  int bw = 0x7fffffff;
#pragma unroll
  for (int dr = -3; dr <= 3; ++dr) {
    const unsigned int* rp = t32 + (ci + dr - d.R0) * stride;
    const unsigned int pat = __builtin_amdgcn_alignbit(rp[1], rp[0], sh) & 0x7Fu;
    bw = min(bw, dr * dr + (int)d.lut7[pat]);
  }
  if (bw <= 9 && bw <= clear * clear) return bw;
  return kNeedSearch;
}
// The whole search: the 7 x 7 look, then the row walks on the slice and on the global bitmap.  Inlined wherever it is used.  The
// scan matcher looks up ~100 poses x Bv cells per particle, many of them beyond the 7 x 7 look; the proposal kernel keeps only
// lookup_code_fast inside its lookup loops and runs this in a phase of its own (with both row walks at each of its lookups it was
// ~100 KB of code against a 64 KB instruction cache shared by two CUs).
__device__ __forceinline__ uint16_t nearest_code_query_body(const GridC& g, const DistSrc& d, int radius, int ci, int cj) {
  if (d.nW > 0) {
    // LDS slice first.  Its answer is the map's answer when no cell outside the slice can be nearer (tile_clear).
    const int C0 = d.W0 * 64, C1 = (d.W0 + d.nW) * 64 - 1;
    if (ci >= d.R0 && ci <= d.R1 && cj >= C0 && cj <= C1) {
      const int clear = tile_clear(g, d, radius, ci, cj);
      const int seen = look7(g, d, radius, ci, cj);
      if (seen >= 0) return (uint16_t)seen;
      if (seen == kNoLook) {
        // the same 7 rows, 64 columns each, by bit scans, branch-free
        const int cjr = cj - C0, s0 = cjr - 32, w = s0 >> 6, sh = s0 & 63;
        int bw = 0x7fffffff;
#pragma unroll
        for (int dr = -3; dr <= 3; ++dr) {
          const int r = ci + dr;
          if (r < d.R0 || r > d.R1) continue;
          const unsigned long long* row = d.tbm + (size_t)(r - d.R0) * d.nW;
          const unsigned long long lo64 = (w >= 0 && w < d.nW) ? row[w] : 0ull, hi64 = (w + 1 >= 0 && w + 1 < d.nW) ? row[w + 1] : 0ull;
          const unsigned long long W = sh ? ((lo64 >> sh) | (hi64 << (64 - sh))) : lo64;  // bit i = column s0 + i, the cell at bit 32
          const unsigned long long L = W & 0x1FFFFFFFFull, Rr = W >> 33;
          int f = 1 << 12;
          if (L) f = __clzll((long long)L) - 31;
          if (Rr) f = min(f, __ffsll((long long)Rr));
          bw = min(bw, dr * dr + f * f);
        }
        if (bw <= 9 && bw <= clear * clear) return (uint16_t)bw;
      }
      const int* any = d.tany;
      const int R0 = d.R0;
      const unsigned long long* tbm = d.tbm;
      const int nW = d.nW;
      const int best = nearest_d2_rows([tbm, nW, R0](int r, int w) { return tbm[(size_t)(r - R0) * nW + w]; }, d.nW, d.R0, d.R1, radius, ci, cj - C0,
                                       [any, R0](int r) { return any[r - R0] != 0; });
      if (best != 0x7fffffff && best <= clear * clear && best <= radius * radius) return (uint16_t)best;
      if (best == 0x7fffffff && clear > radius) return d.code ? d.code[(size_t)ci * g.xsize + cj] : kCodeUnreached;
    }
  }
  const OccT occ = d.occ;
  const int best = nearest_d2_rows([&occ](int r, int w) { return occ.word(r, w); }, g.words, 0, g.xsize - 1, radius, ci, cj,
                                   [&occ](int r) { return occ.row_any(r); });
  // nothing within cell_radius_: the stored code if the handle keeps a stored field (injected / materialised), else
  // "never reached" (the reference keeps whatever an earlier brushfire left there, grid_mapper.cpp:310-313)
  return (best <= radius * radius) ? (uint16_t)best : (d.code ? d.code[(size_t)ci * g.xsize + cj] : kCodeUnreached);
}
// Distance code of cell (ci, cj), or -1 when a windowed lookup falls outside the refreshed window.
__device__ __forceinline__ int lookup_code(const GridC& g, const DistSrc& d, int radius, int ci, int cj) {
  if (d.mode == 2) return nearest_code_query_body(g, d, radius, ci, cj);
  if (d.mode == 1 && (ci < d.win.x || ci > d.win.y || cj < d.win.z || cj > d.win.w)) return -1;
  return stored_code(g, d, ci, cj);
}
// The same without the row walks: in query mode the 7 x 7 look and nothing else, kNeedSearch when that does not give the code.
// The proposal kernel defers those lookups to a phase of their own — ONE inlined copy of the search per phase, run by all
// threads over the marked entries.
__device__ __forceinline__ int lookup_code_fast(const GridC& g, const DistSrc& d, int radius, int ci, int cj) {
  if (d.mode == 2) { const int seen = look7(g, d, radius, ci, cj); return seen >= 0 ? seen : kNeedSearch; }
  if (d.mode == 1 && (ci < d.win.x || ci > d.win.y || cj < d.win.z || cj > d.win.w)) return -1;
  return stored_code(g, d, ci, cj);
}

// ---- the LDS slice of the occupancy bitmap ----------------------------------------------------------------------------------
// Query mode: the bitmap rows / 64-cell word columns within occ_half cells of the sensor cell (sci, scj) — every lookup of the
// workgroup ends within range_max of it, and its nearest obstacle is usually a few cells further at most.  In LDS: the rows
// (nW words each), then any[r] per row.
struct Slice {
  int R0, R1, W0, nW;
  __device__ __forceinline__ int rows() const { return R1 - R0 + 1; }
  __device__ __forceinline__ int* any(unsigned long long* tbm) const { return reinterpret_cast<int*>(tbm + (size_t)rows() * nW); }
};
__device__ __forceinline__ Slice slice_round(const GridC& g, int occ_half, int sci, int scj) {
  const int W0 = max(0, scj - occ_half) >> 6, W1 = min(g.ysize - 1, scj + occ_half) >> 6;
  return Slice{max(0, sci - occ_half), min(g.xsize - 1, sci + occ_half), W0, W1 - W0 + 1};
}
// the plain copy, word by word through the particle's tile table: thread tid of nt takes rows tid, tid + nt, ...
__device__ __forceinline__ void slice_copy_rows(const OccT& occ, const Slice& s, unsigned long long* tbm, int tid, int nt) {
  int* ta = s.any(tbm);
  for (int r = tid; r < s.rows(); r += nt) {
    unsigned long long acc = 0ull;
    for (int w = 0; w < s.nW; ++w) {
      const unsigned long long v = occ.word(s.R0 + r, s.W0 + w);
      tbm[r * s.nW + w] = v;
      acc |= v;
    }
    ta[r] = acc != 0ull;
  }
}
// the 128-entry table of the 7 x 7 look, by the workgroup's first 128 threads
__device__ __forceinline__ void fill_lut7(unsigned char* lut7, int tid) {
  if (tid < 128) {
    int best = 100;
    for (int cbit = 0; cbit < 7; ++cbit) if ((tid >> cbit) & 1) { const int dc = cbit - 3; best = min(best, dc * dc); }
    lut7[tid] = (unsigned char)best;
  }
}
// d.tbm holds slice s (rows, then any[]) and lut7 the table — both visible to the lookups after the caller's next barrier
__device__ __forceinline__ void attach_slice(DistSrc& d, const Slice& s, unsigned long long* tbm, const unsigned char* lut7) {
  d.tany = s.any(tbm); d.R0 = s.R0; d.R1 = s.R1; d.W0 = s.W0; d.nW = s.nW; d.lut7 = lut7;
}

}  // namespace tbnav_rk
#endif

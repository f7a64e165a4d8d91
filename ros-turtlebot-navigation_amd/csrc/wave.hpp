// wave.hpp — every wave-wide reduction and scan of the tree (device code only; gfx950 wavefront = 64 lanes).  common.hpp
// includes it.  Two networks: __shfl_xor butterflies (ds_bpermute: six dependent LDS-latency steps per reduction, every lane
// gets the result) and the DPP network (row_shr / row_bcast; no LDS crossbar round trips, the result read from lane 63).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace tbnav {

// ---- butterflies on __shfl_xor ------------------------------------------------------------------------------------
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { const int o = __shfl_xor(v, off, 64); v = o < v ? o : v; }
  return v;
}
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(v, off, 64);
    v = o > v ? o : v;
  }
  return v;
}
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off, 64);
  return v;
}
__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// ---- wave64 scans on the DPP network (gfx9 row_shr / row_bcast; no LDS crossbar round trips) ---------
// update_dpp(old, src, ctrl, row_mask, bank_mask, bound_ctrl=false): a lane whose source is invalid or masked
// keeps `old`, which is the additive identity here.
template <int CTRL, int ROW_MASK, int BANK_MASK>
__device__ __forceinline__ double dpp_or_zero(double src) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(src), CTRL, ROW_MASK, BANK_MASK, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(src), CTRL, ROW_MASK, BANK_MASK, false);
  return __hiloint2double(hi, lo);
}
// The same for a stage whose row and bank masks are full: `old` can then only reach a lane whose source is out of the row or
// switched off, and bound_ctrl writes the same +0.0 there — no `v_mov_b32 v, 0` in front of each half (mov_dpp leaves `old`
// undefined, and nothing reads it).
template <int CTRL>
__device__ __forceinline__ double dpp_shift_or_zero(double src) {
  const int lo = __builtin_amdgcn_mov_dpp(__double2loint(src), CTRL, 0xf, 0xf, true);
  const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(src), CTRL, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}
// inclusive prefix sum over the lanes of a wave (lane i gets v_0 + ... + v_i); LEAN: the full-mask stages without a zeroed `old`
// (same bits; the kernels of the K = 1024 tick, where every issued VALU instruction counts)
template <bool LEAN = false>
__device__ __forceinline__ double wave_scan_incl(double v, int /*lane*/) {
  double out = v;
  out += LEAN ? dpp_shift_or_zero<0x111>(v) : dpp_or_zero<0x111, 0xf, 0xf>(v);  // row_shr:1
  out += LEAN ? dpp_shift_or_zero<0x112>(v) : dpp_or_zero<0x112, 0xf, 0xf>(v);  // row_shr:2
  out += LEAN ? dpp_shift_or_zero<0x113>(v) : dpp_or_zero<0x113, 0xf, 0xf>(v);  // row_shr:3   -> sums of up to four consecutive lanes
  out += dpp_or_zero<0x114, 0xf, 0xe>(out);  // row_shr:4, banks 1-3
  out += dpp_or_zero<0x118, 0xf, 0xc>(out);  // row_shr:8, banks 2-3 -> inclusive within each row of 16
  out += dpp_or_zero<0x142, 0xa, 0xf>(out);  // row_bcast:15 into rows 1 and 3
  out += dpp_or_zero<0x143, 0xc, 0xf>(out);  // row_bcast:31 into rows 2 and 3
  return out;
}
// whole-wave sum / min on the same network; the result is broadcast from lane 63
__device__ __forceinline__ double lane63(double v) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 63), __builtin_amdgcn_readlane(__double2loint(v), 63));
}
__device__ __forceinline__ double wave_sum_dpp(double v) { return lane63(wave_scan_incl(v, 0)); }
// N wave sums at once, for a wave that has its SIMD to itself (the time-step waves of mppi_combine's straight-line form): nothing
// else fills its issue slots, so every instruction issued is paid for (measured: about 4 cycles each, docs/lab_notebook.md, Round 23).
//  * Only the TOTAL is wanted, and it is read from lane 63.  Lane 63's sum is wave_scan_incl's, stage for stage:
//    ((x + shr1) + shr2) + shr3, then row_shr:4, row_shr:8, row_bcast:15, row_bcast:31 — the same bits as wave_sum_dpp.  What the
//    scan's row and bank masks do is keep `old` = 0 in lanes that must not receive.  For row_shr:4 / 8 those are exactly the lanes
//    whose source lies outside the row, where bound_ctrl writes the same +0.0.  For the two row_bcast they are rows that lane 63
//    never reads afterwards: row_bcast:15 reaches lane 63 from lane 47 and lane 31 from lane 15, row_bcast:31 lane 63 from lane 31.
//    So every stage is a full-mask move with bound_ctrl (dpp_shift_or_zero) and none has a `v_mov_b32 v, 0` in front of each half;
//    the lanes below 63 do NOT hold prefix sums.
//  * Stage s of every value, then stage s + 1: one sum's DPP moves stand between another's add and the moves that read it, where
//    six scans in a row had an `s_nop` for the DPP hazard in most stages.
// v[n] comes back as the total, broadcast.
template <int CTRL, int N>
__device__ __forceinline__ void wave_sums_stage(double (&out)[N], const double (&src)[N]) {
#pragma unroll
  for (int n = 0; n < N; ++n) out[n] += dpp_shift_or_zero<CTRL>(src[n]);
}
template <int N>
__device__ __forceinline__ void wave_sums_dpp(double (&v)[N]) {
  double out[N];
#pragma unroll
  for (int n = 0; n < N; ++n) out[n] = v[n];
  wave_sums_stage<0x111>(out, v);    // row_shr:1 .. 3 read the lane's own value
  wave_sums_stage<0x112>(out, v);
  wave_sums_stage<0x113>(out, v);
  wave_sums_stage<0x114>(out, out);  // row_shr:4
  wave_sums_stage<0x118>(out, out);  // row_shr:8: lane 15 of each row holds the row's sum
  wave_sums_stage<0x142>(out, out);  // row_bcast:15
  wave_sums_stage<0x143>(out, out);  // row_bcast:31
#pragma unroll
  for (int n = 0; n < N; ++n) v[n] = lane63(out[n]);
}
template <int CTRL, int ROW_MASK, int BANK_MASK>
__device__ __forceinline__ double dpp_or_inf(double src) {
  const double inf = __builtin_huge_val();
  const int lo = __builtin_amdgcn_update_dpp(__double2loint(inf), __double2loint(src), CTRL, ROW_MASK, BANK_MASK, false);
  const int hi = __builtin_amdgcn_update_dpp(__double2hiint(inf), __double2hiint(src), CTRL, ROW_MASK, BANK_MASK, false);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double wave_min_dpp(double v) {
  double out = v;
  out = fmin(out, dpp_or_inf<0x111, 0xf, 0xf>(v));
  out = fmin(out, dpp_or_inf<0x112, 0xf, 0xf>(v));
  out = fmin(out, dpp_or_inf<0x113, 0xf, 0xf>(v));
  out = fmin(out, dpp_or_inf<0x114, 0xf, 0xe>(out));
  out = fmin(out, dpp_or_inf<0x118, 0xf, 0xc>(out));
  out = fmin(out, dpp_or_inf<0x142, 0xa, 0xf>(out));
  out = fmin(out, dpp_or_inf<0x143, 0xc, 0xf>(out));
  return lane63(out);
}
// The partner of a butterfly step inside groups of 2 / 4 / 8 / 16 consecutive lanes, on the DPP network: lane ^ 1 and
// lane ^ 2 are quad permutations; once a quad's lanes agree, the mirror image within 8 (row_half_mirror) or 16
// (row_mirror) lanes lies in the other quad / half, which is all a commutative reduction needs.  Every lane has a source inside
// its group and the masks are full, so `old` is never read and stays undefined (mov_dpp) — the lanes of a group must be
// switched on or off together, as they are in the one caller of group_reduce_dpp, mppi_rollout_fused's record loop (a group
// shares its time step).  Changed in place for that reason: no other kernel's code contains it.
template <int STEP>
__device__ __forceinline__ double dpp_group_partner(double v) {
  constexpr int ctrl = STEP == 1 ? 0xB1 : STEP == 2 ? 0x4E : STEP == 4 ? 0x141 : 0x140;  // quad_perm [1,0,3,2] / [2,3,0,1], row_half_mirror, row_mirror
  const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), ctrl, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), ctrl, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}
// all-lanes reduction over groups of R consecutive lanes (R = 2, 4, 8, 16), steps in the order 1, 2, 4, 8
template <int R, class Op>
__device__ __forceinline__ double group_reduce_dpp(double v, Op op) {
  static_assert(R == 2 || R == 4 || R == 8 || R == 16, "groups of 2..16 lanes");
  v = op(v, dpp_group_partner<1>(v));
  if constexpr (R >= 4) v = op(v, dpp_group_partner<2>(v));
  if constexpr (R >= 8) v = op(v, dpp_group_partner<4>(v));
  if constexpr (R >= 16) v = op(v, dpp_group_partner<8>(v));
  return v;
}
// inclusive suffix sum (lane i gets v_i + ... + v_63): mirror the wave, scan, mirror back
__device__ __forceinline__ double readlane_d(double v, int l) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}
__device__ __forceinline__ double wave_scan_incl_rev(double v, int lane) {
  // the mirror image of wave_scan_incl inside each row of 16 lanes (row_shl), then the totals of the later rows — read
  // from their first lanes — are added; no LDS permute (two dependent ones before)
  // (mppi_rollout_fused is the only caller, so the full-mask stages took the bound_ctrl form in place)
  double out = v;
  out += dpp_shift_or_zero<0x101>(v);        // row_shl:1
  out += dpp_shift_or_zero<0x102>(v);        // row_shl:2
  out += dpp_shift_or_zero<0x103>(v);        // row_shl:3
  out += dpp_or_zero<0x104, 0xf, 0x7>(out);  // row_shl:4, banks 0-2
  out += dpp_or_zero<0x108, 0xf, 0x3>(out);  // row_shl:8, banks 0-1 -> inclusive suffix within each row of 16
  const double t1 = readlane_d(out, 16), t2 = readlane_d(out, 32), t3 = readlane_d(out, 48);
  const int row = lane >> 4;
  const double later = row == 0 ? (t1 + t2) + t3 : row == 1 ? t2 + t3 : row == 2 ? t3 : 0.0;
  return out + later;
}

// ---- whole-wave reductions with an identity and an operation, on the DPP network: an inclusive scan inside each row of 16
// lanes by DPP shifts, then the row totals carried down the rows (row_bcast:15 / :31); lane 63 holds the result, which is
// handed to every lane.  A fixed order of operations, the same on every call (the proposal kernel's sums and products are
// compared with the oracle at 1e-9, not bit for bit). ----
#define TBNAV_DPP_D(v, ident, ctrl, rmask)                                                                                      \
  __hiloint2double(__builtin_amdgcn_update_dpp(__double2hiint(ident), __double2hiint(v), ctrl, rmask, 0xf, false),              \
                   __builtin_amdgcn_update_dpp(__double2loint(ident), __double2loint(v), ctrl, rmask, 0xf, false))
template <class Op> __device__ __forceinline__ double wave_reduce_dpp_d(double v, double ident, Op op) {
  v = op(v, TBNAV_DPP_D(v, ident, 0x111, 0xf));  // row_shr:1
  v = op(v, TBNAV_DPP_D(v, ident, 0x112, 0xf));  // row_shr:2
  v = op(v, TBNAV_DPP_D(v, ident, 0x114, 0xf));  // row_shr:4
  v = op(v, TBNAV_DPP_D(v, ident, 0x118, 0xf));  // row_shr:8
  v = op(v, TBNAV_DPP_D(v, ident, 0x142, 0xa));  // row_bcast:15 into rows 1, 3
  v = op(v, TBNAV_DPP_D(v, ident, 0x143, 0xc));  // row_bcast:31 into rows 2, 3
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 63), __builtin_amdgcn_readlane(__double2loint(v), 63));
}
__device__ __forceinline__ double wave_max_d(double v) { return wave_reduce_dpp_d(v, -1.0e300, [](double a, double b) { return fmax(a, b); }); }
__device__ __forceinline__ double wave_sum_d(double v) { return wave_reduce_dpp_d(v, 0.0, [](double a, double b) { return a + b; }); }
__device__ __forceinline__ double wave_prod(double v) { return wave_reduce_dpp_d(v, 1.0, [](double a, double b) { return a * b; }); }
// the same for int
template <class Op> __device__ __forceinline__ int wave_reduce_dpp(int v, int ident, Op op) {
  v = op(v, __builtin_amdgcn_update_dpp(ident, v, 0x111, 0xf, 0xf, false));  // row_shr:1
  v = op(v, __builtin_amdgcn_update_dpp(ident, v, 0x112, 0xf, 0xf, false));  // row_shr:2
  v = op(v, __builtin_amdgcn_update_dpp(ident, v, 0x114, 0xf, 0xf, false));  // row_shr:4
  v = op(v, __builtin_amdgcn_update_dpp(ident, v, 0x118, 0xf, 0xf, false));  // row_shr:8
  v = op(v, __builtin_amdgcn_update_dpp(ident, v, 0x142, 0xa, 0xf, false));  // row_bcast:15 into rows 1, 3
  v = op(v, __builtin_amdgcn_update_dpp(ident, v, 0x143, 0xc, 0xf, false));  // row_bcast:31 into rows 2, 3
  return __builtin_amdgcn_readlane(v, 63);
}
__device__ __forceinline__ int wave_min_dpp(int v) { return wave_reduce_dpp(v, 0x7FFFFFFF, [](int a, int b) { return a < b ? a : b; }); }
__device__ __forceinline__ int wave_max_dpp(int v) { return wave_reduce_dpp(v, (int)0x80000000, [](int a, int b) { return a > b ? a : b; }); }
__device__ __forceinline__ int wave_sum_dpp(int v) { return wave_reduce_dpp(v, 0, [](int a, int b) { return a + b; }); }

}  // namespace tbnav

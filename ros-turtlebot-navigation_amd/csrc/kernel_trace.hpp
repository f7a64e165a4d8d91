// kernel_trace.hpp — the development tracer of a -DTBNAV_PHASE_PROF build, once for every kernel that carries it (rbpf_raycast_box,
// rbpf_propose): wall-clock stamps per wave of two chosen workgroups, every workgroup's entry / exit / CU of the LAST launch, and —
// without -DTBNAV_TRACE_ONLY — per-phase times summed over workgroups behind extra barriers.  The stamps add global stores (the phase
// sums: barriers and contended atomics) — the kernels run measurably slower with them; the numbers are for comparing phases, not for
// the bench.  Without -DTBNAV_PHASE_PROF every macro below expands to nothing.
//   TBNAV_TRACE_ARRAYS(name, WAVES, WG_A, WG_B)   at namespace scope of the kernel's file: the arrays of kernel `name`, WAVES waves
//                                                 stamped in the workgroups blockIdx.x == WG_A and WG_B
//   TRACE(name, i)                                in the kernel: stamp i (< 16) of this wave, if its workgroup is one of the two
//   WG_IN(name) / WG_OUT(name)                    in the kernel: this workgroup's entry (with XCC and CU) / exit
//   TBNAV_TRACE_PRINT(name, kernel, STAMPS, legend)   on the host, in the same file (hipMemcpyFromSymbol needs the symbol's
//                                                 translation unit): copies the arrays and has trace_print print them
//   TBNAV_PHASE_SUMS(name), PHASE_START(), PHASE_STAMP(name, i), PHASE_DONE(name), TBNAV_PHASE_SUMS_READ(name, pw): the phase sums
#pragma once
#include <hip/hip_runtime.h>

#ifndef TBNAV_PHASE_PROF
#define TBNAV_TRACE_ARRAYS(name, WAVES, WG_A, WG_B)
#define TRACE(name, i)
#define WG_IN(name)
#define WG_OUT(name)
#define TBNAV_PHASE_SUMS(name)
#define PHASE_START()
#define PHASE_STAMP(name, i)
#define PHASE_DONE(name)
#else
#include <algorithm>
#include <cstdio>
#include <map>
#include <vector>

namespace tbnav {
constexpr int kTraceStamps = 16, kTraceWgs = 4096;
}
#define TBNAV_TRACE_ARRAYS(name, WAVES, WG_A, WG_B)                                                                                   \
  constexpr int kTraceWaves_##name = WAVES, kTraceWgA_##name = WG_A, kTraceWgB_##name = WG_B;                                         \
  static __device__ unsigned long long g_trace_##name[2][WAVES][::tbnav::kTraceStamps];  /* [which][wave][stamp], 10 ns ticks */       \
  static __device__ unsigned long long g_wg_##name[::tbnav::kTraceWgs][3];   /* [workgroup] entry, exit, XCC_ID << 32 | HW_ID */
#define TRACE(name, i) do { if ((blockIdx.x == kTraceWgA_##name || blockIdx.x == kTraceWgB_##name) && (threadIdx.x & 63) == 0 && (threadIdx.x >> 6) < kTraceWaves_##name) \
  g_trace_##name[blockIdx.x == kTraceWgB_##name][threadIdx.x >> 6][i] = wall_clock64(); } while (0)
#define WG_IN(name) do { if (threadIdx.x == 0 && blockIdx.x < ::tbnav::kTraceWgs) { g_wg_##name[blockIdx.x][0] = wall_clock64(); \
  g_wg_##name[blockIdx.x][2] = ((unsigned long long)__builtin_amdgcn_s_getreg(63508) << 32) | (unsigned int)__builtin_amdgcn_s_getreg(63492); } } while (0)
#define WG_OUT(name) do { if (threadIdx.x == 0 && blockIdx.x < ::tbnav::kTraceWgs) g_wg_##name[blockIdx.x][1] = wall_clock64(); } while (0)
#define TBNAV_TRACE_PRINT(name, kernel, STAMPS, legend) do {                                                                          \
    static unsigned long long tr_[2][kTraceWaves_##name][::tbnav::kTraceStamps], wg_[::tbnav::kTraceWgs][3];                          \
    const bool has_tr_ = hipMemcpyFromSymbol(tr_, HIP_SYMBOL(g_trace_##name), sizeof(tr_)) == hipSuccess;                             \
    const bool has_wg_ = hipMemcpyFromSymbol(wg_, HIP_SYMBOL(g_wg_##name), sizeof(wg_)) == hipSuccess;                                \
    const int ids_[2] = {kTraceWgA_##name, kTraceWgB_##name};                                                                         \
    ::tbnav::trace_print(kernel, legend, has_tr_ ? &tr_[0][0][0] : nullptr, kTraceWaves_##name, STAMPS, ids_, has_wg_ ? wg_ : nullptr); \
  } while (0)

// the phase sums: [i] 10 ns ticks of phase i summed over workgroups, [15] the workgroups counted
#define TBNAV_PHASE_SUMS(name) static __device__ unsigned long long g_phase_##name[16];
#define TBNAV_PHASE_SUMS_READ(name, pw) (hipMemcpyFromSymbol(pw, HIP_SYMBOL(g_phase_##name), sizeof(unsigned long long) * 16) == hipSuccess && pw[15])
#ifdef TBNAV_TRACE_ONLY  // (the sums are contended atomics on ONE address: they distort the very timeline TRACE_ONLY records)
#define PHASE_START()
#define PHASE_STAMP(name, i)
#define PHASE_DONE(name)
#else
#define PHASE_START() unsigned long long t_prev_ = wall_clock64()
#define PHASE_STAMP(name, i) do { __syncthreads(); if (threadIdx.x == 0) { const unsigned long long now_ = wall_clock64(); atomicAdd(&g_phase_##name[i], now_ - t_prev_); t_prev_ = now_; } } while (0)
#define PHASE_DONE(name) do { if (threadIdx.x == 0) atomicAdd(&g_phase_##name[15], 1ull); } while (0)
#endif

namespace tbnav {

// trace: [2][waves][kTraceStamps] or null; wg: [kTraceWgs][3] or null.  Prints the two traced workgroups' wave timelines under the
// kernel's column legend, then of all recorded workgroups: residents over time, entries and mean residence by time of entry, and the
// figures per CU and per XCC.
inline void trace_print(const char* kernel, const char* legend, const unsigned long long* trace, int waves, int stamps, const int wg_id[2],
                        const unsigned long long (*wg)[3]) {
  if (trace && trace[0]) {
    for (int g = 0; g < 2; ++g) {
      const unsigned long long* tr = trace + (size_t)g * waves * kTraceStamps;
      std::fprintf(stderr, "[%s trace of workgroup %d, us since its first stamp; columns: %s]\n", kernel, wg_id[g], legend);
      unsigned long long t0 = ~0ull;
      for (int w = 0; w < waves; ++w) if (tr[w * kTraceStamps] && tr[w * kTraceStamps] < t0) t0 = tr[w * kTraceStamps];
      for (int w = 0; w < waves; ++w) {
        std::fprintf(stderr, "  wave %2d:", w);
        // (0: never stamped, printed as -1; a stamp only some launches make can be an earlier launch's: far below zero)
        for (int i = 0; i < stamps; ++i) std::fprintf(stderr, " %6.2f", tr[w * kTraceStamps + i] ? (double)(long long)(tr[w * kTraceStamps + i] - t0) * 0.01 : -1.0);
        std::fprintf(stderr, "\n");
      }
    }
  }
  if (!wg || !wg[1][0]) return;
  int n = 0;
  unsigned long long t0 = ~0ull, t1 = 0;
  for (int i = 0; i < kTraceWgs; ++i) if (wg[i][0] && wg[i][1]) { ++n; t0 = std::min(t0, wg[i][0]); t1 = std::max(t1, wg[i][1]); }
  if (!n) return;
  std::fprintf(stderr, "[%s workgroups of the last launch] %d recorded, first entry to last exit %.2f us\n", kernel, n, (double)(t1 - t0) * 0.01);
  constexpr int nb = 16;
  const double span = (double)(t1 - t0);
  int active[nb] = {0}, starts[nb] = {0};
  double dur_by_start[nb] = {0};
  // by XCC and by CU: is a slow workgroup's CU slow as a whole?
  std::map<unsigned long long, std::vector<double>> by_cu;   // key: XCC, then cu_id [11:8], sh_id [12], se_id [15:13] of HW_ID
  double xs[16] = {0}; int xn[16] = {0};
  for (int i = 0; i < kTraceWgs; ++i) if (wg[i][0] && wg[i][1]) {
    const double d = (double)(wg[i][1] - wg[i][0]) * 0.01;
    const int bs = std::min(nb - 1, (int)((double)(wg[i][0] - t0) / span * nb));
    ++starts[bs]; dur_by_start[bs] += d;
    for (int b = 0; b < nb; ++b) { const double tm = t0 + (b + 0.5) * span / nb; if ((double)wg[i][0] <= tm && tm < (double)wg[i][1]) ++active[b]; }
    const unsigned int hw = (unsigned int)wg[i][2], xcc = (unsigned int)(wg[i][2] >> 32) & 0xF;
    by_cu[((unsigned long long)xcc << 16) | (hw & 0xFF00u)].push_back(d);
    xs[xcc] += d; ++xn[xcc];
  }
  std::fprintf(stderr, "  time bin (%.2f us each):", span * 0.01 / nb);
  for (int b = 0; b < nb; ++b) std::fprintf(stderr, " %5d", b);
  std::fprintf(stderr, "\n  resident at mid-bin:    ");
  for (int b = 0; b < nb; ++b) std::fprintf(stderr, " %5d", active[b]);
  std::fprintf(stderr, "\n  entered in bin:         ");
  for (int b = 0; b < nb; ++b) std::fprintf(stderr, " %5d", starts[b]);
  std::fprintf(stderr, "\n  mean residence (us):    ");
  for (int b = 0; b < nb; ++b) std::fprintf(stderr, " %5.1f", starts[b] ? dur_by_start[b] / starts[b] : 0.0);
  int hist[16] = {0};
  double spread_in = 0.0, cu_min = 1e9, cu_max = 0, d3 = 0, d4 = 0;
  int n3 = 0, n4 = 0;
  for (auto& kv : by_cu) {
    ++hist[std::min<size_t>(15, kv.second.size())];
    double lo = 1e9, hi = 0, sum = 0;
    for (double d : kv.second) { lo = std::min(lo, d); hi = std::max(hi, d); sum += d; }
    spread_in += hi - lo;
    const double mean = sum / kv.second.size();
    cu_min = std::min(cu_min, mean); cu_max = std::max(cu_max, mean);
    if (kv.second.size() <= 3) { ++n3; d3 += mean; } else { ++n4; d4 += mean; }
  }
  std::fprintf(stderr, "\n  CUs that ran workgroups: %zu; CUs by number of workgroups run:", by_cu.size());
  for (int k = 1; k < 16; ++k) if (hist[k]) std::fprintf(stderr, " %d:%d", k, hist[k]);
  std::fprintf(stderr, "\n  workgroups per XCC:");
  for (int x = 0; x < 16; ++x) if (xn[x]) std::fprintf(stderr, " %d", xn[x]);
  std::fprintf(stderr, "\n  mean residence by XCC (us):");
  for (int x = 0; x < 16; ++x) if (xn[x]) std::fprintf(stderr, " %.1f", xs[x] / xn[x]);
  std::fprintf(stderr, "\n  mean (max - min) inside a CU %.1f us; CU means from %.1f to %.1f us; CUs with <= 3 workgroups: %d, mean %.1f us; with 4+: %d, mean %.1f us\n",
               spread_in / std::max<size_t>(1, by_cu.size()), cu_min, cu_max, n3, n3 ? d3 / n3 : 0.0, n4, n4 ? d4 / n4 : 0.0);
}

}  // namespace tbnav
#endif

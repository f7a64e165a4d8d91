// icp_device.hpp — what the device ICP (icp.hip) and the correlative search in front of it (icp_search.hip) share: the handle,
// the by-value kernel constants, the cloud of contract item 1 (cloud_point with the beam table) and the device buffers (DevBuf: grow, discard the contents).
#pragma once
#include <hip/hip_runtime.h>

#include <array>
#include <cstdint>
#include <vector>

#include "common.hpp"
#include "tbnav_icp.h"

namespace tbnav_icpdev {

constexpr int kThreads = 256;   // B of the header's reduction order
constexpr int kWave = 64;

struct IcpConst {
  float range_min, range_max;
  double trs_c, trs_s, trs_x, trs_y;   // Trs as Transform2D holds it
  double max_corr2;                    // max_corr_dist^2
  double rot_thresh, trans_thresh;     // 1 - transform_eps, transform_eps
  double fitness_eps;
  int max_iter;
};

// the line metric's parameters (tbnav_icp_set_metric)
struct IcpLine {
  double gap2;       // normal_max_gap^2
  double min_cond;   // TBNAV_ICP_LINE_MIN_COND
  int window;        // normal_window
};

// one alignment: scan indices (-1: the handle's stored scan) and the float-rounded initial guess
struct IcpPair {
  int32_t tgt, src;
  double c, s, x, y;
};

struct IcpOut {
  double R00, R10, tx, ty, mse;
  int32_t iterations, correspondences, criterion, pad;
};

__device__ __forceinline__ bool cloud_point(float r, float2 cs, const IcpConst& k, float2& p) {
  if (!(r >= k.range_min && r < k.range_max)) return false;
  const double px = (double)r * (double)cs.x, py = (double)r * (double)cs.y;
  p.x = (float)(((k.trs_c * px) - (k.trs_s * py)) + k.trs_x);
  p.y = (float)(((k.trs_s * px) + (k.trs_c * py)) + k.trs_y);
  return true;
}

using tbnav::DeviceGuard;

// a device buffer that only grows and forgets its contents when it does: every user writes it before reading it
struct DevBuf {
  void* ptr = nullptr;
  size_t cap = 0;   // bytes
  // at least `bytes` bytes; on failure the buffer is left empty
  int reserve(size_t bytes) {
    if (bytes <= cap) return TBNAV_OK;
    if (ptr) TBNAV_HIP(hipFree(ptr));
    ptr = nullptr; cap = 0;
    void* p = nullptr;
    TBNAV_HIP(hipMalloc(&p, bytes));
    ptr = p;
    cap = bytes;
    return TBNAV_OK;
  }
  void release() {
    (void)hipFree(ptr);
    ptr = nullptr; cap = 0;
  }
  template <class T>
  T* as() const { return static_cast<T*>(ptr); }
};

// the correlative search's state in the handle (tbnav_icp.h, CORRELATIVE SEARCH); the buffers are icp_search.hip's
struct IcpSearch {
  bool on = false;
  tbnav_icp_search_params p{};      // the defaults while the search is off
  tbnav_icp_search_info last{};     // tbnav_icp_last_search
  bool shape_on = false;            // tbnav_icp_set_search_shape (F1-F6): idle while the search itself is off
  tbnav_icp_search_shape_params shape_p{};   // the defaults while the shape is off
  tbnav_icp_search_shape last_shape{};       // tbnav_icp_last_search_shape
  bool wide_on = false;             // tbnav_icp_set_search_wide (W1-W8): idle while the search itself is off
  tbnav_icp_search_wide_params wide_p{};     // the defaults while the wide stage is off
  tbnav_icp_search_wide_info last_wide{};    // tbnav_icp_last_search_wide
  tbnav_icp_search_params stamp_of{};  // the parameters d_stamp was built from
  bool have_stamp = false;
  uint8_t* d_stamp = nullptr;       // [(2k+1)^2]
  DevBuf d_tables;                  // uint8_t [chunk][padded table]
  DevBuf d_in;                      // per chunk: the pairs, then their rotations
  DevBuf d_rec;                     // SearchRec [chunk][na] partial results
  DevBuf d_sel;                     // SearchSel [chunk] results
  DevBuf d_tgt_points;              // uint32_t [chunk]: the valid target points
  DevBuf d_scores;                  // uint32_t: the test hook's score volume
  DevBuf d_shape;                   // ShapeRec [chunk]: the integers of F3 (icp_search_shape.hip)
  DevBuf d_win;                     // the wide stage (icp_search_wide.hip): the escalated pairs' places, then their rotations
  DevBuf d_wrec;                    // WideRec [pairs of a launch][na][tiles] partial results
  DevBuf d_wsel;                    // SearchSel [escalated pairs] results
  DevBuf d_wshape;                  // ShapeRec [escalated pairs][tiles]: F3's integers per tile
  DevBuf d_wscores;                 // uint32_t: the wide test hook's score volume
  DevBuf d_map_in;                  // the map search (icp_search_map.hip): the value-by-d2 table, then the chunk's MapPairs
  hipEvent_t map_ev = nullptr;      // ... "the filter's stream has come this far", created at the first map search
  bool map_ran = false;             // ... tbnav_icp_last_map_kernel
  std::vector<unsigned char> h_in, h_sel, h_shape, h_win, h_wsel, h_wshape, h_map;
};

// the global search's state in the handle (tbnav_icp.h, GLOBAL SEARCH; icp_global.hip owns the buffers, grown on demand)
struct IcpGlobal {
  tbnav_icp_global_info last{};     // tbnav_icp_last_global
  const char* kernels = "";         // tbnav_icp_last_global_kernels
  DevBuf d_lik, d_pool;             // uint8_t [P][P]: L2's map and L5's pooled copy, zero margin included
  DevBuf d_in;                      // per call: the value-by-d2 table, then the headings' (cos, sin)
  DevBuf d_scan;                    // float [n_beams]
  DevBuf d_off;                     // uint32_t [NA][n_beams]: L3's offsets per heading, packed, compacted in no order
  DevBuf d_cnt;                     // uint32_t [NA]: how many each heading holds
  DevBuf d_bounds;                  // uint32_t [blocks]
  DevBuf d_list;                    // uint32_t: the blocks of a round
  DevBuf d_scores;                  // uint32_t: the test hook's score volume
  DevBuf d_rec;                     // GlobalRec, then the seeding histogram
  std::vector<unsigned char> h_in;
};

// the hypotheses' state in the handle (tbnav_icp.h, HYPOTHESES; icp_global.hip owns the buffers, grown on demand, icp_hyp.hip fills them)
struct IcpHyp {
  tbnav_icp_hyp_info last{};        // tbnav_icp_last_hyp
  const char* kernels = "";         // tbnav_icp_last_hyp_kernels
  DevBuf d_cands;                   // uint64 [cand_cap]: the keys of the candidates with score >= t, in no order
  DevBuf d_flags;                   // uint8 [cand_cap]: 1 where the candidate is a peak
  DevBuf d_peaks;                   // uint64 [cand_cap]: the peaks' keys, compacted
  DevBuf d_bins;                    // uint64 [bins]: each bin's greatest key
  DevBuf d_alive;                   // uint8 [bins]: 0 where the bin's winner was knocked
  DevBuf d_rec;                     // HypRec
};

}  // namespace tbnav_icpdev

struct tbnav_icp {
  tbnav_icp_params p{};
  tbnav_icpdev::IcpConst k{};
  int device = 0;
  hipStream_t stream = nullptr;
  int table_beams = 0;                 // beam count the device table was built for
  float2* d_table = nullptr;           // cosf / sinf per beam [table_beams]
  tbnav_icpdev::DevBuf d_stored;       // float [stored_beams]: the stored scan (pclICPWrapper's old_scan)
  int stored_beams = 0;
  bool have_stored = false;
  tbnav_icpdev::DevBuf d_scans;        // float: batch scans / match inputs
  tbnav_icpdev::DevBuf d_pairs, d_out; // IcpPair / IcpOut per alignment
  int last_launches = 0;
  int metric = TBNAV_ICP_METRIC_POINT;  // tbnav_icp_set_metric
  tbnav_icpdev::IcpLine line{TBNAV_ICP_LINE_NORMAL_MAX_GAP * TBNAV_ICP_LINE_NORMAL_MAX_GAP, TBNAV_ICP_LINE_MIN_COND,
                             TBNAV_ICP_LINE_NORMAL_WINDOW};
  double line_gap = TBNAV_ICP_LINE_NORMAL_MAX_GAP;
  std::vector<tbnav_icpdev::IcpPair> h_pairs;
  std::vector<tbnav_icpdev::IcpOut> h_out;
  tbnav_icpdev::IcpSearch search;
  tbnav_icpdev::IcpGlobal global;
  tbnav_icpdev::IcpHyp hyp;
  tbnav_icpdev::DevBuf d_align_in, d_align_rec;     // the map alignment (icp_align_map.hip): its pairs; the test hook's pairing record
  int align_map_p = 0;                              // ... the P of its last launch, 0: none yet (tbnav_icp_last_align_map_kernel)
  tbnav_icpdev::DevBuf d_verify_in, d_verify_out, d_verify_rec;   // the map check (icp_verify_map.hip): its pairs, their records; the test hook's per-beam record
  int verify_map_p = 0;                             // ... the P of its last launch, 0: none yet (tbnav_icp_last_verify_map_kernel)
  std::vector<std::array<double, 3>> h_init;       // T_init of h_pairs, as given (the search starts from the doubles)
  std::vector<tbnav_icp_search_info> h_sinfo;       // the search record of h_pairs (run_pairs)
  std::vector<tbnav_icp_search_shape> h_sshape;     // and the shape record beside it (computed = 0 where the shape did not run)
  std::vector<tbnav_icp_search_wide_info> h_swide;  // and the wide stage's (W5: the first stage's record, and whether the wide stage ran)
};

namespace tbnav_icpdev {

struct MapSource;   // icp_search_device.hpp

// icp.hip
int ensure_table(tbnav_icp* h, int n_beams);

// icp_search.hip: the search of h->h_pairs[0, n_pairs) from h->h_init (scans already in d_scans / d_stored, the beam table
// built) with parameters sp -> h->h_sinfo[0, n_pairs).  scores (n_pairs == 1 only): the whole score volume, or null.
// shp: the shape of the score volume (F1-F6) behind the selection -> h->h_sshape and the shaped T in h->h_sinfo, or null.
// map: the tables come from a filter particle's occupancy bits (MAP SEARCH, M1-M9; icp_search_device.hpp) instead of target scans.
// wp: the wide second stage (W1-W8) for the pairs W3 names -> h->h_sinfo holds the OUTCOME (W5) and h->h_swide the first
// stage's record, or null; wide_scores (n_pairs == 1 only): the wide stage's score volume, or null.
int search_pairs(tbnav_icp* h, int n_pairs, int n_beams, const tbnav_icp_search_params& sp, uint32_t* scores,
                 const tbnav_icp_search_shape_params* shp, const tbnav_icp_search_wide_params* wp = nullptr,
                 uint32_t* wide_scores = nullptr, const MapSource* map = nullptr);
void search_free(tbnav_icp* h);
// icp_global.hip
void global_free(tbnav_icp* h);

}  // namespace tbnav_icpdev

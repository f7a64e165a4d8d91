// rbpf.hip — bmapping::ParticleFilter::SLAM on MI355X (gfx950) behind the C-ABI of include/tbnav_rbpf.h: the launch sequence of
// one scan, create / destroy and tbnav_rbpf_slam.  The handle itself and the other host files (batch pipeline, sharded scan, blobs,
// queries / options, reference-field plumbing): rbpf_host.hpp.  Reference (paths relative to the reference tree):
//   bmapping/src/bmapping/particle_filter.cpp:141-251 (SLAM), :295-322, :383-437, :442-500, :504-599
//   bmapping/src/bmapping/grid_mapper.cpp:69-182 (likelihood field, integrateScan), :549-898
//   bmapping/src/bmapping/sensor_model.cpp:43-112 (laserEndPoints)
// The kernels live in their families' files (all -ffp-contract=off; DESIGN.md section 4 has the reasoning and the numbers):
//   rbpf_propose.hip   rbpf_mix_lut, rbpf_sample_normals, rbpf_likelihood_one, rbpf_field_by_query, rbpf_scanmatch, rbpf_propose
//   rbpf_raycast.hip   rbpf_raycast_box<512 / 1024> (default map update), rbpf_raycast (beam-ordered), rbpf_add_repeated_test
//   rbpf_field.hip     rbpf_densify, rbpf_window, rbpf_edt<C>, rbpf_edt_compact<R> (stored-field modes, on-demand fields)
//   rbpf_resample.hip  rbpf_normalize, rbpf_resample_apply, rbpf_pool_init, dense <-> tiles, rbpf_argmax, rbpf_export_map
//   rbpf_migrate.hip   particle blobs for the sharded filter's cross-rank resample
//   rbpf_device.hpp    what they share: launch-argument structs, map accessors, reductions, kernel declarations, the lists of forms
//   rbpf_plan.hpp      which form a scan gets and with how much LDS: the selection, as plain host arithmetic (no HIP, testable on a CPU)
//   rbpf_normalize.hpp the normalise / selection body (a kernel of its own and workgroup 0 of the map update)
#include "rbpf_host.hpp"

namespace tbnav_rh {

StatePtrs state_ptrs(double* base, int N) { return {base, base + (size_t)3 * N, base + (size_t)6 * N}; }
MapT map_of(const tbnav_rbpf* h) { return MapT{h->d_table[h->cur], h->d_shed, h->TW, h->TT}; }

// The stored u16 distance field exists only once something needs it: 2 * N * G * 2 bytes (double-buffered like the
// rest of the particle state).  Refused beyond 32 GB — BASELINE configs[4]-sized handles run in query mode only.
int ensure_codes(tbnav_rbpf* h) {
  if (h->d_code[0]) return TBNAV_OK;
  const size_t bytes = sizeof(uint16_t) * h->G * (size_t)h->N;
  if (2 * bytes > ((size_t)32 << 30) || h->N > 65535) return TBNAV_ERR_UNSUPPORTED;
  for (int b = 0; b < 2; ++b) {
    TBNAV_HIP(hipMalloc((void**)&h->d_code[b], bytes));
    TBNAV_HIP(hipMemset(h->d_code[b], 0xFF, bytes));  // occ_dist = max_occ_dist_ (grid_mapper.cpp:49,58)
  }
  TBNAV_HIP(hipMalloc((void**)&h->d_bm_dense, sizeof(unsigned long long) * (size_t)h->N * h->xsize * h->words));
  TBNAV_HIP(hipMalloc((void**)&h->d_rc_dense, sizeof(int) * (size_t)h->N * h->xsize));
  return TBNAV_OK;
}

double logodds_to_prob(double l) { return 1 - (1 / (1 + std::exp(l))); }  // grid_mapper.hpp:27-30 (glibc on the host)

// smallest l with prob(l) >= p_occ, found by bisection on the host (prob is monotone in l)
double find_occ_cut(double l_occ_nominal, double p_occ) {
  double lo = l_occ_nominal - 1.0, hi = l_occ_nominal + 1.0;  // prob(lo) < p_occ <= prob(hi)
  for (int it = 0; it < 200; ++it) {
    const double mid = 0.5 * (lo + hi);
    if (mid == lo || mid == hi) break;
    if (logodds_to_prob(mid) >= p_occ) hi = mid; else lo = mid;
  }
  return hi;
}

// Break points of the exported map value as a function of the log-odds, found with the HOST libm by bisection
// (the exported value is monotone in l apart from the prob == 0.5 plateau, which maps to -1).
int export_value_host(double l) {  // GridMapper::gridMap after updateCellState, evaluated as the reference does
  const double prob = logodds_to_prob(l);
  if (prob == 0.5) return -1;
  if (prob >= 0.90) return 100;
  if (prob <= 0.35) return 0;
  return (int)(int8_t)(prob * 100);
}
double bisect_first(double lo, double hi, bool (*pred)(double, int), int arg) {  // pred(lo) false, pred(hi) true, monotone
  for (int it = 0; it < 300; ++it) {
    const double mid = 0.5 * (lo + hi);
    if (mid == lo || mid == hi) break;
    if (pred(mid, arg)) hi = mid; else lo = mid;
  }
  return hi;
}
ExportCuts derive_export_cuts(double cut_occ) {
  ExportCuts c{};
  c.occ_cut = cut_occ;
  // largest l with prob <= 0.35: the predecessor of the first l with prob > 0.35
  const double first_above = bisect_first(-3.0, 0.0, [](double l, int) { return logodds_to_prob(l) > 0.35; }, 0);
  c.free_cut = std::nextafter(first_above, -1.0e9);
  c.half_lo = bisect_first(-1.0, 1.0, [](double l, int) { return logodds_to_prob(l) >= 0.5; }, 0);
  const double first_gt = bisect_first(-1.0, 1.0, [](double l, int) { return logodds_to_prob(l) > 0.5; }, 0);
  c.half_hi = std::nextafter(first_gt, -1.0e9);
  c.n_steps = 0;
  for (int k = 36; k <= 89; ++k)  // smallest l (outside the 0.5 plateau) whose exported value is >= k
    c.step[c.n_steps++] = bisect_first(c.free_cut, cut_occ, [](double l, int kk) { const int v = export_value_host(l); return v == 100 || (v >= kk); }, k);
  return c;
}

// the part of ScanC the beam mixture term needs (also what the handle's table of it is built from at create)
bool mixture_consts(const tbnav_rbpf* h, ScanC& c) {
  const tbnav_rbpf_params& P = h->p;
  c.g = GridC{P.xmin, P.xmax, P.ymin, P.ymax, P.resolution, h->xsize, h->ysize, h->words, h->max_occ_dist, 1.0 / P.resolution};
  c.z_hit = P.z_hit;
  c.var_hit = P.sigma_hit * P.sigma_hit;                       // grid_mapper.cpp:77
  if (almost_equal(c.var_hit, 0.0)) return false;
  c.sqrt_inv_hit = 1.0 / std::sqrt(2.0 * kPI * c.var_hit);    // pdfNormal, grid_mapper.cpp:25
  c.rand_term = P.z_rand / P.z_max;                            // grid_mapper.cpp:121
  return true;
}

int build_scan_consts(tbnav_rbpf* h, ScanC& c, const float* scan, int n_beams, const double u[3],
                      const double cur_odom[3], const double prev_odom[3], int icp_ok, const double T_icp[3],
                      std::vector<double2>& beams) {
  const tbnav_rbpf_params& P = h->p;
  c.N = h->N; c.k = h->k; c.icp_ok = icp_ok ? 1 : 0;
  for (int q = 0; q < 3; ++q) { c.Trs[q] = P.Trs[q]; c.Ld[q] = std::sqrt(P.sample_range[q]); c.Lm[q] = std::sqrt(P.motion_noise[q]);
                                c.Ticp[q] = T_icp[q]; c.u[q] = u[q]; }
  if (!mixture_consts(h, c)) return TBNAV_ERR_PDF_VARIANCE;
  c.scan_min = P.scan_likelihood_min; c.scan_max = P.scan_likelihood_max;
  c.pose_min = P.pose_likelihood_min; c.pose_max = P.pose_likelihood_max;
  c.a1 = P.srr; c.a2 = P.srt; c.a3 = P.str_; c.a4 = P.stt;
  // odometry deltas (particle_filter.cpp:393-403), identical for every particle and sample
  c.rot1 = std::atan2(cur_odom[2] - prev_odom[2], cur_odom[1] - prev_odom[1]) - prev_odom[0];
  const double dxo = cur_odom[1] - prev_odom[1], dyo = cur_odom[2] - prev_odom[2];
  c.trans = std::sqrt(dxo * dxo + dyo * dyo);
  c.rot2 = normalize_angle_PI(normalize_angle_PI(cur_odom[0]) - normalize_angle_PI(prev_odom[0]) - c.rot1);
  c.d_free = h->l_free - h->l_prior;
  c.d_occ = h->l_occ - h->l_prior;
  c.cut_occ = h->cut_occ;
  c.stride_normals = icp_ok ? 3 * h->k + 3 : 3;
  c.p0 = 0;
  // valid beams in the sensor frame, sensor_model.cpp:73-108 (float limits, double angle accumulation)
  // (the angle of beam i does not depend on the scan: its cosine and sine — glibc's, in the reference's accumulation
  //  order — are kept from one call to the next; 2 x 360 libm calls were a tenth of the host's time per scan)
  if ((int)h->beam_cs.size() != n_beams) {
    h->beam_cs.resize(n_beams);
    double beam_angle = P.beam_min;
    for (int i = 0; i < n_beams; ++i) {
      h->beam_cs[i] = double2{std::cos(beam_angle), std::sin(beam_angle)};
      beam_angle += P.beam_delta;
      if (P.beam_max < 0.0 && beam_angle <= P.beam_max) beam_angle = P.beam_min;
      else if (P.beam_max >= 0.0 && beam_angle >= P.beam_max) beam_angle = P.beam_min;
    }
  }
  beams.clear();
  c.rmax = 0.0;
  for (int i = 0; i < n_beams; ++i) {
    const double range = scan[i];
    if (range >= P.range_min && range < P.range_max) {
      beams.push_back(double2{range * h->beam_cs[i].x, range * h->beam_cs[i].y});
      c.rmax = std::max(c.rmax, range);
    }
  }
  c.Bv = (int)beams.size();
  return TBNAV_OK;
}

int status_from_err(const int err[4]) {
  // (first: a scan whose beam table never arrived has computed nothing — whatever else is raised would be an artefact of that)
  if (err[3] & 16) { tbnav::last_hip_error_slot() = "rbpf_propose: the scan's beam table never reached the device (the launch's leading workgroup never published it)"; return TBNAV_ERR_HIP; }
  if (err[0]) return TBNAV_ERR_OUT_OF_WORLD;
  if (err[2]) return TBNAV_ERR_PDF_VARIANCE;
  if (err[1]) return TBNAV_ERR_ETA_ZERO;
  if (err[3] & 8) return TBNAV_ERR_POOL_EXHAUSTED;  // no free log-odds tile left (the scan of that particle was not applied)
  if (err[3] & 4) return TBNAV_ERR_UNSUPPORTED;  // a likelihood lookup left the particle's refreshed window: the window rule (lookup_half_cells) missed a lookup (it once missed the scan matcher's travel)
  if (err[3]) return TBNAV_ERR_BRESENHAM;
  return TBNAV_OK;
}

// The three tiers of the exact distance transform for particles [p0, p0 + count): windowed (tiles_x = the
// tiles a window can span) or whole-map (tiles_x = every tile; the caller has set win/skip accordingly).
int run_distance_field(tbnav_rbpf* h, const GridC& g, int p0, int count, int tiles64) {
  hipStream_t st = h->stream;
  // dense bitmap rows + row counts of these particles, from their tiles
  hipLaunchKernelGGL(rbpf_densify, dim3((h->xsize + 3) / 4, count), dim3(256), 0, st, g, p0, h->pool, map_of(h), h->d_trow[h->cur],
                     h->d_bm_dense, h->d_rc_dense);
  TBNAV_HIP(hipGetLastError());
  // tier 0: <= kEdtRowsA non-empty rows, tier 1: <= kEdtRowsB, tier 2: the general kernel (decided on the device)
  TBNAV_HIP(hipMemsetAsync(h->d_tier + p0, 0, sizeof(int) * count, st));
  const EdtJob job{h->d_win, h->d_skip, p0};
  const dim3 gridc(tiles64, count);
  hipLaunchKernelGGL(rbpf_edt_compact<kEdtRowsA>, gridc, dim3(kWave), edt_compact_lds(kEdtRowsA), st, g, h->radius,
                     h->d_bm_dense, h->d_rc_dense, h->d_code[h->cur], h->d_tier, 0, job);
  TBNAV_HIP(hipGetLastError());
  hipLaunchKernelGGL(rbpf_edt_compact<kEdtRowsB>, gridc, dim3(kWave), edt_compact_lds(kEdtRowsB), st, g, h->radius,
                     h->d_bm_dense, h->d_rc_dense, h->d_code[h->cur], h->d_tier, 1, job);
  TBNAV_HIP(hipGetLastError());
  const int C = h->edt_cols;
  const size_t lds = edt_lds_bytes(h->xsize, h->words, C);
  const dim3 grid(tiles64 * (kWave / C), count);
  if (C == 64) hipLaunchKernelGGL(rbpf_edt<64>, grid, dim3(64), lds, st, g, h->radius, h->d_bm_dense, h->d_code[h->cur], h->d_tier, 2, job);
  else hipLaunchKernelGGL(rbpf_edt<32>, grid, dim3(32), lds, st, g, h->radius, h->d_bm_dense, h->d_code[h->cur], h->d_tier, 2, job);
  TBNAV_HIP(hipGetLastError());
  return TBNAV_OK;
}

GridC grid_of(const tbnav_rbpf* h) {
  return GridC{h->p.xmin, h->p.xmax, h->p.ymin, h->p.ymax, h->p.resolution, h->xsize, h->ysize, h->words, h->max_occ_dist, 1.0 / h->p.resolution};
}

// Whole-field refresh of ONE particle, on demand (state 2 afterwards).
int ensure_full_field(tbnav_rbpf* h, int particle) {
  { const int rc = ensure_codes(h); if (rc != TBNAV_OK) return rc; }
  hipStream_t st = h->stream;
  int stt = 0;
  TBNAV_HIP(hipStreamSynchronize(st));
  TBNAV_HIP(hipMemcpy(&stt, h->d_fstate + particle, sizeof(int), hipMemcpyDeviceToHost));
  if (stt == 2) return TBNAV_OK;
  const int zero = 0, two = 2;
  if (h->edt_cols == 0) {
    const GridC g = grid_of(h);
    hipLaunchKernelGGL(rbpf_field_by_query, dim3((unsigned)((h->G + 255) / 256)), dim3(256), 0, st, g, h->radius, particle,
                       h->pool, map_of(h), h->d_trow[h->cur], h->d_code[h->cur]);
    TBNAV_HIP(hipGetLastError());
    TBNAV_HIP(hipStreamSynchronize(st));
    TBNAV_HIP(hipMemcpy(h->d_fstate + particle, &two, sizeof two, hipMemcpyHostToDevice));
    h->fstate_dirty = true;
    return TBNAV_OK;
  }
  const int4 full = make_int4(0, h->xsize - 1, 0, h->ysize - 1);
  TBNAV_HIP(hipMemcpy(h->d_win + particle, &full, sizeof full, hipMemcpyHostToDevice));
  TBNAV_HIP(hipMemcpy(h->d_skip + particle, &zero, sizeof zero, hipMemcpyHostToDevice));
  int rc = run_distance_field(h, grid_of(h), particle, 1, (h->ysize + kWave - 1) / kWave);
  if (rc != TBNAV_OK) return rc;
  TBNAV_HIP(hipStreamSynchronize(st));
  TBNAV_HIP(hipMemcpy(h->d_fstate + particle, &two, sizeof two, hipMemcpyHostToDevice));
  h->fstate_dirty = true;
  return TBNAV_OK;
}

// lowVarianceResampling's copies on the device: d_parent holds the parent of every slot and, behind them, how many slots
// chose each particle.  One launch (rbpf_resample_apply): tables and reference counts, and state / counts / field state
// into the alternate buffers (the occupancy bits travel with the tiles: nothing of map size is copied).
int resample_on_device(tbnav_rbpf* h) {
  const int N = h->N, nxt = 1 - h->cur;
  hipStream_t st = h->stream;
  const size_t n = (size_t)N * h->TT;
  const int blocks = (int)std::min<size_t>((n + kResampleThreads - 1) / kResampleThreads, 8192);
  const size_t work = h->d_code[0] ? h->G / 4 : (size_t)0;
  const int chunks = (int)std::min<size_t>(std::max<size_t>(work / 2048, 1), 64);
  const GatherArgs ga{h->G, h->TW, h->d_state[h->cur], h->d_state[nxt], h->d_trow[h->cur], h->d_trow[nxt], h->d_nocc[h->cur], h->d_nocc[nxt],
                      h->d_fstate, h->d_fstate_alt, h->d_code[h->cur], h->d_code[nxt], (h->df_mode != 2 || h->ref_field) ? 1 : 0};
  hipLaunchKernelGGL(rbpf_resample_apply, dim3(blocks + N * chunks), dim3(kResampleThreads), 0, st, N, h->TT, h->d_parent, h->d_parent + N,
                     h->d_table[h->cur], h->d_table[nxt], h->d_shed, h->pool, blocks, chunks, ga);
  TBNAV_HIP(hipGetLastError());
  std::swap(h->d_fstate, h->d_fstate_alt);
  h->cur = nxt;
  return TBNAV_OK;
}

#define TBNAV_TRY(call) do { const int tbnav_rc_ = (call); if (tbnav_rc_ != TBNAV_OK) return tbnav_rc_; } while (0)

static int launch_normalize(tbnav_rbpf* h, const NormArgs& a) {
  hipLaunchKernelGGL(rbpf_normalize, dim3(1), dim3(256), 0, h->stream, a.N, a.zp, a.weight, a.weight_out, a.cs, a.parent, a.out,
                     a.gate, a.gate_prev, a.seq, a.seq_val, a.children);
  TBNAV_HIP(hipGetLastError());
  return TBNAV_OK;
}

// default: box counters (rbpf_raycast_box), the form the plan names
static int launch_raycast_box(tbnav_rbpf* h, const ScanC& c, const RaycastPlan& p, const double* sens, const NormArgs* nz, int* err,
                              const double2* beams_dev) {
  const StatePtrs sp = state_ptrs(h->d_state[h->cur], h->N);
  const MapT M = map_of(h);
  unsigned long long* touched = h->count_touched ? h->d_touched : nullptr;
  const NormArgs na = nz ? *nz : NormArgs{0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0u, nullptr};
  const size_t lds_launch = nz ? std::max(p.lds, sizeof(double) * 2 * kNormChunk) : p.lds;  // (workgroup 0's two arrays)
  const int need_slot = (int)(h->rc_launches++ % 3u);
#define TBNAV_X(NT_, WPS_, C16_, EV_)                                                                                                           \
  if (p.threads == NT_ && p.wps == WPS_ && p.c16 == C16_ && p.ev == EV_) {                                                                      \
    hipLaunchKernelGGL((rbpf_raycast_box<NT_, WPS_, C16_, EV_>), dim3(p.grid), dim3(NT_), lds_launch, h->stream, c, h->pool, M, beams_dev,     \
                       sp.pose, sens, h->d_trow[h->cur], h->d_nocc[h->cur], err, (int)p.cap_win, touched, na, h->d_box_need,                   \
                       h->d_box_need_host, need_slot, p.hash_words);                                                                            \
    TBNAV_HIP(hipGetLastError());                                                                                                               \
    return TBNAV_OK;                                                                                                                            \
  }
  TBNAV_RAYCAST_BOX_FORMS(TBNAV_X)
#undef TBNAV_X
  return TBNAV_ERR_UNSUPPORTED;  // (a form the plan names and the list does not have: never another form in its place)
}

// beam-ordered kernel: scans the LDS tile cannot hold, and the reference distance-field mode (it logs the occupied-set changes in
// the reference's order); the normalise behind it as a launch of its own
static int launch_raycast_ordered(tbnav_rbpf* h, const ScanC& c, const RaycastPlan& p, const NormArgs* nz, int* err, const double2* beams_dev) {
  OccLog log{nullptr, nullptr, 0};
  if (h->ref_field) TBNAV_TRY(ref_field_prepare_log(h, c.Bv, log));
  const int bvn = c.Bv > 0 ? c.Bv : 1;
  hipLaunchKernelGGL(rbpf_raycast, dim3(p.grid), dim3(kWave), sizeof(int) * (2 * bvn + (h->TT + 31) / 32), h->stream, c, h->pool, map_of(h),
                     beams_dev, state_ptrs(h->d_state[h->cur], h->N).pose, h->d_trow[h->cur], h->d_nocc[h->cur], err, log,
                     nz ? nz->gate_prev : nullptr);
  TBNAV_HIP(hipGetLastError());
  return nz ? launch_normalize(h, *nz) : TBNAV_OK;
}

// GridMapper::integrateScan's map update (grid_mapper.cpp:140-178) for particles [c.p0, c.p0 + count) at their poses.
// sens: the sensor transforms the proposal kernel left for exactly these poses (NULL: the raycast derives them).
// nz (optional): the weights' normalise / select step to run with this update — inside the box-counter kernel's launch as
// workgroup 0 (no second stream, no event), behind the other map-update kernels as a launch of its own.
// Which kernel, and how large its LDS array: plan_raycast (rbpf_plan.hpp), from the handle's options, the scan and the boxes'
// need — a mapped word the device writes asynchronously, so it is read ONCE: what the selection used is what is reported.
int launch_raycast(tbnav_rbpf* h, const ScanC& c, int count, const double* sens, const NormArgs* nz, int* err,
                   const double2* beams_dev) {
  if (!err) err = h->d_err;
  if (!beams_dev) beams_dev = h->d_beams;
  const int need = (h->raycast_adapt && h->h_box_need) ? *reinterpret_cast<volatile int*>(h->h_box_need) : 0;
  RaycastPlan p = plan_raycast(RaycastIn{h->tile_cap, h->p.resolution, {h->p.Trs[0], h->p.Trs[1], h->p.Trs[2]}, c.rmax, c.Bv,
                                         h->raycast_threads, h->raycast_adapt, h->raycast_cell16, h->raycast_band_rows, need, h->ref_field});
  p.grid = count + (p.box() && nz ? 1 : 0);
  h->last_raycast = p;
  return p.box() ? launch_raycast_box(h, c, p, sens, nz, err, beams_dev) : launch_raycast_ordered(h, c, p, nz, err, beams_dev);
}

// the scan's valid beams into d_beams (shared by slam_impl and the one-particle entry points)
int upload_beams(tbnav_rbpf* h, const std::vector<double2>& beams, int n_beams, int Bv, bool stage_only, int slot) {
  if (n_beams > h->max_beams) {
    TBNAV_HIP(hipStreamSynchronize(h->stream));  // (a scan still in flight reads the buffers about to go)
    (void)hipFree(h->d_beams);
    (void)hipHostFree(h->h_beams);
    h->d_beams = nullptr; h->h_beams = nullptr; h->max_beams = 0;
    TBNAV_HIP(hipMalloc((void**)&h->d_beams, sizeof(double2) * n_beams));
    TBNAV_HIP(hipHostMalloc((void**)&h->h_beams, sizeof(double2) * n_beams * kScanSlots, hipHostMallocDefault));
    h->max_beams = n_beams;
  }
  if (Bv) {
    double2* hb = h->h_beams + (size_t)slot * h->max_beams;
    std::memcpy(hb, beams.data(), sizeof(double2) * Bv);
    if (!stage_only) TBNAV_HIP(hipMemcpyAsync(h->d_beams, hb, sizeof(double2) * Bv, hipMemcpyHostToDevice, h->stream));
  }
  return TBNAV_OK;
}

// ---- the stages of scan_enqueue, in launch order ----------------------------------------------------------------------------------------
static int mark(tbnav_rbpf* h, int i) {   // event timing (tbnav_rbpf_set_timing): ev[i] on the handle's stream
  if (h->timing) TBNAV_HIP(hipEventRecord(h->ev[i], h->stream));
  return TBNAV_OK;
}

// rbpf_sample_normals for the n_norm normals of one scan into d_normals (the last is the resampling offset's).  sharded: this shard's
// slice of the ensemble's stream, from `base`, + the ensemble's resampling offset at z_index (same on every rank); else the
// stream's first n_norm.  n_copy beams are carried from host_beams to dev_beams on the way.
static int launch_sample_normals(tbnav_rbpf* h, size_t n_norm, unsigned long long seed, unsigned long long scan, bool sharded, size_t base,
                                 size_t z_index, const double2* host_beams, double2* dev_beams, int n_copy) {
  const int blocks = (int)std::min<size_t>((n_norm / 2 + 255) / 256, 4096);
  hipLaunchKernelGGL(rbpf_sample_normals, dim3(blocks), dim3(256), 0, h->stream, sharded ? n_norm - 1 : n_norm, seed, scan, h->d_normals,
                     host_beams, dev_beams, n_copy, (size_t)0, (size_t)0, sharded ? base : (size_t)0, sharded ? z_index : ~(size_t)0,
                     sharded ? n_norm - 1 : (size_t)0);
  TBNAV_HIP(hipGetLastError());
  return TBNAV_OK;
}

// What the hand-over of device noise needs: the offset's slot, the "table is there" words and a copy of the beam table, the last two
// in fine-grained device memory.  false: the platform gives none — the option switches itself off for good (the stored-first form
// computes the same values).
static bool ensure_noise_handover(tbnav_rbpf* h) {
  hipError_t ea = hipSuccess;
  if (!h->d_zslot) {
    ea = hipMalloc((void**)&h->d_zslot, sizeof(double));
    if (ea == hipSuccess) ea = hipExtMallocWithFlags((void**)&h->d_beam_ready, sizeof(unsigned int) * kReadyCopies * kReadyStride, hipDeviceMallocFinegrained);
    if (ea == hipSuccess) ea = hipMemsetAsync(h->d_beam_ready, 0, sizeof(unsigned int) * kReadyCopies * kReadyStride, h->stream);
    h->beam_seq = 0;
  }
  if (ea == hipSuccess && h->fg_beams_cap < h->max_beams) {
    ea = hipStreamSynchronize(h->stream);
    (void)hipFree(h->d_beams_fg); h->d_beams_fg = nullptr; h->fg_beams_cap = 0;
    if (ea == hipSuccess) ea = hipExtMallocWithFlags((void**)&h->d_beams_fg, sizeof(double2) * h->max_beams, hipDeviceMallocFinegrained);
    if (ea == hipSuccess) h->fg_beams_cap = h->max_beams;
  }
  if (ea == hipSuccess) return true;
  (void)hipGetLastError();
  (void)hipFree(h->d_zslot); (void)hipFree(h->d_beam_ready); (void)hipFree(h->d_beams_fg);
  h->d_zslot = nullptr; h->d_beam_ready = nullptr; h->d_beams_fg = nullptr; h->fg_beams_cap = 0;
  h->noise_in_kernel = 0;
  return false;
}

// The scan's noise, staged: where the proposal kernel gets its normals from, and the handle's record of it (last_drawn / last_normals /
// last_z_*: tbnav_rbpf_get_normals, the normalise).  in_kernel: drawn inside the proposal kernel, whose leading workgroup also carries
// the beam table over (src) — unless a kernel in front of it needs the table on the device (the per-particle scan matcher), the scan
// comes prepared with its chunk (tbnav_rbpf_slam_batch), or the option is off: then `normals` is a stored stream — the caller's,
// the batch's, or what rbpf_sample_normals stores first, as up to round 4
// (... or the reference-field mode may have to run the proposal twice: the stored stream is there for the second run)
struct ScanNoise { NoiseSrc src{}; const double* normals = nullptr; bool in_kernel = false; };
static int stage_noise(tbnav_rbpf* h, const ScanC& c, const double* normals, const Prefetched* pre, int slot, ScanNoise& out) {
  hipStream_t st = h->stream;
  const size_t n_norm = (size_t)h->N * c.stride_normals + 1;
  const double2* const host_beams = h->h_beams + (size_t)slot * h->max_beams;
  const bool sharded = h->rng_n_global != 0;  // this shard's slice of the ensemble's stream + the ensemble's resampling offset
  const size_t base = sharded ? (size_t)h->rng_first * c.stride_normals : 0;
  const size_t z_index = sharded ? (size_t)h->rng_n_global * c.stride_normals : (size_t)h->N * c.stride_normals;
  bool dn = !pre && !normals && !(h->sm_on && c.icp_ok) && h->noise_in_kernel == 1 && !h->ref_field;
  if (dn) dn = ensure_noise_handover(h);
  h->last_drawn.valid = false;
  if (dn) {
    if (++h->beam_seq == 0u) ++h->beam_seq;   // (0 is the cleared word)
    out.src = NoiseSrc{h->seed, h->scan_index, base, z_index, h->d_zslot, host_beams, h->d_beams, h->d_beams_fg, h->d_beam_ready, h->beam_seq};
    h->last_drawn.seed = h->seed; h->last_drawn.scan = h->scan_index; h->last_drawn.base = base; h->last_drawn.z_index = z_index;
    h->last_drawn.n = n_norm; h->last_drawn.valid = true;
  } else if (!pre) {   // (a prepared scan's were drawn with the rest of its chunk)
    if (n_norm > h->normals_cap) {
      TBNAV_HIP(hipStreamSynchronize(st));  // (a scan still in flight reads the old buffer)
      (void)hipFree(h->d_normals);
      h->d_normals = nullptr;
      TBNAV_HIP(hipMalloc((void**)&h->d_normals, sizeof(double) * n_norm));
      h->normals_cap = n_norm;
    }
    if (normals) TBNAV_HIP(hipMemcpyAsync(h->d_normals, normals, sizeof(double) * n_norm, hipMemcpyHostToDevice, st));
    else TBNAV_TRY(launch_sample_normals(h, n_norm, h->seed, h->scan_index, sharded, base, z_index, host_beams, h->d_beams, c.Bv));
  }
  ++h->scan_index;
  out.in_kernel = dn;
  out.normals = dn ? nullptr : (pre ? pre->d_normals : h->d_normals);
  h->last_normals = out.normals;
  h->last_z_index = (size_t)h->N * c.stride_normals;
  h->last_z_ptr = dn ? h->d_zslot : out.normals + h->last_z_index;
  return TBNAV_OK;
}

// Distance-field refresh for this call's lookups, windowed (the stored-field modes; query mode needs neither windows nor skip
// flags: the proposal kernel reads the field state itself)
static int refresh_fields(tbnav_rbpf* h, const ScanC& c, const double u[3], const double T_icp[3], double spread, bool matching) {
  if (h->df_mode == 2) return TBNAV_OK;
  const int half_cells = lookup_half_cells((double)h->p.range_max, h->p.Trs, T_icp, u, spread, matching ? h->sm.max_moves * h->sm.lstep : 0.0,
                                           h->p.resolution, h->full_edt, h->xsize);
  hipLaunchKernelGGL(rbpf_window, dim3((h->N + 255) / 256), dim3(256), 0, h->stream, c.g, h->N, half_cells, h->df_mode == 1 ? 1 : 0,
                     state_ptrs(h->d_state[h->cur], h->N).pose, h->d_fstate, h->d_skip, h->d_win);
  TBNAV_HIP(hipGetLastError());
  if (h->df_mode != 1) return TBNAV_OK;
  const int tiles = std::min((2 * half_cells + 1 + kWave - 1) / kWave + 1, (h->ysize + kWave - 1) / kWave);
  return run_distance_field(h, c.g, 0, h->N, tiles);
}

// which particles' lookups go to the stored field: skip[p] == eq (query mode reads the field state itself)
struct SkipRule { const int* arr; int eq; };
static SkipRule skip_rule(const tbnav_rbpf* h) { return h->df_mode == 2 ? SkipRule{h->d_fstate, 2} : SkipRule{h->d_skip, 1}; }

// N1 option: every particle refines T(pose) * T_icp against its own map first; the samples are drawn round that (d_center)
static int launch_scanmatch(tbnav_rbpf* h, const ScanC& c, const ProposePlan& pp, const double2* beams_dev, int* d_err, const int* gate_prev) {
  const SkipRule sk = skip_rule(h);
  hipLaunchKernelGGL(rbpf_scanmatch, dim3(h->N), dim3(kMatchThreads), pp.sm_lds, h->stream, c, h->sm, beams_dev, h->d_code[h->cur],
                     h->pool, map_of(h), h->d_trow[h->cur], sk.arr, sk.eq, h->df_mode, h->radius, pp.occ_half,
                     h->d_nocc[h->cur], h->d_win, state_ptrs(h->d_state[h->cur], h->N).pose, h->d_center, h->d_score, d_err, gate_prev, h->d_mixlut);
  TBNAV_HIP(hipGetLastError());
  return TBNAV_OK;
}

// the proposal, in the form the plan names (center: the matcher's poses, or NULL)
static int launch_propose(tbnav_rbpf* h, const ScanC& c, const ProposePlan& pp, const ScanNoise& nz, const double2* beams_dev, const double* center,
                          int* d_err, const int* gate_prev) {
  const SkipRule sk = skip_rule(h);
  const StatePtrs sp = state_ptrs(h->d_state[h->cur], h->N);
  int* const pend = h->ref_field ? h->d_pend : nullptr;
  h->last_propose = pp;
#define TBNAV_X(NT_, DN_)                                                                                                                        \
  if (pp.threads == NT_ && pp.dn == DN_) {                                                                                                       \
    hipLaunchKernelGGL((rbpf_propose<NT_, DN_>), dim3(h->N + (DN_ ? 1 : 0)), dim3(NT_), pp.lds, h->stream, c, beams_dev, h->d_code[h->cur],      \
                       h->pool, map_of(h), h->d_trow[h->cur], sk.arr, sk.eq, h->df_mode, h->radius, pp.occ_half, h->d_nocc[h->cur], h->d_win,    \
                       nz.normals, center, sp.pose, sp.prev, sp.weight, h->tr, h->d_sens, d_err, gate_prev, h->d_mixlut, nz.src, pend);          \
    TBNAV_HIP(hipGetLastError());                                                                                                                \
    return TBNAV_OK;                                                                                                                             \
  }
  TBNAV_PROPOSE_FORMS(TBNAV_X)
#undef TBNAV_X
  return TBNAV_ERR_UNSUPPORTED;  // (a form the plan names and the list does not have)
}

// legacy placement (TBNAV_RBPF_FULL_EDT=1): whole field of every particle right after the map update,
// where the reference runs its brushfire (grid_mapper.cpp:181)
static int place_full_fields(tbnav_rbpf* h, const ScanC& c) {
  TBNAV_HIP(hipMemsetAsync(h->d_skip, 0, sizeof(int) * h->N, h->stream));
  return run_distance_field(h, c.g, 0, h->N, (h->ysize + kWave - 1) / kWave);
}

// the map changed: every field is stale until the next refresh (whole-map mode: fresh everywhere).  In query mode
// the states are all zero already unless a field was injected or materialised since the last call.
static int mark_fields_stale(tbnav_rbpf* h) {
  if (h->full_edt) {
    TBNAV_HIP(hipMemsetD32Async((hipDeviceptr_t)h->d_fstate, 2, h->N, h->stream));
    h->fstate_dirty = true;
  } else if (h->fstate_dirty || h->df_mode != 2) {
    TBNAV_HIP(hipMemsetD32Async((hipDeviceptr_t)h->d_fstate, 0, h->N, h->stream));
    h->fstate_dirty = h->df_mode != 2;
  }
  return TBNAV_OK;
}

int scan_enqueue(tbnav_rbpf* h, const float* scan, int n_beams, const double u[3], const double cur_odom[3],
                 const double prev_odom[3], int icp_ok, const double T_icp[3], const double* normals,
                 tbnav_rbpf_stats* out, bool local_only, int slot, const int* gate_prev, ScanTicket& tk,
                 const Prefetched* pre, hipEvent_t weights_ready) {
  int* const d_err = h->d_err + 4 * slot;
  int* const h_err = h->h_err + 4 * slot;
  ++h->scans_done;
  ScanC c;
  std::vector<double2>& beams = h->beams_tmp;  // (kept between calls: no allocation per scan)
  int rc;
  if (pre) { c = pre->c; rc = pre->rc; }
  else rc = build_scan_consts(h, c, scan, n_beams, u, cur_odom, prev_odom, icp_ok, T_icp, beams);
  std::memset(out, 0, sizeof *out);
  if (rc != TBNAV_OK) { out->status = rc; return rc; }
  out->n_valid_beams = c.Bv;
  tk.slot = slot; tk.n_valid = c.Bv; tk.local_only = local_only;
  // (device noise: the noise kernel carries the beams over)
  if (!pre) TBNAV_TRY(upload_beams(h, beams, n_beams, c.Bv, /*stage_only=*/normals == nullptr, slot));
  ScanNoise noise;
  TBNAV_TRY(stage_noise(h, c, normals, pre, slot, noise));
  const double2* const beams_dev = pre ? pre->d_beams : h->d_beams;
  for (int q = 0; q < 4; ++q) h_err[q] = 0;  // mapped: the scan that last owned the slot has been waited for
  h->h_norm[slot] = NormOut{};
  const bool matching = h->sm_on && c.icp_ok;
  const double spread = sampling_spread(h->p.sample_range, h->p.motion_noise);
  ProposePlan pp = plan_propose(ProposeIn{h->k, c.Bv, h->df_mode, h->xsize, h->words, (double)h->p.range_max, spread, h->p.resolution});
  pp.dn = noise.in_kernel;

  // ---- distance-field refresh for this call's lookups (windowed), then the particle update
  if (h->ref_field) { rc = ref_field_before_propose(h); if (rc != TBNAV_OK) { out->status = rc; return rc; } }
  TBNAV_TRY(mark(h, 0));
  TBNAV_TRY(refresh_fields(h, c, u, T_icp, spread, matching));
  TBNAV_TRY(mark(h, 1));
  if (!pp.fits) return TBNAV_ERR_UNSUPPORTED;  // scan x samples too large for one workgroup's LDS
  if (matching) TBNAV_TRY(launch_scanmatch(h, c, pp, beams_dev, d_err, gate_prev));
  const double* const center = matching ? h->d_center : nullptr;
  TBNAV_TRY(launch_propose(h, c, pp, noise, beams_dev, center, d_err, gate_prev));
  if (h->ref_field) {  // lookups that met cells the lazy brushfire has not written: resume those states, run the proposal again
    rc = ref_field_settle(h, h_err, [&]() { return launch_propose(h, c, pp, noise, beams_dev, center, d_err, gate_prev); });
    if (rc != TBNAV_OK) { out->status = rc; return rc; }
  }
  if (weights_ready) TBNAV_HIP(hipEventRecord(weights_ready, h->stream));  // (sharded filter: the exchange starts here, beside the map update)
  TBNAV_TRY(mark(h, 2));
  // normalise / select needs only the weights the proposal kernel left: it rides in the map update's launch as one extra
  // workgroup (the chain of adds it is made of would otherwise sit on the critical path, and a second stream costs an
  // event and a dependent boundary).  With event timing on it is a launch of its own, so that the intervals mean what
  // they say.
  tk.seq = (unsigned int)h->scans_done;
  double* const weight = state_ptrs(h->d_state[h->cur], h->N).weight;
  const NormArgs nz{h->N, h->last_z_ptr, weight, weight, h->d_cs, h->d_parent, h->d_norm + slot, h->d_gate + slot, gate_prev,
                    tk.poll ? h->d_seq + slot : nullptr, tk.seq, h->d_parent + h->N};
  const bool overlap = !local_only && !h->timing;
  if ((gate_prev || tk.poll) && !overlap) return TBNAV_ERR_INVALID_ARG;  // (a gated or polled scan is a batch scan: never local-only or timed)
  TBNAV_TRY(launch_raycast(h, c, h->N, h->d_sens, overlap ? &nz : nullptr, d_err, beams_dev));
  TBNAV_TRY(mark(h, 3));
  if (h->full_edt) TBNAV_TRY(place_full_fields(h, c));
  TBNAV_TRY(mark(h, 4));
  if (!local_only && !overlap)   // (no gate, no flag: see above)
    TBNAV_TRY(launch_normalize(h, NormArgs{nz.N, nz.zp, nz.weight, nz.weight_out, nz.cs, nz.parent, nz.out, nullptr, nullptr, nullptr, 0u, nz.children}));
  TBNAV_TRY(mark(h, 5));
  return mark_fields_stale(h);
}

int scan_finish(tbnav_rbpf* h, const ScanTicket& tk, tbnav_rbpf_stats* out) {
  hipStream_t st = h->stream;
  const bool local_only = tk.local_only;
  int rc = TBNAV_OK;
  if (tk.poll) {
    // the normalise / select workgroup raises the slot's flag as soon as its result is in host memory — the host need not
    // wait for the rest of the map update (error flags raised later in that launch: see tbnav_rbpf_slam_batch)
    volatile unsigned int* flag = h->h_seq + tk.slot;
    for (unsigned long spins = 1; *flag != tk.seq; ++spins) {
      __builtin_ia32_pause();
      if ((spins & 0xFFFF) == 0) {
        const hipError_t q = hipStreamQuery(st);
        if (q == hipSuccess && *flag != tk.seq) return TBNAV_ERR_HIP;  // the stream drained and the flag never came
        if (q != hipSuccess && q != hipErrorNotReady) TBNAV_HIP(q);
      }
    }
    std::atomic_thread_fence(std::memory_order_acquire);
  } else {
    TBNAV_HIP(hipStreamSynchronize(st));
  }
  const int* err = h->h_err + 4 * tk.slot;
  const NormOut no = h->h_norm[tk.slot];
  out->status = status_from_err(err);
  out->sum_w = no.sum_w; out->sq_sum = no.sq_sum; out->neff = no.neff; out->resampled = no.resampled;
  bool gathered = false;
  if (!local_only && no.resampled && out->status == TBNAV_OK) {
    // lowVarianceResampling's deep copies (particle_filter.cpp:495): tables and state move on the device
    if (h->timing) TBNAV_HIP(hipEventRecord(h->ev[6], st));
    rc = resample_on_device(h);
    if (rc != TBNAV_OK) return rc;
    if (h->timing) TBNAV_HIP(hipEventRecord(h->ev[7], st));
    gathered = true;
  }
  if (gathered && !tk.poll) TBNAV_HIP(hipStreamSynchronize(st));  // (a batch goes straight on: the next scan is behind the copies in the stream)
  for (float& v : h->last_ms) v = 0.f;
  if (h->timing) {
    float e01, e12, e23, e34, e45;
    TBNAV_HIP(hipEventElapsedTime(&e01, h->ev[0], h->ev[1]));
    TBNAV_HIP(hipEventElapsedTime(&e12, h->ev[1], h->ev[2]));
    TBNAV_HIP(hipEventElapsedTime(&e23, h->ev[2], h->ev[3]));
    TBNAV_HIP(hipEventElapsedTime(&e34, h->ev[3], h->ev[4]));
    TBNAV_HIP(hipEventElapsedTime(&e45, h->ev[4], h->ev[5]));
    h->last_ms[0] = e12;        // propose
    h->last_ms[1] = e23;        // raycast
    h->last_ms[2] = 0.f;        // (occupancy pass: folded into the raycast)
    h->last_ms[3] = e01 + e34;  // distance field (windowed refresh before the update, or whole-map after it)
    h->last_ms[4] = e45;        // normalise / select
    if (gathered) TBNAV_HIP(hipEventElapsedTime(&h->last_ms[5], h->ev[6], h->ev[7]));
  }
  if (h->ref_field && out->status == TBNAV_OK) {
    rc = ref_field_after_scan(h, gathered);
    if (rc != TBNAV_OK) return rc;
  }
  return out->status;
}

int slam_impl(tbnav_rbpf* h, const float* scan, int n_beams, const double u[3], const double cur_odom[3],
              const double prev_odom[3], int icp_ok, const double T_icp[3], const double* normals,
              tbnav_rbpf_stats* out, bool local_only) {
  if (!h || !scan || n_beams <= 0 || !u || !cur_odom || !prev_odom || !T_icp || !out) return TBNAV_ERR_INVALID_ARG;
  if (h->ref_field && (local_only || h->comm)) return TBNAV_ERR_UNSUPPORTED;  // the reference-field mode is a single-handle mode
  if (h->comm && !local_only) {  // this process's rank of a sharded filter: the exchange is issued from here (sharded_scan)
    const double* nr[1] = {normals};
    return sharded_scan(1, &h, scan, n_beams, u, cur_odom, prev_odom, icp_ok, T_icp, nr, out, nullptr);
  }
  DeviceGuard guard(h->device);
  ScanTicket tk;
  const int rc = scan_enqueue(h, scan, n_beams, u, cur_odom, prev_odom, icp_ok, T_icp, normals, out, local_only, 0, nullptr, tk);
  if (rc != TBNAV_OK) return rc;
  return scan_finish(h, tk, out);
}

// host threads for the reference-field mode: the cores this process may run on — its affinity mask, and under a cgroup CPU quota
// (cpu.max: a container that sees 128 CPUs but may use 32 of them) no more than that — at most 128; TBNAV_RBPF_OPT_HOST_THREADS
// overrides.  (Round 4 capped this at 32: the bench box has more.)
int host_cpu_budget(double& quota_cpus) {
  int n = 0;
  cpu_set_t set;
  if (sched_getaffinity(0, sizeof set, &set) == 0) n = CPU_COUNT(&set);
  if (n <= 0) n = (int)std::thread::hardware_concurrency();
  if (n < 1) n = 1;
  quota_cpus = (double)n;
  if (FILE* f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {   // cgroup v2: "<quota> <period>" or "max <period>"
    long long quota = 0, period = 0;
    if (std::fscanf(f, "%lld %lld", &quota, &period) == 2 && quota > 0 && period > 0) quota_cpus = std::min((double)n, (double)quota / (double)period);
    std::fclose(f);
  }
  return n;
}
int default_host_threads() {
  double q = 1.0;
  const int n = host_cpu_budget(q);
  const int t = std::min(n, (int)std::ceil(q));
  return t < 1 ? 1 : (t > 128 ? 128 : t);
}
// free lists: rbpf_device.hpp.  (TBNAV_POOL_SHARD_MIN: a test hook — the GPU suite is run once with every pool of 32 tiles or
//  more on sixteen lists, so that the small parity cases pop from lists a few tiles long, move on and gather all the time)
unsigned int pool_lists_for(size_t cap_tiles) {
  size_t shard_min = kPoolShardMin;
  if (const char* ev = std::getenv("TBNAV_POOL_SHARD_MIN")) { const long v = std::atol(ev); if (v >= kPoolShards) shard_min = (size_t)v; }
  return cap_tiles >= shard_min ? (unsigned int)kPoolShards : 1u;
}
int pool_free_tiles(tbnav_rbpf* h, uint64_t* free_tiles) {
  unsigned long long ctr[kPoolCtrWords];
  TBNAV_HIP(hipMemcpy(ctr, h->pool.ctr, sizeof ctr, hipMemcpyDeviceToHost));
  uint64_t f = 0;
  for (unsigned int s = 0; s < h->pool.shards; ++s) f += ctr[s * kPoolCtrStride + 1] - ctr[s * kPoolCtrStride];
  *free_tiles = f;
  return TBNAV_OK;
}
// ---- create, in stages: each goes on only while `e` is hipSuccess and leaves the first failure in it ---------------------------------------
static void dev_alloc(hipError_t& e, void** p, size_t bytes) { if (e == hipSuccess) e = hipMalloc(p, bytes); }
#define TBNAV_A(ptr, bytes) dev_alloc(e, (void**)&(ptr), (bytes))

static void create_buffers(tbnav_rbpf* h, hipError_t& e) {
  const int N = h->N;
  const size_t table_entries = (size_t)N * h->TT;
  for (int b = 0; b < 2; ++b) {
    TBNAV_A(h->d_state[b], sizeof(double) * 7 * N);
    TBNAV_A(h->d_table[b], sizeof(unsigned int) * table_entries);
    TBNAV_A(h->d_nocc[b], sizeof(int) * N);
    TBNAV_A(h->d_trow[b], sizeof(int) * (size_t)N * h->TW);
  }
  TBNAV_A(h->d_shed, sizeof(unsigned int) * table_entries);
  TBNAV_A(h->d_cs, sizeof(double) * N);
  TBNAV_A(h->d_sens, sizeof(double) * 4 * N);
  TBNAV_A(h->d_tile_scratch, sizeof(unsigned int) * h->TT);
  TBNAV_A(h->d_touched, sizeof(unsigned long long) * 2);
  TBNAV_A(h->d_box_need, sizeof(int) * 3);
  TBNAV_A(h->d_parent, sizeof(int) * 2 * N);
  TBNAV_A(h->d_best, sizeof(int));
  TBNAV_A(h->d_best_pose, sizeof(double) * 3);
  TBNAV_A(h->d_export, h->G);
  TBNAV_A(h->d_fstate, sizeof(int) * N);
  TBNAV_A(h->d_fstate_alt, sizeof(int) * N);
  TBNAV_A(h->d_center, sizeof(double) * 3 * N);
  TBNAV_A(h->d_score, sizeof(double) * N);
  TBNAV_A(h->d_skip, sizeof(int) * N);
  TBNAV_A(h->d_win, sizeof(int4) * N);
  TBNAV_A(h->d_tier, sizeof(int) * N);
  if (e == hipSuccess) e = hipHostMalloc((void**)&h->h_err, sizeof(int) * 4 * kScanSlots, hipHostMallocMapped);
  if (e == hipSuccess) e = hipHostMalloc((void**)&h->h_norm, sizeof(NormOut) * kScanSlots, hipHostMallocMapped);
  if (e == hipSuccess) { std::memset(h->h_err, 0, sizeof(int) * 4 * kScanSlots); std::memset((void*)h->h_norm, 0, sizeof(NormOut) * kScanSlots); }
  TBNAV_A(h->d_gate, sizeof(int) * kScanSlots);
  if (e == hipSuccess) e = hipMemset(h->d_gate, 0, sizeof(int) * kScanSlots);
  if (e == hipSuccess) e = hipHostMalloc((void**)&h->h_seq, sizeof(unsigned int) * kScanSlots, hipHostMallocMapped);
  if (e == hipSuccess) { std::memset(h->h_seq, 0, sizeof(unsigned int) * kScanSlots); e = hipHostGetDevicePointer((void**)&h->d_seq, h->h_seq, 0); }
  if (e == hipSuccess) e = hipHostGetDevicePointer((void**)&h->d_err, h->h_err, 0);
  if (e == hipSuccess) e = hipHostGetDevicePointer((void**)&h->d_norm, h->h_norm, 0);
  // the proposal's trace: sampled, p_scan, p_pose, mu, sigma, eta, new_pose, weight_raw, back to back
  const size_t kk = (size_t)h->k;
  const size_t trace_doubles = (size_t)N * (kk * 3 + kk + kk + 3 + 9 + 1 + 3 + 1);
  TBNAV_A(h->d_trace, sizeof(double) * trace_doubles);
  if (e == hipSuccess) {
    double* t = h->d_trace;
    h->tr.sampled = t; t += (size_t)N * kk * 3;
    h->tr.p_scan = t; t += (size_t)N * kk;
    h->tr.p_pose = t; t += (size_t)N * kk;
    h->tr.mu = t; t += (size_t)N * 3;
    h->tr.sigma = t; t += (size_t)N * 9;
    h->tr.eta = t; t += (size_t)N;
    h->tr.new_pose = t; t += (size_t)N * 3;
    h->tr.weight_raw = t;
    e = hipMemset(h->d_trace, 0, sizeof(double) * trace_doubles);
  }
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
  for (auto& ev : h->ev) if (e == hipSuccess) e = hipEventCreate(&ev);
}

// the tile pool: everything the particles' maps can ever need if that fits the budget, else the budget.
// Default budget: half of the memory that is free now (several handles can live side by side).
static void create_pool(tbnav_rbpf* h, uint64_t max_pool_bytes, hipError_t& e) {
  if (e != hipSuccess) return;
  size_t free_b = 0, total_b = 0;
  e = hipMemGetInfo(&free_b, &total_b);
  const size_t per_tile = sizeof(double) * kTileCells + sizeof(unsigned int) * kTS + sizeof(int) + sizeof(unsigned int);
  const size_t budget = max_pool_bytes ? (size_t)max_pool_bytes : free_b / 2;
  // worst case: every table entry its own tile, plus the tiles the entries left since the last resample (still named by
  // the shed notes until the next resample settles them), plus the zero tile
  size_t cap = 2 * (size_t)h->N * h->TT + 1;
  if (cap * per_tile > budget) cap = budget / per_tile;
  if (cap > 0xFFFFFFF0ull) cap = 0xFFFFFFF0ull;
  if (cap < (size_t)h->N + 2 && e == hipSuccess) e = hipErrorOutOfMemory;  // not even one tile per particle
  h->pool.cap = (unsigned int)cap;
  h->pool.shards = pool_lists_for(cap);
  h->pool.shard_cap = (unsigned int)((cap + h->pool.shards - 1) / h->pool.shards);
  TBNAV_A(h->pool.lo, sizeof(double) * kTileCells * cap);
  TBNAV_A(h->pool.bm, sizeof(unsigned int) * kTS * cap);
  TBNAV_A(h->pool.ref, sizeof(int) * cap);
  TBNAV_A(h->pool.ring, sizeof(unsigned int) * (size_t)h->pool.shard_cap * h->pool.shards);
  TBNAV_A(h->pool.ctr, sizeof(unsigned long long) * kPoolCtrWords);
}

// initParticleSet, particle_filter.cpp:125-138, and empty maps
static void create_state(tbnav_rbpf* h, hipError_t& e) {
  if (e != hipSuccess) return;
  const int N = h->N;
  const size_t table_entries = (size_t)N * h->TT;
  std::vector<double> s((size_t)7 * N);
  for (int i = 0; i < N; ++i) {
    for (int q = 0; q < 3; ++q) { s[(size_t)i * 3 + q] = h->p.pose0[q]; s[(size_t)3 * N + i * 3 + q] = h->p.pose0[q]; }
    s[(size_t)6 * N + i] = 1.0 / N;
  }
  e = hipMemcpy(h->d_state[0], s.data(), sizeof(double) * 7 * N, hipMemcpyHostToDevice);
  // empty maps: every table entry names the shared zero tile (log_odds_prior_ = log(1) = 0)
  if (e == hipSuccess) e = hipMemset(h->d_table[0], 0, sizeof(unsigned int) * table_entries);
  if (e == hipSuccess) e = hipMemset(h->d_shed, 0, sizeof(unsigned int) * table_entries);
  if (e == hipSuccess) e = hipMemset(h->pool.lo, 0, sizeof(double) * kTileCells);  // tile 0
  if (e == hipSuccess) e = hipMemset(h->pool.ref, 0, sizeof(int) * h->pool.cap);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(rbpf_pool_init, dim3(1024), dim3(256), 0, h->stream, h->pool);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemset(h->d_touched, 0, sizeof(unsigned long long) * 2);
  if (e == hipSuccess) {  // the queue's scratch memory, before the first map update that needs it (see the kernel)
    hipLaunchKernelGGL(rbpf_warm_scratch, dim3(1024), dim3(512), 0, h->stream, reinterpret_cast<int*>(h->d_touched), 0);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemset(h->d_box_need, 0, sizeof(int) * 3);
  if (e == hipSuccess) e = hipHostMalloc((void**)&h->h_box_need, sizeof(int), hipHostMallocMapped);
  if (e == hipSuccess) { *h->h_box_need = 0; e = hipHostGetDevicePointer((void**)&h->d_box_need_host, h->h_box_need, 0); }
  if (e == hipSuccess) e = hipMemset(h->d_nocc[0], 0, sizeof(int) * N);
  if (e == hipSuccess) e = hipMemset(h->d_skip, 0, sizeof(int) * N);
  if (e == hipSuccess) e = hipMemset(h->d_tier, 0xFF, sizeof(int) * N);  // -1: no transform launch has covered the particle yet (tbnav_rbpf_last_field_kernels)
  // empty maps: the field "everything unreached" is what any lookup computes, no stored field needed (state 0)
  if (e == hipSuccess) e = hipMemset(h->d_fstate, 0, sizeof(int) * N);
  if (e == hipSuccess) e = hipMemset(h->d_fstate_alt, 0, sizeof(int) * N);
  h->fstate_dirty = false;
  if (e == hipSuccess) {
    std::vector<int4> w(N, make_int4(0, h->xsize - 1, 0, h->ysize - 1));
    e = hipMemcpy(h->d_win, w.data(), sizeof(int4) * N, hipMemcpyHostToDevice);
  }
  if (e == hipSuccess) e = hipMemset(h->d_trow[0], 0, sizeof(int) * (size_t)N * h->TW);
  if (e == hipSuccess) e = hipMemset(h->pool.bm, 0, sizeof(unsigned int) * kTS);  // tile 0
}

// dynamic LDS beyond the 64 KB default, for every kernel form that can be launched with it (the forms: rbpf_device.hpp's lists)
static void create_lds_attributes(tbnav_rbpf* h, hipError_t& e) {
  auto lds = [&e](const void* kernel, size_t bytes) { if (e == hipSuccess) e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes); };
  if (h->edt_cols == 64) lds(reinterpret_cast<const void*>(&rbpf_edt<64>), edt_lds_bytes(h->xsize, h->words, 64));
  if (h->edt_cols == 32) lds(reinterpret_cast<const void*>(&rbpf_edt<32>), edt_lds_bytes(h->xsize, h->words, 32));
  // (2.3 KB of static LDS: the embedded normalise's scan scratch)
#define TBNAV_X(NT_, WPS_, C16_, EV_) lds(reinterpret_cast<const void*>(&rbpf_raycast_box<NT_, WPS_, C16_, EV_>), kMaxLds - 4096);
  TBNAV_RAYCAST_BOX_FORMS(TBNAV_X)
#undef TBNAV_X
  lds(reinterpret_cast<const void*>(&rbpf_raycast), kMaxLds - 1024);
  // the proposal / scan-match kernels carry the scan, the per-sample data and the bitmap slice: more than the 64 KB
  // default for long scans or many samples
#define TBNAV_X(NT_, DN_) lds(reinterpret_cast<const void*>(&rbpf_propose<NT_, DN_>), kMaxLds - 3072);   /* (2.3 KB static) */
  TBNAV_PROPOSE_FORMS(TBNAV_X)
#undef TBNAV_X
  lds(reinterpret_cast<const void*>(&rbpf_scanmatch), kMaxLds - 1024);
  lds(reinterpret_cast<const void*>(&rbpf_edt_compact<kEdtRowsA>), edt_compact_lds(kEdtRowsA));
  lds(reinterpret_cast<const void*>(&rbpf_edt_compact<kEdtRowsB>), edt_compact_lds(kEdtRowsB));
}

// the beam mixture term per distance code: constants of the handle, tabulated once
static void create_mix_lut(tbnav_rbpf* h, hipError_t& e) {
  TBNAV_A(h->d_mixlut, sizeof(double) * kMixLut);
  ScanC cm{};
  if (e == hipSuccess && mixture_consts(h, cm)) {  // (a zero variance is reported by the first scan, as the reference throws there)
    hipLaunchKernelGGL(rbpf_mix_lut, dim3(kMixLut / 256), dim3(256), 0, h->stream, cm, h->d_mixlut);
    e = hipGetLastError();
  }
}
#undef TBNAV_A

int create_impl(const tbnav_rbpf_params* P, uint64_t max_pool_bytes, tbnav_rbpf** out) {
  if (!P || !out) return TBNAV_ERR_INVALID_ARG;
  *out = nullptr;
  if (P->num_particles <= 0 || P->num_samples_mode <= 0 || !(P->resolution > 0.0) || !(P->xmax > P->xmin) || !(P->ymax > P->ymin))
    return TBNAV_ERR_INVALID_ARG;
  const int xsize = (int)static_cast<unsigned int>(std::ceil((P->xmax - P->xmin) / P->resolution));  // mapSize, grid_mapper.cpp:31-34
  const int ysize = (int)static_cast<unsigned int>(std::ceil((P->ymax - P->ymin) / P->resolution));
  if (xsize != ysize) return TBNAV_ERR_UNSUPPORTED;  // the reference indexes both axes with xsize_ (grid_mapper.cpp:195-197,896)
  if (xsize < 4 || xsize > 32000 || (xsize & 1)) return TBNAV_ERR_UNSUPPORTED;  // vectorised code copies need G % 4 == 0
  if (P->num_particles > (1 << 20)) return TBNAV_ERR_UNSUPPORTED;
  const int radius = (int)static_cast<unsigned int>(std::ceil((10.0 - 0.0) / P->resolution));         // cell_radius_, grid_mapper.cpp:50
  if (radius > 254) return TBNAV_ERR_UNSUPPORTED;  // row-pass distances are stored as u8 (and radius^2 must fit the u16 code)
  int dev = 0;
  if (const int rc = tbnav::pick_device(P->device, &dev)) return rc;
  DeviceGuard guard(dev);
  if (!guard.ok) return TBNAV_ERR_NO_DEVICE;

  tbnav_rbpf* h = new (std::nothrow) tbnav_rbpf();
  if (!h) return TBNAV_ERR_INVALID_ARG;
  h->p = *P; h->device = dev; h->N = P->num_particles; h->k = P->num_samples_mode;
  h->host_threads = default_host_threads();
  h->host_affinity = host_cpu_budget(h->host_quota_cpus);
  h->xsize = xsize; h->ysize = ysize; h->words = (ysize + 63) / 64; h->radius = radius;
  h->edt_cols = edt_cols_for(xsize, h->words);
  h->G = (size_t)xsize * ysize;
  h->TW = (xsize + kTS - 1) / kTS; h->TT = h->TW * h->TW;
  h->tile_cap = tile_cap_for((double)P->range_max, P->Trs, P->resolution);
  h->df_mode = 2;  // exact query at lookup; the other modes are selected with tbnav_rbpf_set_option
  h->full_edt = false;
  // log-odds constants with the host libm, exactly as the reference's ctor (grid_mapper.cpp:42-47)
  h->l_prior = std::log(0.5 / (1 - 0.5));
  h->l_occ = std::log(0.90 / (1 - 0.90));
  h->l_free = std::log(0.35 / (1 - 0.35));
  h->cut_occ = find_occ_cut(h->l_occ, 0.90);
  h->cuts = derive_export_cuts(h->cut_occ);
  hipError_t e = hipSuccess;
  create_buffers(h, e);
  create_pool(h, max_pool_bytes, e);
  create_state(h, e);
  create_lds_attributes(h, e);
  create_mix_lut(h, e);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    const int rc = tbnav::hip_fail(e, "tbnav_rbpf_create allocation", __FILE__, __LINE__);
    tbnav_rbpf_destroy(h);
    return rc;
  }
  *out = h;
  return TBNAV_OK;
}

}  // namespace tbnav_rh

extern "C" {

int tbnav_rbpf_create(const tbnav_rbpf_params* P, tbnav_rbpf** out) { return create_impl(P, 0, out); }
int tbnav_rbpf_create_pool(const tbnav_rbpf_params* P, uint64_t max_pool_bytes, tbnav_rbpf** out) { return create_impl(P, max_pool_bytes, out); }

int tbnav_rbpf_pool_stats(tbnav_rbpf* h, uint64_t* capacity_tiles, uint64_t* free_tiles, uint64_t* tile_bytes) {
  if (!h) return TBNAV_ERR_INVALID_ARG;
  DeviceGuard guard(h->device);
  TBNAV_HIP(hipStreamSynchronize(h->stream));
  uint64_t free_now = 0;
  { const int rc = tbnav_rh::pool_free_tiles(h, &free_now); if (rc != TBNAV_OK) return rc; }
  if (capacity_tiles) *capacity_tiles = h->pool.cap - 1;  // tile 0 is the shared zero tile
  if (free_tiles) *free_tiles = free_now;
  if (tile_bytes) *tile_bytes = sizeof(double) * kTileCells;
  return TBNAV_OK;
}

void tbnav_rbpf_destroy(tbnav_rbpf* h) {
#ifdef TBNAV_PHASE_PROF
  rbpf_prof_print_propose();
  rbpf_prof_print_raycast();
#endif
  if (!h) return;
  DeviceGuard guard(h->device);
  for (int b = 0; b < 2; ++b) { (void)hipFree(h->d_state[b]); (void)hipFree(h->d_table[b]); (void)hipFree(h->d_code[b]); (void)hipFree(h->d_nocc[b]); (void)hipFree(h->d_trow[b]); }
  (void)hipFree(h->d_bm_dense); (void)hipFree(h->d_rc_dense);
  (void)hipFree(h->pool.lo); (void)hipFree(h->pool.bm); (void)hipFree(h->pool.ref); (void)hipFree(h->pool.ring); (void)hipFree(h->pool.ctr);
  (void)hipFree(h->d_sens); (void)hipFree(h->d_shed); (void)hipFree(h->d_dense); (void)hipFree(h->d_cs); (void)hipFree(h->d_touched); (void)hipFree(h->d_box_need); if (h->h_box_need) (void)hipHostFree(h->h_box_need); (void)hipFree(h->d_fstate_alt);
  (void)hipFree(h->d_log_ev); (void)hipFree(h->d_log_cnt); (void)hipFree(h->d_tile_scratch); (void)hipFree(h->d_log_pack); (void)hipFree(h->d_log_off); (void)hipFree(h->d_code_src);
  (void)hipFree(h->d_pend); (void)hipHostFree(h->h_pend); (void)hipFree(h->d_state_snap); (void)hipFree(h->d_jentries); (void)hipFree(h->d_jjobs);
  (void)hipFree(h->d_gw); (void)hipFree(h->d_gcs); (void)hipFree(h->d_gparent); (void)hipFree(h->d_gz);
  (void)hipFree(h->d_gw_raw); (void)hipFree(h->d_sendbuf); (void)hipFree(h->d_recvbuf); (void)hipFree(h->d_sizes); (void)hipFree(h->d_status);
  if (h->ev_w) (void)hipEventDestroy(h->ev_w);
  if (h->stream2) (void)hipStreamDestroy(h->stream2);
  (void)hipFree(h->d_zslot); (void)hipFree(h->d_beam_ready); (void)hipFree(h->d_beams_fg);
  (void)hipFree(h->d_beams); (void)hipFree(h->d_normals); (void)hipFree(h->d_parent); (void)hipFree(h->d_best); (void)hipFree(h->d_best_pose); (void)hipFree(h->d_export); (void)hipFree(h->d_tier); (void)hipFree(h->d_fstate); (void)hipFree(h->d_skip); (void)hipFree(h->d_win); (void)hipFree(h->d_center); (void)hipFree(h->d_mixlut); (void)hipFree(h->d_bslots); (void)hipFree(h->d_bcount); (void)hipFree(h->d_bitems); (void)hipFree(h->d_bhdr); (void)hipFree(h->d_score);
  (void)hipFree(h->d_trace);
  (void)hipHostFree(h->h_beams); (void)hipHostFree(h->h_err); (void)hipHostFree(h->h_norm); (void)hipFree(h->d_gate);
  for (auto& ev : h->ev) if (ev) (void)hipEventDestroy(ev);
  (void)hipHostFree(h->h_seq); (void)hipHostFree(h->h_beam_ring); (void)hipFree(h->d_beam_ring); (void)hipFree(h->d_norm_ring);
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h->ref;
  delete h;
}

int tbnav_rbpf_grid_size(const tbnav_rbpf* h, int32_t* xsize, int32_t* ysize) {
  if (!h || !xsize || !ysize) return TBNAV_ERR_INVALID_ARG;
  *xsize = h->xsize; *ysize = h->ysize;
  return TBNAV_OK;
}

int tbnav_rbpf_set_seed(tbnav_rbpf* h, uint64_t seed) {
  if (!h) return TBNAV_ERR_INVALID_ARG;
  h->seed = seed;
  h->scan_index = 0;
  return TBNAV_OK;
}

int tbnav_rbpf_set_rng_shard(tbnav_rbpf* h, uint64_t first_particle, uint64_t particles_global) {
  if (!h || (particles_global && particles_global < first_particle + (uint64_t)h->N)) return TBNAV_ERR_INVALID_ARG;
  h->rng_first = first_particle;
  h->rng_n_global = particles_global;
  return TBNAV_OK;
}

int tbnav_rbpf_get_normals(tbnav_rbpf* h, double* out, int64_t n) {
  if (!h || !out || n <= 0) return TBNAV_ERR_INVALID_ARG;
  DeviceGuard guard(h->device);
  TBNAV_HIP(hipStreamSynchronize(h->stream));
  if (h->last_drawn.valid) {
    // the last scan drew its noise inside the proposal kernel and stored none of it: the same counters through rbpf_sample_normals
    // give the same values (one definition: normal_pair) — what the kernel used, regenerated for whoever asks
    if ((size_t)n > h->last_drawn.n) return TBNAV_ERR_INVALID_ARG;
    const size_t nn = h->last_drawn.n;
    if (nn > h->normals_cap) {
      (void)hipFree(h->d_normals); h->d_normals = nullptr; h->normals_cap = 0;
      TBNAV_HIP(hipMalloc((void**)&h->d_normals, sizeof(double) * nn));
      h->normals_cap = nn;
    }
    const bool sharded = h->last_drawn.z_index != nn - 1 || h->last_drawn.base != 0;
    TBNAV_TRY(launch_sample_normals(h, nn, h->last_drawn.seed, h->last_drawn.scan, sharded, h->last_drawn.base, h->last_drawn.z_index,
                                    nullptr, nullptr, 0));
    TBNAV_HIP(hipStreamSynchronize(h->stream));
    TBNAV_HIP(hipMemcpy(out, h->d_normals, sizeof(double) * n, hipMemcpyDeviceToHost));
    return TBNAV_OK;
  }
  if ((size_t)n > std::max(h->normals_cap, h->norm_ring_stride)) return TBNAV_ERR_INVALID_ARG;
  TBNAV_HIP(hipMemcpy(out, h->last_normals ? h->last_normals : h->d_normals, sizeof(double) * n, hipMemcpyDeviceToHost));
  return TBNAV_OK;
}

int64_t tbnav_rbpf_num_normals(const tbnav_rbpf* h, int32_t icp_ok) {
  if (!h) return -1;
  return (int64_t)h->N * (icp_ok ? 3 * h->k + 3 : 3) + 1;
}

int tbnav_rbpf_slam(tbnav_rbpf* h, const float* scan, int32_t n_beams, const double u[3], const double cur_odom[3],
                    const double prev_odom[3], int32_t icp_ok, const double T_icp[3], const double* normals,
                    tbnav_rbpf_stats* out) {
  return slam_impl(h, scan, n_beams, u, cur_odom, prev_odom, icp_ok, T_icp, normals, out, false);
}

}  // extern "C"

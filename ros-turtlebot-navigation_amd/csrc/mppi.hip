// mppi.hip — MI355X (gfx950) implementation of controller::MPPI::newControls behind the C-ABI of include/tbnav_mppi.h: the handle,
// the launchers and the single-GPU entry points.  Which kernel a (K, T) takes and which instantiation a tick launches is decided in
// mppi_plan.hpp (plain arithmetic, no HIP); the launchers here fill its inputs from the handle, launch what comes back, update the
// handle.  Reference: controller/src/controller/mppi.cpp:72-140, rk4.cpp:49-115, controller/include/controller/mppi.hpp:41-105
// (paths relative to the reference tree).
// Kernels: mppi_rollout.hip (four rollout families), mppi_softmin.hip (records, combine, exchange words, noise) over mppi_device.hpp;
// the cost field: mppi_field.hip; communicator attachment, the sharded tick and groups: mppi_sharded.hip; the handle: mppi_host.hpp.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <atomic>
#include <chrono>
#include <new>
#include <type_traits>
#include <vector>

#include "mppi_host.hpp"

using namespace tbnav_mh;

namespace tbnav_mh {
Lam lam_of(double lambda) {
  const double inv = 1.0 / lambda;
  unsigned long long bits; std::memcpy(&bits, &lambda, sizeof bits);
  const bool all_ones = (bits & 0xFFFFFFFFFFFFFull) == 0xFFFFFFFFFFFFFull;   // the one significand Markstein's theorem excludes
  return Lam{lambda, (std::isnormal(inv) && std::isnormal(lambda) && !all_ones) ? inv : 0.0};
}
}  // namespace tbnav_mh

namespace {
using TickGraph = tbnav_mppi::TickGraph;
void drop_graph(TickGraph& g) {
  if (g.exec) { (void)hipGraphExecDestroy(g.exec); g.exec = nullptr; }
  if (g.graph) { (void)hipGraphDestroy(g.graph); g.graph = nullptr; }
}

// the publication the sharded tick has asked for, taken over by the launch that can carry it out (see pub_pending)
DirectPub take_pub(tbnav_mppi* h) {
  if (!h->pub_pending) return DirectPub{nullptr, 0, 0, 0, 0u, 0};
  h->pub_pending = false;
  return h->pub_next;
}

RolloutArgs rollout_args(const tbnav_mppi* h, const double x0[3]) {
  RolloutArgs a;
  a.half_r = h->p.wheel_radius / 2.0;
  a.r_over_b = h->p.wheel_radius / h->p.wheel_base;
  a.r_d = h->p.wheel_radius * (1 / h->p.wheel_base);
  a.h = h->p.dt;
  a.h6 = h->p.dt / 6.0;
  for (int c = 0; c < 3; ++c) { a.x0[c] = x0[c]; a.xd[c] = h->xd[c]; a.Q[c] = h->p.Q[c]; a.P1[c] = h->p.P1[c]; }
  a.R[0] = h->p.R[0]; a.R[1] = h->p.R[1];
  a.T = h->T; a.K = h->K;
  a.lds_from = 0;
  return a;
}

// the rollout kernel of the three-kernel tick: plan_rollout names the form, the family's list gives the instantiation
int launch_rollout(tbnav_mppi* h, const double x0[3], const double* d_duL, const double* d_duR, hipStream_t st) {
  const RolloutPlan p = plan_rollout(RolloutIn{h->T, h->K, h->dyn, h->trig, h->scan_tc, h->prefix_rg, h->lds_from, h->field_on});
  RolloutArgs a = rollout_args(h, x0);
  a.lds_from = p.lds_from;
  const USrc usrc = usrc_of(h);
  const dim3 grid(p.grid), block(kWave, p.block_y);
  const KernelForm& f = p.form;
  auto launched = [&]() {
    TBNAV_HIP(hipGetLastError());
    h->lk_rollout = f;
    h->j_valid = true;
    h->prefix_rows = p.prefix_rows;
    return (int)TBNAV_OK;
  };
  if (f.family == kField) { const int rc = launch_rollout_field(h, p, a, usrc, d_duL, d_duR, st); return rc != TBNAV_OK ? rc : launched(); }
#define TBNAV_X(TR, TC, MW) if (f.is(kScan, TR, TC, MW)) { hipLaunchKernelGGL((mppi_rollout_scan<TR, TC, MW>), grid, block, p.lds, st, a, d_duL, d_duR, usrc, h->d_J); return launched(); }
  TBNAV_MPPI_SCAN_FORMS(TBNAV_X)
#undef TBNAV_X
#define TBNAV_X(RG) if (f.is(kPrefix, RG)) { hipLaunchKernelGGL((mppi_rollout_prefix<RG>), grid, block, p.lds, st, a, d_duL, d_duR, usrc, h->d_J, h->d_total); return launched(); }
  TBNAV_MPPI_PREFIX_FORMS(TBNAV_X)
#undef TBNAV_X
#define TBNAV_X(TR) if (f.is(kCost, TR)) { hipLaunchKernelGGL((mppi_rollout_cost<TR>), grid, block, p.lds, st, a, d_duL, d_duR, usrc, h->d_J); return launched(); }
  TBNAV_MPPI_COST_FORMS(TBNAV_X)
#undef TBNAV_X
  return TBNAV_ERR_UNSUPPORTED;  // (a form the plan names and the list does not have: never another form in its place)
}

// rollout + partial records in one launch (small K); the caller follows with launch_combine(..., fused_S)
int launch_fused(tbnav_mppi* h, const double x0[3], const double* d_duL, const double* d_duR, hipStream_t st,
                 const RngArgs* rng = nullptr) {
  const FusedPlan p = plan_fused(FusedIn{h->T, h->K, h->dyn, h->trig, h->sampler, h->fused_r, h->fused_S, rng != nullptr});
  const RolloutArgs a = rollout_args(h, x0);
  const USrc usrc = usrc_of(h);
  const RngArgs g = rng ? *rng : RngArgs{0, 0, 0.0, 0.0};
  auto launched = [&]() {
    TBNAV_HIP(hipGetLastError());
    h->lk_rollout = p.form;
    h->j_valid = h->keep_j;
    h->prefix_rows = 0;
    return (int)TBNAV_OK;
  };
#define TBNAV_X(TR, RR, TL, RG)                                                                                                                       \
  if (p.form.is(kFused, TR, RR, TL, RG)) {                                                                                                            \
    hipLaunchKernelGGL((mppi_rollout_fused<TR, RR, TL, RG>), dim3(p.grid), dim3(p.block), p.lds, st, usrc.p, (const double*)g.ahead,                  \
                       (const uint64_t*)g.ahead_tag, g.tick0, usrc.shift, h->T, h->K, h->fused_S, h->d_records_f, h->keep_j ? h->d_J : nullptr, a,    \
                       usrc.init_l, usrc.init_r, lam_of(h), d_duL, d_duR, rng_rest(g));                                                               \
    return launched();                                                                                                                                \
  }
  TBNAV_MPPI_FUSED_FORMS(TBNAV_X)
#undef TBNAV_X
  return TBNAV_ERR_UNSUPPORTED;  // (a form the plan names and the list does not have)
}

int launch_partials(tbnav_mppi* h, const double* d_duL, const double* d_duR, double* d_records, hipStream_t st) {
  const dim3 grid(h->S, h->T), block(kSliceThreads);
  hipLaunchKernelGGL(mppi_partials, grid, block, 0, st, h->T, h->K, h->S, lam_of(h), h->d_J, d_duL, d_duR, d_records, h->prefix_rows, h->d_total);
  TBNAV_HIP(hipGetLastError());
  return TBNAV_OK;
}

}  // namespace
int tbnav_mh::launch_combine(tbnav_mppi* h, const double* d_records, int G, hipStream_t st, int S, const DirectSrc* direct,
                             const RngArgs* next) {
  if (S < 0) S = h->S;
  const USrc usrc = usrc_of(h);
  // (records that came through an all-gather: only the error words — a poisoned record raises them, see mppi_combine)
  const DirectSrc ds = direct ? *direct : DirectSrc{nullptr, 0ull, (G > 1 && h->comm) ? h->d_dx_err : nullptr, (G > 1 && h->comm) ? h->d_dx_dead : nullptr, 0u};
  // noise ahead (the one-group form only): sampler blocks behind the time steps' blocks
  const RngArgs off{0, 0, 0.0, 0.0};
  const RngArgs nx = next ? *next : off;
  const CombinePlan p = plan_combine(h->T, h->K, G, S, direct != nullptr, ds.err != nullptr, h->wide_combine, nx.ahead != nullptr);
  double* const out_host = h->publish_next ? h->d_out_host : nullptr;
  const double seq = (double)(h->seq + 1);
  auto launched = [&]() {
    TBNAV_HIP(hipGetLastError());
    h->lk_combine = p.form;
    h->lk_records = direct ? nullptr : d_records; h->lk_S = S; h->lk_G = G; h->lk_ushift = usrc.shift;
    ++h->seq;
    if (h->publish_next) h->published = h->seq;
    h->ucur = 1 - h->ucur;       // the freshly written vector is current ...
    h->pending_shift = true;     // ... and its shift is still owed
    return (int)TBNAV_OK;
  };
  if (p.form.family == kCombineWide) {
    hipLaunchKernelGGL(mppi_combine_wide, dim3(p.grid), dim3(p.block), 0, st, h->T, S, lam_of(h), h->p.max_wheel_vel, usrc, d_records, h->d_u[1 - h->ucur], h->d_out,
                       out_host, seq);
    return launched();
  }
#define TBNAV_X(KEEP, MODE)                                                                                                                           \
  if (p.form.is(kCombine, KEEP, MODE)) {                                                                                                              \
    hipLaunchKernelGGL((mppi_combine<KEEP, MODE>), dim3(p.grid), dim3(p.block), 0, st, d_records, usrc.p, MODE == 0 ? nx.ahead : nullptr,             \
                       MODE == 0 ? nx.tick0 : nullptr, h->T, S, usrc.shift, p.blocks, G, p.tpr_log2, MODE == 0 ? nx.ahead_tag : nullptr, lam_of(h),   \
                       h->p.max_wheel_vel, usrc.init_l, usrc.init_r, h->d_u[1 - h->ucur], h->d_out, out_host, seq, ds, rng_rest(MODE == 0 ? nx : off)); \
    return launched();                                                                                                                                \
  }
  TBNAV_MPPI_COMBINE_FORMS(TBNAV_X)
#undef TBNAV_X
  return TBNAV_ERR_UNSUPPORTED;  // (a form the plan names and the list does not have)
}
namespace {

// Apply an owed shift for real (host side; only the state accessors need the materialised vector).
int materialize_controls(tbnav_mppi* h, double* u_host /*[2][T], may be null*/) {
  const int T = h->T;
  std::vector<double> tmp((size_t)2 * T);
  TBNAV_HIP(hipDeviceSynchronize());
  TBNAV_HIP(hipMemcpy(tmp.data(), h->d_u[h->ucur], sizeof(double) * 2 * T, hipMemcpyDeviceToHost));
  if (h->pending_shift) {
    for (int i = 0; i + 1 < T; ++i) { tmp[i] = tmp[i + 1]; tmp[T + i] = tmp[T + i + 1]; }
    tmp[T - 1] = h->uinit[0];
    tmp[2 * T - 1] = h->uinit[1];
    TBNAV_HIP(hipMemcpy(h->d_u[h->ucur], tmp.data(), sizeof(double) * 2 * T, hipMemcpyHostToDevice));
    h->pending_shift = false;
  }
  if (u_host) std::memcpy(u_host, tmp.data(), sizeof(double) * 2 * T);
  return TBNAV_OK;
}

// counter of rollout 0, step 0 of this handle at tick `tick`: counter(k, i) = tick*T*K_global + (k0 + k)*T + i, so the
// shards of one ensemble draw disjoint perturbations from one seed (and the same ones as the unsharded ensemble)
uint64_t rng_base(const tbnav_mppi* h, uint64_t tick) { return tick * (uint64_t)h->T * h->k_global + h->k0 * (uint64_t)h->T; }

bool pick_noise(tbnav_mppi* h, const double*& d_duL, const double*& d_duR) {
  if (!d_duL && !d_duR) { d_duL = h->d_duL; d_duR = h->d_duR; return true; }
  return d_duL && d_duR;
}

// the plan's predicates on this handle (a handle with a cost field takes neither the fused kernel nor the noise-ahead draw)
bool rng_in_kernel(const tbnav_mppi* h) { return tbnav_mk::rng_in_kernel(fused_rng(h), h->fused_r); }
bool ahead_wanted(const tbnav_mppi* h) { return tbnav_mk::ahead_wanted(h->fused_rng, h->fused_r); }
bool ahead_on(const tbnav_mppi* h) { return h->noise_ahead && h->d_ahead && ahead_wanted(h) && !h->comm; }
// the device noise source of tick `tick` under `seed` ...
RngArgs rng_args(const tbnav_mppi* h, uint64_t seed, uint64_t tick) { return RngArgs{seed, rng_base(h, tick), std::sqrt(h->p.ul_var), std::sqrt(h->p.ur_var)}; }
// ... and with the noise-ahead fields: the pair buffer, its tag and what a tag must say to be this launch's
RngArgs with_ahead(const tbnav_mppi* h, RngArgs g) {
  g.ahead = h->d_ahead; g.ahead_tag = h->d_ahead_tag; g.epoch = h->cfg_epoch; g.kind = h->sampler == 1 ? 2 : 1; g.K = h->K;
  return g;
}
// (re)allocate the pair buffer and its tag for the handle's kernel choice; a fresh tag matches no tick
hipError_t ahead_alloc(tbnav_mppi* h) {
  (void)hipFree(h->d_ahead); (void)hipFree(h->d_ahead_tag);
  h->d_ahead = nullptr; h->d_ahead_tag = nullptr;
  if (!ahead_wanted(h)) return hipSuccess;
  hipError_t e = hipMalloc((void**)&h->d_ahead, (size_t)2 * h->T * h->K * sizeof(double));
  if (e == hipSuccess) e = hipMalloc((void**)&h->d_ahead_tag, kTagWords * sizeof(uint64_t));
  if (e == hipSuccess) e = hipMemset(h->d_ahead_tag, 0xFF, kTagWords * sizeof(uint64_t));
  return e;
}

// One device-noise tick on the fused kernel: with noise ahead, the fused kernel takes its pairs from the buffer when the tag is
// its own and the combine draws the next tick's (the tick after `g`: the counters of one tick further on, same tick0 word)
int rng_tick(tbnav_mppi* h, const double x0[3], RngArgs g, hipStream_t st) {
  const bool ahead = ahead_on(h);
  if (ahead) g = with_ahead(h, g);
  const int rc = launch_fused(h, x0, h->d_duL, h->d_duR, st, &g);
  if (rc != TBNAV_OK) return rc;
  RngArgs nx = g;
  nx.base += (uint64_t)h->T * h->k_global;
  return launch_combine(h, h->d_records_f, 1, st, h->fused_S, nullptr, ahead ? &nx : nullptr);
}

// the fused kernel's fine records folded into the K-slice records that the ranks exchange (published by the kernel itself when the
// sharded tick has asked for it)
int launch_merge(tbnav_mppi* h, double* d_records_out, hipStream_t st) {
  hipLaunchKernelGGL(mppi_merge_records, dim3(h->S, h->T), dim3(kWave), 0, st, h->T, h->fused_S, kSlice / h->fused_r, h->S,
                     lam_of(h), h->d_records_f, d_records_out, take_pub(h));
  TBNAV_HIP(hipGetLastError());
  return TBNAV_OK;
}

// `launch(r)`, r = 0 .. reps-1, back to back between ONE pair of events; ms[which] = the mean.  Nothing runs once rc is an error.
template <class Launch>
void timed(hipEvent_t (&ev)[2], hipStream_t st, int reps, float* ms, int which, int& rc, Launch&& launch) {
  if (rc != TBNAV_OK) return;
  if (hipEventRecord(ev[0], st) != hipSuccess) { rc = TBNAV_ERR_HIP; return; }
  for (int r = 0; r < reps && rc == TBNAV_OK; ++r) rc = launch(r);
  if (rc != TBNAV_OK) return;
  float t = 0.f;
  if (hipEventRecord(ev[1], st) != hipSuccess || hipEventSynchronize(ev[1]) != hipSuccess ||
      hipEventElapsedTime(&t, ev[0], ev[1]) != hipSuccess) { rc = TBNAV_ERR_HIP; return; }
  ms[which] = t / (float)reps;
}

}  // namespace

extern "C" {

int tbnav_mppi_create(const tbnav_mppi_params* params, tbnav_mppi** out) {
  if (!params || !out) return TBNAV_ERR_INVALID_ARG;
  *out = nullptr;
  if (params->rollouts <= 0 || !(params->dt > 0.0) || !(params->horizon > 0.0) ||
      !(params->lambda > 0.0) || !(params->wheel_base != 0.0))
    return TBNAV_ERR_INVALID_ARG;
  const int T = static_cast<int>(params->horizon / params->dt);  // mppi.cpp:47
  if (T <= 0) return TBNAV_ERR_INVALID_ARG;
  int dev = 0;
  if (const int rc = tbnav::pick_device(params->device, &dev)) return rc;
  DeviceGuard guard(dev);
  if (!guard.ok) return TBNAV_ERR_NO_DEVICE;

  tbnav_mppi* h = new (std::nothrow) tbnav_mppi();
  if (!h) return TBNAV_ERR_INVALID_ARG;
  h->p = *params;
  h->T = T;
  h->K = params->rollouts;
  h->device = dev;
  {
    // which kernel this (K, T) takes on this chip: mppi_plan.hpp (plan_create: the rules, the measurements behind them)
    hipDeviceProp_t prop;
    int cus = 256;
    if (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) cus = prop.multiProcessorCount;
    const CreatePlan c = plan_create(h->K, T, cus);
    h->S = c.S; h->lds_from = c.lds_from; h->prefix_rg = c.prefix_rg; h->scan_tc = c.scan_tc;
    h->fused_dev = c.fused_dev; h->fused_rng = c.fused_rng; h->fused_r = c.fused_r; h->fused_S = c.fused_S;
  }
  h->k_global = (uint64_t)h->K;
  const size_t tk = (size_t)T * h->K;
  hipError_t e = hipSuccess;
  auto alloc = [&](double** p, size_t n) { if (e == hipSuccess) e = hipMalloc((void**)p, n * sizeof(double)); };
  alloc(&h->d_u[0], 2 * (size_t)T);
  alloc(&h->d_u[1], 2 * (size_t)T);
  alloc(&h->d_J, tk);
  alloc(&h->d_duL, tk);
  alloc(&h->d_duR, tk);
  alloc(&h->d_records, (size_t)T * h->S * TBNAV_MPPI_REC);
  if (h->prefix_rg) alloc(&h->d_total, (size_t)h->K);
  if (h->fused_r) alloc(&h->d_records_f, (size_t)T * h->fused_S * TBNAV_MPPI_REC);
  if (e == hipSuccess) e = ahead_alloc(h);
  alloc(&h->d_out, 2);
  if (e == hipSuccess) e = hipMemset(h->d_out, 0, 2 * sizeof(double));
  if (e == hipSuccess) e = hipHostMalloc((void**)&h->h_out, 4 * sizeof(double), hipHostMallocMapped);
  if (e == hipSuccess) { for (int q = 0; q < 4; ++q) h->h_out[q] = 0.0; e = hipHostGetDevicePointer((void**)&h->d_out_host, h->h_out, 0); }
  if (e == hipSuccess) e = hipMemset(h->d_u[0], 0, 2 * (size_t)T * sizeof(double));
  if (e == hipSuccess) e = hipMemset(h->d_u[1], 0, 2 * (size_t)T * sizeof(double));
  if (e == hipSuccess) e = hipMemset(h->d_J, 0, tk * sizeof(double));
  if (e == hipSuccess) e = hipMemset(h->d_duL, 0, tk * sizeof(double));
  if (e == hipSuccess) e = hipMemset(h->d_duR, 0, tk * sizeof(double));
  // dynamic LDS beyond the 64 KB default for every form of the sequential kernel (lds_from only ever grows afterwards)
  const int lds_max = (int)staged_lds_bytes(T, h->lds_from);
#define TBNAV_X(TR) if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(&mppi_rollout_cost<TR>), hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
  TBNAV_MPPI_COST_FORMS(TBNAV_X)
#undef TBNAV_X
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    const int rc = tbnav::hip_fail(e, "tbnav_mppi_create allocation", __FILE__, __LINE__);
    tbnav_mppi_destroy(h);
    return rc;
  }
  *out = h;
  return TBNAV_OK;
}

void tbnav_mppi_destroy(tbnav_mppi* h) {
  if (!h) return;
  DeviceGuard guard(h->device);
  // A handle that is still attached detaches first — for a multi-process direct exchange that is COLLECTIVE (every rank's destroy or
  // detach meets in tbnav_mppi_attach_comm: a peer one tick ahead may still be storing into this rank's buffer; round-4 advisor
  // finding: the buffer used to be freed here without the rendezvous) — so the communicator must still be alive: destroy handles
  // before their communicators, or detach explicitly first.
  if (h->comm) (void)tbnav_mppi_attach_comm(h, nullptr);
  (void)hipDeviceSynchronize();
  (void)hipFree(h->d_u[0]); (void)hipFree(h->d_u[1]); (void)hipFree(h->d_J); (void)hipFree(h->d_duL); (void)hipFree(h->d_duR);
  (void)hipFree(h->d_total); (void)hipFree(h->d_records_all);
  direct_teardown(h);
  exchange_words_free(h);
  (void)hipFree(h->d_raw); (void)hipFree(h->d_records); (void)hipFree(h->d_records_f); (void)hipFree(h->d_out);
  (void)hipFree(h->d_ahead); (void)hipFree(h->d_ahead_tag); (void)hipFree(h->d_field);
  if (h->h_out) (void)hipHostFree(h->h_out);
  drop_graph(h->tg); drop_graph(h->tgs);
  (void)hipFree(h->d_tick0);
  delete h;
}

int tbnav_mppi_steps(const tbnav_mppi* h) { return h ? h->T : -1; }
int tbnav_mppi_set_dynamics(tbnav_mppi* h, int32_t model) {
  if (!h || (model != TBNAV_MPPI_DYN_RK4 && model != TBNAV_MPPI_DYN_ARC)) return TBNAV_ERR_INVALID_ARG;
  h->dyn = model;
  ++h->cfg_epoch;
  return TBNAV_OK;
}

int tbnav_mppi_set_option(tbnav_mppi* h, int32_t option, int32_t value) {
  if (!h) return TBNAV_ERR_INVALID_ARG;
  DeviceGuard guard(h->device);
  const int T = h->T;
  ++h->cfg_epoch;  // (any option may change what a captured graph of ticks has baked in)
  switch (option) {
    case TBNAV_MPPI_OPT_KEEP_J: h->keep_j = value != 0; return TBNAV_OK;
    case TBNAV_MPPI_OPT_TRIG:
      if (value < 1 || value > 3) return TBNAV_ERR_INVALID_ARG;
      h->trig = value;
      return TBNAV_OK;
    case TBNAV_MPPI_OPT_NO_LDS_STAGING:
      if (value) { h->lds_from = T; h->prefix_rg = 0; }
      return TBNAV_OK;
    case TBNAV_MPPI_OPT_REG_TAIL:   // (the round-2 kernel this switched is gone — mppi_rollout_prefix superseded it; accepted and ignored)
      return TBNAV_OK;
    case TBNAV_MPPI_OPT_PREFIX_FORM:
      if (!value) h->prefix_rg = 0;
      return TBNAV_OK;
    case TBNAV_MPPI_OPT_BATCH_GRAPH:
      h->graph_on = value != 0;
      return TBNAV_OK;
    case TBNAV_MPPI_OPT_DIRECT_EXCHANGE:  // (takes effect at the next tbnav_mppi_attach_comm)
      h->direct_want = value != 0;
      h->dx_withhold = value == 2;                       // (tests of the bound: see dx_withhold)
      h->dx_budget = value == 2 ? 30000000ull : 200000000ull;  // 0.3 s there
      return TBNAV_OK;
    case TBNAV_MPPI_OPT_FAULT_INJECT:   // (tests) the next sharded tick's local half reports a failure; 0 takes it back
      h->fail_next = value != 0;
      return TBNAV_OK;
    case TBNAV_MPPI_OPT_WIDE_COMBINE:   // 0: always the one-wave-per-step combine (A-B); default 1
      h->wide_combine = value != 0;
      return TBNAV_OK;
    case TBNAV_MPPI_OPT_SAMPLER:        // 1 (default): fp64 Box-Muller on 52-bit uniforms (utilities.cpp:20-24's width); 0: fp32 on 24-bit uniforms
      if (value != 0 && value != 1) return TBNAV_ERR_INVALID_ARG;
      h->sampler = value;
      return TBNAV_OK;
    case TBNAV_MPPI_OPT_NOISE_AHEAD:    // 1 (default): a device-noise tick's combine draws the next tick's perturbations; 0: the fused kernel draws its own
      if (value != 0 && value != 1) return TBNAV_ERR_INVALID_ARG;
      h->noise_ahead = value != 0;
      return TBNAV_OK;
    case TBNAV_MPPI_OPT_KERNEL: {
      // 0: mppi_rollout_cost (sequential); n > 0: mppi_rollout_scan with n steps per thread; -4 / -8 / -16: fused, that many rollouts per workgroup
      const KernelOption o = plan_kernel_option(T, h->K, value);   // (which values a horizon admits: mppi_plan.hpp)
      if (!o.ok) return TBNAV_ERR_INVALID_ARG;
      h->scan_tc = o.scan_tc; h->fused_r = o.fused_r; h->fused_dev = o.fused_dev; h->fused_rng = o.fused_rng; h->fused_S = o.fused_S;
      (void)hipFree(h->d_records_f);
      h->d_records_f = nullptr;
      if (o.fused_r) TBNAV_HIP(hipMalloc((void**)&h->d_records_f, sizeof(double) * (size_t)T * h->fused_S * TBNAV_MPPI_REC));
      TBNAV_HIP(hipDeviceSynchronize());   // (a queued tick may still read the old pair buffer)
      TBNAV_HIP(ahead_alloc(h));
      return TBNAV_OK;
    }
    default: return TBNAV_ERR_INVALID_ARG;
  }
}

int tbnav_mppi_set_rng_shard(tbnav_mppi* h, uint64_t first_rollout, uint64_t rollouts_global) {
  if (!h || rollouts_global < first_rollout + (uint64_t)h->K) return TBNAV_ERR_INVALID_ARG;
  h->k0 = first_rollout;
  h->k_global = rollouts_global;
  ++h->cfg_epoch;
  return TBNAV_OK;
}

int tbnav_mppi_rollout_variant(const tbnav_mppi* h) { return h ? (h->fused_dev ? -h->fused_r : h->scan_tc) : 0; }
int tbnav_mppi_streaming_form(const tbnav_mppi* h) {
  if (!h) return -1;
  return (h->dyn == 0 && h->trig == 1 && h->prefix_rg > 0) ? 2 : 0;
}
int64_t tbnav_mppi_graph_replayed_ticks(const tbnav_mppi* h) { return h ? (int64_t)h->graph_ticks : -1; }
int tbnav_mppi_rollouts(const tbnav_mppi* h) { return h ? h->K : -1; }
int tbnav_mppi_records_per_step(const tbnav_mppi* h) { return h ? h->S : -1; }

int tbnav_mppi_set_initial_controls(tbnav_mppi* h, double uL, double uR) {
  if (!h) return TBNAV_ERR_INVALID_ARG;
  DeviceGuard guard(h->device);
  h->uinit[0] = uL; h->uinit[1] = uR;
  ++h->cfg_epoch;
  double* tmp = new (std::nothrow) double[2 * (size_t)h->T];
  if (!tmp) return TBNAV_ERR_INVALID_ARG;
  for (int i = 0; i < h->T; ++i) { tmp[i] = uL; tmp[h->T + i] = uR; }
  hipError_t e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(h->d_u[h->ucur], tmp, 2 * (size_t)h->T * sizeof(double), hipMemcpyHostToDevice);
  h->pending_shift = false;
  delete[] tmp;
  TBNAV_HIP(e);
  return TBNAV_OK;
}

int tbnav_mppi_set_waypoint(tbnav_mppi* h, double x, double y, double theta) {
  if (!h) return TBNAV_ERR_INVALID_ARG;
  h->xd[0] = x; h->xd[1] = y; h->xd[2] = theta;
  ++h->cfg_epoch;
  return TBNAV_OK;
}

int tbnav_mppi_get_controls(tbnav_mppi* h, double* u_host) {
  if (!h || !u_host) return TBNAV_ERR_INVALID_ARG;
  DeviceGuard guard(h->device);
  return materialize_controls(h, u_host);
}

int tbnav_mppi_set_controls(tbnav_mppi* h, const double* u_host) {
  if (!h || !u_host) return TBNAV_ERR_INVALID_ARG;
  DeviceGuard guard(h->device);
  TBNAV_HIP(hipDeviceSynchronize());
  TBNAV_HIP(hipMemcpy(h->d_u[h->ucur], u_host, 2 * (size_t)h->T * sizeof(double), hipMemcpyHostToDevice));
  h->pending_shift = false;
  return TBNAV_OK;
}

int tbnav_mppi_shard_partials(tbnav_mppi* h, const double x0[3], const double* d_duL,
                              const double* d_duR, void* stream, double* d_records_out) {
  if (!h || !x0 || !d_records_out || !pick_noise(h, d_duL, d_duR)) return TBNAV_ERR_INVALID_ARG;
  DeviceGuard guard(h->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (fused_dev(h) && kSlice % h->fused_r == 0) {
    // small K: the fused rollout+partials kernel, then its fine records folded into the K-slice records that the
    // ranks exchange (two short launches instead of three)
    const int rcf = launch_fused(h, x0, d_duL, d_duR, st);
    return rcf != TBNAV_OK ? rcf : launch_merge(h, d_records_out, st);
  }
  int rc = launch_rollout(h, x0, d_duL, d_duR, st);
  if (rc != TBNAV_OK) return rc;
  return launch_partials(h, d_duL, d_duR, d_records_out, st);
}

// Same, with this shard's perturbations drawn on the device (tbnav_mppi_set_rng_shard gives the shard its place in
// the ensemble's counter space): inside the fused kernel when that is the handle's kernel, else sampled first.
int tbnav_mppi_shard_partials_rng(tbnav_mppi* h, const double x0[3], uint64_t seed, uint64_t tick, void* stream, double* d_records_out) {
  if (!h || !x0 || !d_records_out) return TBNAV_ERR_INVALID_ARG;
  if (!(rng_in_kernel(h) && kSlice % h->fused_r == 0)) {
    const int rc = tbnav_mppi_sample_noise(h, seed, tick, stream);
    return rc != TBNAV_OK ? rc : tbnav_mppi_shard_partials(h, x0, nullptr, nullptr, stream, d_records_out);
  }
  DeviceGuard guard(h->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const RngArgs g = rng_args(h, seed, tick);
  const int rcf = launch_fused(h, x0, h->d_duL, h->d_duR, st, &g);
  return rcf != TBNAV_OK ? rcf : launch_merge(h, d_records_out, st);
}

int tbnav_mppi_shard_combine(tbnav_mppi* h, const double* d_records_all, int32_t n_shards, void* stream) {
  if (!h || !d_records_all || n_shards <= 0) return TBNAV_ERR_INVALID_ARG;
  DeviceGuard guard(h->device);
  return launch_combine(h, d_records_all, n_shards, static_cast<hipStream_t>(stream));
}

int tbnav_mppi_enqueue_dev(tbnav_mppi* h, const double x0[3], const double* d_duL,
                           const double* d_duR, void* stream) {
  if (!h || !x0 || !pick_noise(h, d_duL, d_duR)) return TBNAV_ERR_INVALID_ARG;
  if (h->comm) return sharded_tick(h, x0, d_duL, d_duR, nullptr, 0, stream);
  DeviceGuard guard(h->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (fused_dev(h)) {
    const int rcf = launch_fused(h, x0, d_duL, d_duR, st);
    if (rcf != TBNAV_OK) return rcf;
    return launch_combine(h, h->d_records_f, 1, st, h->fused_S);
  }
  int rc = launch_rollout(h, x0, d_duL, d_duR, st);
  if (rc != TBNAV_OK) return rc;
  // (fusing the combine into the partials kernel's last workgroup was measured and rejected: DESIGN.md section 4)
  rc = launch_partials(h, d_duL, d_duR, h->d_records, st);
  if (rc != TBNAV_OK) return rc;
  return launch_combine(h, h->d_records, 1, st);
}

int tbnav_mppi_profile_tick(tbnav_mppi* h, const double x0[3], const double* d_duL,
                            const double* d_duR, void* stream, float ms[TBNAV_MPPI_NKERNELS]) {
  if (!h || !x0 || !ms || !pick_noise(h, d_duL, d_duR)) return TBNAV_ERR_INVALID_ARG;
  DeviceGuard guard(h->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipEvent_t ev[TBNAV_MPPI_NKERNELS + 1];
  for (auto& e : ev) TBNAV_HIP(hipEventCreate(&e));
  int rc = TBNAV_OK;
  TBNAV_HIP(hipEventRecord(ev[0], st));
  if (fused_dev(h)) {  // rollout and partials are one kernel: its time is reported under [0], [1] is the empty interval
    rc = launch_fused(h, x0, d_duL, d_duR, st);
    if (rc == TBNAV_OK) { TBNAV_HIP(hipEventRecord(ev[1], st)); TBNAV_HIP(hipEventRecord(ev[2], st)); rc = launch_combine(h, h->d_records_f, 1, st, h->fused_S); }
  } else {
    rc = launch_rollout(h, x0, d_duL, d_duR, st);
    if (rc == TBNAV_OK) { TBNAV_HIP(hipEventRecord(ev[1], st)); rc = launch_partials(h, d_duL, d_duR, h->d_records, st); }
    if (rc == TBNAV_OK) { TBNAV_HIP(hipEventRecord(ev[2], st)); rc = launch_combine(h, h->d_records, 1, st); }
  }
  if (rc == TBNAV_OK) {
    TBNAV_HIP(hipEventRecord(ev[3], st));
    TBNAV_HIP(hipEventSynchronize(ev[3]));
    for (int i = 0; i < TBNAV_MPPI_NKERNELS; ++i) TBNAV_HIP(hipEventElapsedTime(&ms[i], ev[i], ev[i + 1]));
  }
  for (auto& e : ev) (void)hipEventDestroy(e);
  return rc;
}


// Per-kernel durations without the event overhead: every kernel of the tick is launched `reps` times back to back
// between ONE pair of events (a single launch of a 5 us kernel between two events measures the events as much as
// the kernel).  The controller state advances as if `reps` ticks had run on the same inputs.
int tbnav_mppi_profile_kernels(tbnav_mppi* h, const double x0[3], const double* d_duL, const double* d_duR, void* stream,
                               int32_t reps, float ms[TBNAV_MPPI_NKERNELS]) {
  if (!h || !x0 || !ms || reps < 2 || (reps & 1) || !pick_noise(h, d_duL, d_duR)) return TBNAV_ERR_INVALID_ARG;
  DeviceGuard guard(h->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipEvent_t ev[2];
  for (auto& e : ev) TBNAV_HIP(hipEventCreate(&e));
  int rc = TBNAV_OK;
  for (int i = 0; i < TBNAV_MPPI_NKERNELS; ++i) ms[i] = 0.f;
  if (fused_dev(h)) {
    timed(ev, st, reps, ms, 0, rc, [&](int) { return launch_fused(h, x0, d_duL, d_duR, st); });
    timed(ev, st, reps, ms, 2, rc, [&](int) { return launch_combine(h, h->d_records_f, 1, st, h->fused_S); });
  } else {
    timed(ev, st, reps, ms, 0, rc, [&](int) { return launch_rollout(h, x0, d_duL, d_duR, st); });
    timed(ev, st, reps, ms, 1, rc, [&](int) { return launch_partials(h, d_duL, d_duR, h->d_records, st); });
    timed(ev, st, reps, ms, 2, rc, [&](int) { return launch_combine(h, h->d_records, 1, st); });
  }
  for (auto& e : ev) (void)hipEventDestroy(e);
  return rc;
}

int tbnav_mppi_profile_kernels_rng(tbnav_mppi* h, const double x0[3], uint64_t seed, uint64_t tick, void* stream, int32_t reps,
                                   float ms[TBNAV_MPPI_NKERNELS]) {
  if (!h || !x0 || !ms || reps < 2 || (reps & 1)) return TBNAV_ERR_INVALID_ARG;
  if (!(fused_dev(h) && rng_in_kernel(h))) {
    // no in-kernel noise for this configuration: the production tick samples into the handle's buffers and runs the plain kernels
    const int rc = tbnav_mppi_sample_noise(h, seed, tick, stream);
    return rc != TBNAV_OK ? rc : tbnav_mppi_profile_kernels(h, x0, nullptr, nullptr, stream, reps, ms);
  }
  DeviceGuard guard(h->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipEvent_t ev[2];
  for (auto& e : ev) TBNAV_HIP(hipEventCreate(&e));
  int rc = TBNAV_OK;
  for (int i = 0; i < TBNAV_MPPI_NKERNELS; ++i) ms[i] = 0.f;
  // the launches of tbnav_mppi_enqueue_rng, kernel by kernel, in the form the steady-state tick runs them: the in-kernel-noise
  // instantiation of the fused kernel and, with noise ahead, that kernel finding its pairs drawn (one untimed tick `tick` draws
  // tick + 1's; every timed launch is tick + 1 and hits) and the combine with its sampler blocks (drawing tick + 2 + r)
  const bool ahead = ahead_on(h);
  RngArgs g = rng_args(h, seed, tick);
  if (ahead) {
    rc = rng_tick(h, x0, g, st);
    g = with_ahead(h, g);
  }
  timed(ev, st, reps, ms, 0, rc, [&](int r) {
    RngArgs gr = g;
    gr.base = rng_base(h, ahead ? tick + 1 : tick + (uint64_t)r);
    return launch_fused(h, x0, h->d_duL, h->d_duR, st, &gr);
  });
  timed(ev, st, reps, ms, 2, rc, [&](int r) {
    RngArgs nx = g;
    nx.base = rng_base(h, tick + 2 + (uint64_t)r);
    return launch_combine(h, h->d_records_f, 1, st, h->fused_S, nullptr, ahead ? &nx : nullptr);
  });
  for (auto& e : ev) (void)hipEventDestroy(e);
  return rc;
}

int tbnav_mppi_last_kernel_names(const tbnav_mppi* h, char* rollout, int32_t rollout_cap, char* combine, int32_t combine_cap) {
  if (!h) return TBNAV_ERR_INVALID_ARG;
  if (rollout && rollout_cap > 0) form_name(h->lk_rollout, rollout, (size_t)rollout_cap);   // (as the profiler spells the instantiation)
  if (combine && combine_cap > 0) form_name(h->lk_combine, combine, (size_t)combine_cap);
  return TBNAV_OK;
}

int tbnav_mppi_last_controls(tbnav_mppi* h, void* stream, double u_out[2]) {
  if (!h || !u_out) return TBNAV_ERR_INVALID_ARG;
  DeviceGuard guard(h->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  auto exchange_ok = [&]() -> int { return exchange_error(h); };  // (the stream has been waited for) an exchange that failed left its mark in host memory
  if (h->published != h->seq) {  // the last tick was enqueue-only: fetch the device copy
    TBNAV_HIP(hipMemcpyAsync(h->h_out, h->d_out, 2 * sizeof(double), hipMemcpyDeviceToHost, st));
    TBNAV_HIP(hipStreamSynchronize(st));
    u_out[0] = h->h_out[0];
    u_out[1] = h->h_out[1];
    return exchange_ok();
  }
  // The last combine published (ul, ur, tick number) in mapped host memory.  Poll for its number for a short while (a
  // control loop calls this right behind the enqueue: the answer is microseconds away and a stream synchronisation
  // costs more than the tick), then fall back to waiting on the stream.
  const double want = (double)h->seq;
  volatile double* vo = h->h_out;
  const auto t0 = std::chrono::steady_clock::now();
  bool seen = vo[2] == want;
  while (!seen && std::chrono::steady_clock::now() - t0 < std::chrono::microseconds(200)) seen = vo[2] == want;
  if (!seen) TBNAV_HIP(hipStreamSynchronize(st));
  std::atomic_thread_fence(std::memory_order_acquire);
  u_out[0] = vo[0];
  u_out[1] = vo[1];
  return exchange_ok();
}

int tbnav_mppi_new_controls_dev(tbnav_mppi* h, const double x0[3], const double* d_duL,
                                const double* d_duR, void* stream, double u_out[2]) {
  if (!u_out) return TBNAV_ERR_INVALID_ARG;
  if (h) h->publish_next = true;
  int rc = tbnav_mppi_enqueue_dev(h, x0, d_duL, d_duR, stream);
  if (h) h->publish_next = false;
  if (rc != TBNAV_OK) return rc;
  return tbnav_mppi_last_controls(h, stream, u_out);
}

int tbnav_mppi_new_controls(tbnav_mppi* h, const double x0[3], const double* noise_host,
                            double u_out[2]) {
  if (!h || !x0 || !noise_host || !u_out) return TBNAV_ERR_INVALID_ARG;
  DeviceGuard guard(h->device);
  const size_t n = (size_t)h->T * h->K;
  if (!h->d_raw) TBNAV_HIP(hipMalloc((void**)&h->d_raw, 2 * n * sizeof(double)));
  TBNAV_HIP(hipMemcpyAsync(h->d_raw, noise_host, 2 * n * sizeof(double), hipMemcpyHostToDevice, nullptr));
  const int blocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
  hipLaunchKernelGGL(mppi_unpack_noise, dim3(blocks), dim3(256), 0, nullptr, h->T, h->K, h->d_raw,
                     h->d_duL, h->d_duR);
  TBNAV_HIP(hipGetLastError());
  return tbnav_mppi_new_controls_dev(h, x0, nullptr, nullptr, nullptr, u_out);
}

int tbnav_mppi_sample_noise(tbnav_mppi* h, uint64_t seed, uint64_t tick, void* stream) {
  if (!h) return TBNAV_ERR_INVALID_ARG;
  DeviceGuard guard(h->device);
  const size_t n = (size_t)h->T * h->K;
  const int blocks = (int)((n + 255) / 256 < 8192 ? (n + 255) / 256 : 8192);
  hipLaunchKernelGGL(mppi_sample_noise, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream),
                     h->T, h->K, seed, rng_base(h, tick), std::sqrt(h->p.ul_var), std::sqrt(h->p.ur_var), h->sampler, h->d_duL,
                     h->d_duR);
  TBNAV_HIP(hipGetLastError());
  return TBNAV_OK;
}

// Production tick: the perturbations of tick `tick` under `seed` are the ones tbnav_mppi_sample_noise would write, but
// for the fused small-K kernel they are generated inside it and never stored (the soft-min reads them from the
// workgroup's LDS tile).  Other configurations sample into the handle's buffers first — same values, same result.
int tbnav_mppi_enqueue_rng(tbnav_mppi* h, const double x0[3], uint64_t seed, uint64_t tick, void* stream) {
  if (!h || !x0) return TBNAV_ERR_INVALID_ARG;
  if (h->comm) return sharded_tick(h, x0, nullptr, nullptr, &seed, tick, stream);
  if (!rng_in_kernel(h)) {
    const int rc = tbnav_mppi_sample_noise(h, seed, tick, stream);
    return rc != TBNAV_OK ? rc : tbnav_mppi_enqueue_dev(h, x0, nullptr, nullptr, stream);
  }
  DeviceGuard guard(h->device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  return rng_tick(h, x0, rng_args(h, seed, tick), st);
}

namespace {
bool graph_usable(const tbnav_mppi* h, const TickGraph& g, const double* x0, uint64_t seed, hipStream_t st) {
  return g.exec && g.epoch == h->cfg_epoch && g.seed == seed && g.stream == st && std::memcmp(g.x0, x0, sizeof g.x0) == 0;
}
// Capture `len` ticks (len even: the controls' double buffer is back where it was after a replay) and a last node that advances
// the device's tick word by len.  A capture that fails turns the replays off for good (plain launches from there on).
void build_graph(tbnav_mppi* h, TickGraph& g, int len, const double* x0, uint64_t seed, hipStream_t st) {
  // (another stream may not have run the previous replay's tick-advance node yet: what the device word holds is unknown)
  h->tg_dev_tick = ~0ull;
  drop_graph(g);
  if (!h->d_tick0 && hipMalloc((void**)&h->d_tick0, sizeof(uint64_t)) != hipSuccess) { h->d_tick0 = nullptr; h->graph_on = false; }
  if (!h->graph_on) return;
  if (hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed) != hipSuccess) { h->graph_on = false; (void)hipGetLastError(); return; }
  const int ucur0 = h->ucur; const uint64_t seq0 = h->seq;
  int rc = TBNAV_OK;
  for (int t = 0; t < len && rc == TBNAV_OK; ++t) {
    RngArgs ra = rng_args(h, seed, (uint64_t)t);
    ra.tick0 = h->d_tick0; ra.per_tick = (uint64_t)h->T * h->k_global;
    rc = rng_tick(h, x0, ra, st);   // (the last tick's combine draws the first tick of the next replay: the tag holds the resolved counters)
  }
  if (rc == TBNAV_OK) { hipLaunchKernelGGL(mppi_tick_advance, dim3(1), dim3(1), 0, st, h->d_tick0, (uint64_t)len); if (hipGetLastError() != hipSuccess) rc = TBNAV_ERR_HIP; }
  hipGraph_t gr = nullptr;
  const hipError_t e_end = hipStreamEndCapture(st, &gr);
  h->ucur = ucur0; h->seq = seq0;  // nothing ran: the host-side state goes back
  if (rc == TBNAV_OK && e_end == hipSuccess && gr && hipGraphInstantiate(&g.exec, gr, nullptr, nullptr, 0) == hipSuccess) {
    g.graph = gr; g.len = len; g.seed = seed; g.stream = st; g.ucur = h->ucur; g.epoch = h->cfg_epoch; std::memcpy(g.x0, x0, sizeof g.x0);
  } else {
    if (gr) (void)hipGraphDestroy(gr);
    g.exec = nullptr; h->graph_on = false; (void)hipGetLastError();
  }
}
int replay_graph(tbnav_mppi* h, const TickGraph& g, uint64_t t0, hipStream_t st) {
  // (consecutive replays need no copy: the last node of the one before has advanced the device word)
  if (t0 != h->tg_dev_tick) {
    h->tg_dev_tick = ~0ull;
    hipLaunchKernelGGL(mppi_tick_set, dim3(1), dim3(1), 0, st, h->d_tick0, t0);
    TBNAV_HIP(hipGetLastError());
  }
  { const hipError_t eg = hipGraphLaunch(g.exec, st); if (eg != hipSuccess) { h->tg_dev_tick = ~0ull; TBNAV_HIP(eg); } }
  h->tg_dev_tick = t0 + (uint64_t)g.len;
  h->seq += (uint64_t)g.len;  // ucur: unchanged after an even number of ticks; the shift stays owed
  h->graph_ticks += (uint64_t)g.len;
  return TBNAV_OK;
}
}  // namespace

int tbnav_mppi_enqueue_rng_batch(tbnav_mppi* h, const double* x0s, int32_t x0_stride, uint64_t seed, uint64_t first_tick, int32_t n_ticks,
                                 void* stream) {
  if (!h || !x0s || n_ticks < 0 || (x0_stride != 0 && x0_stride < 3)) return TBNAV_ERR_INVALID_ARG;
  int32_t i = 0;
  constexpr int kGraphTicks = 100;  // (even: the controls' double buffer is back where it was after a chunk)
  constexpr int kShortMin = 8;      // the shortest batch worth a graph of its own
  hipStream_t st = static_cast<hipStream_t>(stream);
  // (only where the tick is short enough for the launches themselves to matter: graph_worth_it, mppi_plan.hpp)
  if (h->graph_on && !h->comm && x0_stride == 0 && st != nullptr && graph_worth_it(rng_in_kernel(h), h->fused_r, h->K, n_ticks)) {
    DeviceGuard guard(h->device);
    // (the chunk graph is built by the first batch call that could use one, however short — a warm-up call, typically — so that a
    //  later long call does not pay the ~1 ms of capture + instantiation)
    // the first tick after set_controls / set_initial_controls reads the vector unshifted: keep it out of the graphs
    if (!h->pending_shift) { const int rc = tbnav_mppi_enqueue_rng(h, x0s, seed, first_tick, stream); if (rc != TBNAV_OK) return rc; ++i; }
    const bool usable = graph_usable(h, h->tg, x0s, seed, st);
    // (a graph has the controls' double buffer baked in as it stood at capture: on the other parity ONE plain tick brings it
    //  back — a rebuild would cost ~0.5 ms inside the caller's batch)
    if (usable && h->tg.ucur != h->ucur && n_ticks - i > kGraphTicks) {
      const int rc = tbnav_mppi_enqueue_rng(h, x0s, seed, first_tick + (uint64_t)i, stream);
      if (rc != TBNAV_OK) return rc;
      ++i;
    }
    const bool same = usable && h->tg.ucur == h->ucur;
    if (!same && (!usable || n_ticks - i >= kGraphTicks)) build_graph(h, h->tg, kGraphTicks, x0s, seed, st);
    while (h->tg.exec && n_ticks - i >= kGraphTicks) {
      const int rc = replay_graph(h, h->tg, first_tick + (uint64_t)i, st);
      if (rc != TBNAV_OK) return rc;
      i += kGraphTicks;
    }
    // What is left (or a batch shorter than a chunk): one graph of exactly that many ticks, less one if odd.  Built by the second
    // batch in a row that asks for the same length on the same parity of the double buffer — a caller that times blocks of 20
    // ticks gets it in its second block; one with batches of ever-changing length never pays for a graph it would not reuse.
    // (Measured at K = 1024, T = 50, blocks of 20 between synchronisations: 9.3 us per tick replayed, 9.8-12.1 launched one by
    //  one — the spread is the host's launch rate, which the replay does not depend on.  An earlier note here gave a 10-tick
    //  replay 9.9-10.2 us against 8.9: that was a chunk graph plus plain ticks plus the tick-set launch in one batch.)
    // (an odd batch leaves the double buffer on the other parity: ONE plain tick in front brings the next batch back to the parity
    //  the graph was captured on, if what is left then still is the graph's length)
    if (h->graph_on && graph_usable(h, h->tgs, x0s, seed, st) && h->tgs.ucur != h->ucur && ((n_ticks - i - 1) & ~1) == h->tgs.len) {
      const int rc = tbnav_mppi_enqueue_rng(h, x0s, seed, first_tick + (uint64_t)i, stream);
      if (rc != TBNAV_OK) return rc;
      ++i;
    }
    const int L = (n_ticks - i) & ~1;
    if (h->graph_on && h->tg.exec && L >= kShortMin) {
      const bool fits = graph_usable(h, h->tgs, x0s, seed, st) && h->tgs.len == L && h->tgs.ucur == h->ucur;
      if (!fits && h->tgs_wish_len == L && h->tgs_wish_ucur == h->ucur) build_graph(h, h->tgs, L, x0s, seed, st);
      h->tgs_wish_len = L; h->tgs_wish_ucur = h->ucur;
      if (h->tgs.exec && graph_usable(h, h->tgs, x0s, seed, st) && h->tgs.len == L && h->tgs.ucur == h->ucur) {
        const int rc = replay_graph(h, h->tgs, first_tick + (uint64_t)i, st);
        if (rc != TBNAV_OK) return rc;
        i += L;
      }
    }
  }
  for (; i < n_ticks; ++i) {
    const int rc = tbnav_mppi_enqueue_rng(h, x0s + (size_t)i * x0_stride, seed, first_tick + (uint64_t)i, stream);
    if (rc != TBNAV_OK) return rc;
  }
  return TBNAV_OK;
}

int tbnav_mppi_new_controls_rng(tbnav_mppi* h, const double x0[3], uint64_t seed, uint64_t tick, void* stream, double u_out[2]) {
  if (!h || !u_out) return TBNAV_ERR_INVALID_ARG;
  h->publish_next = true;
  const int rc = tbnav_mppi_enqueue_rng(h, x0, seed, tick, stream);
  h->publish_next = false;
  return rc != TBNAV_OK ? rc : tbnav_mppi_last_controls(h, stream, u_out);
}

int tbnav_mppi_get_noise(tbnav_mppi* h, double* duL_host, double* duR_host) {
  if (!h || !duL_host || !duR_host) return TBNAV_ERR_INVALID_ARG;
  DeviceGuard guard(h->device);
  const size_t n = (size_t)h->T * h->K;
  TBNAV_HIP(hipDeviceSynchronize());
  TBNAV_HIP(hipMemcpy(duL_host, h->d_duL, n * sizeof(double), hipMemcpyDeviceToHost));
  TBNAV_HIP(hipMemcpy(duR_host, h->d_duR, n * sizeof(double), hipMemcpyDeviceToHost));
  return TBNAV_OK;
}

int tbnav_mppi_debug_sincos(const double* x_host, int32_t n, double* sin_host, double* cos_host) {
  if (!x_host || !sin_host || !cos_host || n <= 0) return TBNAV_ERR_INVALID_ARG;
  double *dx = nullptr, *ds = nullptr, *dc = nullptr;
  hipError_t e = hipMalloc((void**)&dx, sizeof(double) * n);
  if (e == hipSuccess) e = hipMalloc((void**)&ds, sizeof(double) * n);
  if (e == hipSuccess) e = hipMalloc((void**)&dc, sizeof(double) * n);
  if (e == hipSuccess) e = hipMemcpy(dx, x_host, sizeof(double) * n, hipMemcpyHostToDevice);
  if (e == hipSuccess) { hipLaunchKernelGGL(mppi_debug_sincos, dim3((n + 255) / 256), dim3(256), 0, nullptr, n, dx, ds, dc); e = hipGetLastError(); }
  if (e == hipSuccess) e = hipMemcpy(sin_host, ds, sizeof(double) * n, hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(cos_host, dc, sizeof(double) * n, hipMemcpyDeviceToHost);
  (void)hipFree(dx); (void)hipFree(ds); (void)hipFree(dc);
  TBNAV_HIP(e);
  return TBNAV_OK;
}

int tbnav_mppi_debug_div_lambda(const double* x_host, int32_t n, double lambda, double* out_host, int32_t* used_reciprocal) {
  if (!x_host || !out_host || n <= 0) return TBNAV_ERR_INVALID_ARG;
  const Lam lam = lam_of(lambda);
  if (used_reciprocal) *used_reciprocal = lam.inv != 0.0;
  double *dx = nullptr, *dy = nullptr;
  hipError_t e = hipMalloc((void**)&dx, sizeof(double) * n);
  if (e == hipSuccess) e = hipMalloc((void**)&dy, sizeof(double) * n);
  if (e == hipSuccess) e = hipMemcpy(dx, x_host, sizeof(double) * n, hipMemcpyHostToDevice);
  if (e == hipSuccess) { hipLaunchKernelGGL(mppi_debug_div_lambda, dim3((n + 255) / 256), dim3(256), 0, nullptr, n, dx, lam, dy); e = hipGetLastError(); }
  if (e == hipSuccess) e = hipMemcpy(out_host, dy, sizeof(double) * n, hipMemcpyDeviceToHost);
  (void)hipFree(dx); (void)hipFree(dy);
  TBNAV_HIP(e);
  return TBNAV_OK;
}

int tbnav_mppi_debug_combine_general(tbnav_mppi* h, double* u_host) {
  if (!h || !u_host) return TBNAV_ERR_INVALID_ARG;
  const KernelForm last = h->lk_combine;
  const int keep = last.arg[0], S = h->lk_S, T = h->T;
  if (last.family != kCombine || last.arg[1] != 0 || !h->lk_records || h->lk_G != 1 || S > keep * kWave) return TBNAV_ERR_INVALID_ARG;
  DeviceGuard guard(h->device);
  // the last tick's own geometry (one group, nothing drawn ahead), run by the general form <KEEP, 1>; the tick's input controls are
  // the vector that is no longer current (the tick wrote the other one), read with the shift the tick read them with
  const CombinePlan p = plan_combine(T, h->K, 1, S, false, false, false, false);
  const DirectSrc ds{nullptr, 0ull, nullptr, nullptr, 0u};
  const RngArgs off{0, 0, 0.0, 0.0};
  double* d = nullptr;   // [2][T] controls, then the two to apply
  TBNAV_HIP(hipDeviceSynchronize());
  hipError_t e = hipMalloc((void**)&d, sizeof(double) * (2 * (size_t)T + 2));
  if (e == hipSuccess) {
    e = hipErrorInvalidDeviceFunction;   // (a KEEP the list does not have)
#define TBNAV_X(KEEP, MODE)                                                                                                                            \
    if (MODE == 1 && keep == KEEP) {                                                                                                                   \
      hipLaunchKernelGGL((mppi_combine<KEEP, MODE>), dim3(p.blocks), dim3(p.block), 0, nullptr, h->lk_records, (const double*)h->d_u[1 - h->ucur],    \
                         (double*)nullptr, (const uint64_t*)nullptr, T, S, h->lk_ushift, p.blocks, 1, p.tpr_log2, (uint64_t*)nullptr, lam_of(h),       \
                         h->p.max_wheel_vel, h->uinit[0], h->uinit[1], d, d + 2 * (size_t)T, (double*)nullptr, 0.0, ds, rng_rest(off));                \
      e = hipGetLastError();                                                                                                                           \
    }
    TBNAV_MPPI_COMBINE_FORMS(TBNAV_X)
#undef TBNAV_X
  }
  if (e == hipSuccess) e = hipMemcpy(u_host, d, sizeof(double) * 2 * (size_t)T, hipMemcpyDeviceToHost);
  (void)hipFree(d);
  TBNAV_HIP(e);
  return TBNAV_OK;
}

int tbnav_mppi_get_cost_to_go(tbnav_mppi* h, double* J_host) {
  if (!h || !J_host) return TBNAV_ERR_INVALID_ARG;
  if (!h->j_valid) return TBNAV_ERR_INVALID_ARG;  // the last tick ran the fused kernel without TBNAV_MPPI_OPT_KEEP_J
  DeviceGuard guard(h->device);
  TBNAV_HIP(hipDeviceSynchronize());
  TBNAV_HIP(hipMemcpy(J_host, h->d_J, (size_t)h->T * h->K * sizeof(double), hipMemcpyDeviceToHost));
  if (h->prefix_rows > 0) {  // rows below prefix_rows hold exclusive prefixes: J(i) = S - E(i), as mppi_partials forms it
    std::vector<double> tot((size_t)h->K);
    TBNAV_HIP(hipMemcpy(tot.data(), h->d_total, tot.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (int i = 0; i < h->prefix_rows; ++i)
      for (int k = 0; k < h->K; ++k)   // (a total that overflowed: +inf on every row, as mppi_partials reads it)
        J_host[(size_t)i * h->K + k] = std::isinf(tot[k]) ? tot[k] : tot[k] - J_host[(size_t)i * h->K + k];
  }
  return TBNAV_OK;
}

}  // extern "C"

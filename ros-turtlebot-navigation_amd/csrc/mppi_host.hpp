// mppi_host.hpp — the MPPI handle and what the host files share (mppi.hip: create / options / launchers / single-GPU C-ABI;
// mppi_field.hip: the cost field; mppi_sharded.hip: communicator attachment, direct exchange, sharded tick, groups).  Kernels and
// launch structs: mppi_device.hpp; what a handle decides and which instantiation a tick launches: mppi_plan.hpp.
#ifndef TBNAV_MPPI_HOST_HPP
#define TBNAV_MPPI_HOST_HPP
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "comm.hpp"
#include "common.hpp"
#include "mppi_device.hpp"
#include "tbnav_mppi.h"

using tbnav_mk::DirectPub;

// =================================================================================================
// Handle
// =================================================================================================
struct tbnav_mppi {
  tbnav_mppi_params p;
  int T = 0, K = 0, S = 0, device = 0;
  tbnav_mk::KernelForm lk_rollout, lk_combine;   // the instantiations the last rollout launch and the last combine picked (tbnav_mppi_last_kernel_names)
  const double* lk_records = nullptr;   // ... what that combine read: its records, S, G and whether it read the controls shifted
  int lk_S = 0, lk_G = 0, lk_ushift = 0;   //     (tbnav_mppi_debug_combine_general)
  double xd[3] = {0, 0, 0};
  double uinit[2] = {0, 0};
  double* d_u[2] = {nullptr, nullptr};  // [2][T] each; d_u[ucur] holds the controls, d_u[1-ucur] receives the next update
  int ucur = 0;
  bool pending_shift = false;   // d_u[ucur] is an updated, not yet shifted vector (the shift is applied on read)
  double* d_J = nullptr;        // [T][K]
  double* d_duL = nullptr;      // [T][K] own noise buffers (host-noise upload / device RNG)
  double* d_duR = nullptr;
  double* d_raw = nullptr;      // [K][T][2] staging for host-order noise (lazy)
  double* d_records = nullptr;  // [T][S][8]
  double* d_out = nullptr;      // [2] device copy of the last controls
  double* d_out_host = nullptr; // device view of h_out
  double* h_out = nullptr;      // mapped pinned [4]: ul, ur, tick number of the combine that published them
  uint64_t seq = 0;             // combines enqueued so far
  uint64_t published = 0;       // tick number of the last combine that was asked to publish to h_out
  bool publish_next = false;    // set by the synchronous entry points round their enqueue
  // tbnav_mppi_enqueue_rng_batch replays captured hipGraphs of ticks (two launches each) instead of launching them one by one:
  // chunks of kGraphTicks (~0.5 us less per tick of a 8-9 us tick) and, for what is left — or a batch shorter than a chunk —,
  // ONE graph of the batch's own length (tgs): a batch of 20 ticks is one submission instead of forty, 9.3 us per tick whatever
  // the host's launch rate is doing (9.8-12.1 launched one by one)
  bool graph_on = true;         // TBNAV_MPPI_OPT_BATCH_GRAPH; cleared for good if a capture ever fails
  struct TickGraph {
    hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr;
    int len = 0; uint64_t seed = 0; double x0[3] = {0, 0, 0}; hipStream_t stream = nullptr; int ucur = -1; uint64_t epoch = ~0ull;
  };
  TickGraph tg, tgs;
  int tgs_wish_len = 0, tgs_wish_ucur = -1;   // the short graph is built by the SECOND batch in a row that could use the same one
  // The graph's kernel nodes hold BY VALUE everything launch_fused / launch_combine read from the handle when it was captured
  // (waypoint, uinit, lambda, dynamics, trig, keep_j + the J pointer, the rng shard, fused_S and the record buffer).  Every
  // setter that changes one of those bumps cfg_epoch; a graph captured under another epoch is rebuilt, never replayed.
  uint64_t cfg_epoch = 0;
  uint64_t graph_ticks = 0;  // ticks enqueued through graph replays so far (tbnav_mppi_graph_replayed_ticks: what a bench line should say ran)
  uint64_t* d_tick0 = nullptr;
  uint64_t tg_dev_tick = ~0ull;  // what *d_tick0 holds once everything enqueued so far has run (each replay's last node adds the chunk)
  int lds_from = 0;           // first time step whose loss is staged in LDS (0 = all of them)
  int prefix_rg = 0;          // > 0: mppi_rollout_prefix (the large-K default): exact suffix sums for the last 4*prefix_rg steps, exclusive prefixes before
  int prefix_rows = 0;        // rows of d_J that hold exclusive prefixes after the LAST rollout launch (0: every row is J)
  double* d_total = nullptr;  // [K] whole cost of every rollout (mppi_rollout_prefix)
  int scan_tc = 0;            // steps per thread of the time-parallel rollout kernel (0 = sequential kernel)
  int fused_r = 0;            // rollouts per workgroup of the fused rollout+partials kernel (0 = off: three kernels)
  int fused_S = 0;            // its records per time step, ceil(K / fused_r)
  // which ticks take the fused kernel: resident-noise ticks (tbnav_mppi_enqueue_dev, new_controls*) and device-noise ticks
  // (tbnav_mppi_enqueue_rng ...: the perturbations are drawn inside it) cross over to the three-kernel tick at different K
  bool fused_dev = false, fused_rng = false;
  double* d_records_f = nullptr;  // [T][fused_S][8]
  int trig = 1;               // sincos evaluations per RK4 step (1 = angle addition, 3 = the reference's three)
  int dyn = 0;                // rollout dynamics: 0 = the reference's RK4 cart, 1 = exact arcs (tbnav_mppi_set_dynamics)
  bool keep_j = false;        // the fused kernel also writes J to HBM (parity hook tbnav_mppi_get_cost_to_go); other kernels always do
  bool j_valid = false;       // d_J holds the last tick's cost-to-go
  uint64_t k0 = 0, k_global = 0;  // device noise source: this handle's rollouts are [k0, k0 + K) of k_global (sharded ensembles)
  // sharded ensemble (tbnav_mppi_attach_comm / tbnav_mppi_group_*): every tick is shard partials -> ONE all-gather of the
  // records (RCCL) -> the combine of all shards' records, all enqueued on the tick's stream
  tbnav_comm* comm = nullptr;
  double* d_records_all = nullptr;  // [nranks][T][S][8]; this rank's records are written in place at [rank]
  // direct exchange (mppi_direct_publish / _collect): set up at attach for multi-process communicators when every rank can
  // (fine-grained memory, IPC mapping, a self-test); otherwise the communicator's all-gather carries the records
  bool direct_want = true, direct_on = false;   // TBNAV_MPPI_OPT_DIRECT_EXCHANGE
  unsigned long long* d_dx = nullptr;           // [2 parities][nranks][2 * n] tagged words (n = T * S * 8), fine-grained
  unsigned long long** d_dx_peers = nullptr;    // [nranks] every rank's d_dx as mapped into this process
  std::vector<void*> dx_opened;                 // the mappings of the peers' buffers (closed at detach)
  // the exchange's error words, alive while a communicator is attached (either exchange): mapped pinned, raised by a combine that ran
  // out of time waiting for a peer's words (bit 0) or met a poisoned record — a rank whose own rollouts failed (bit 1); latched
  int* h_dx_err = nullptr; int* d_dx_err = nullptr;
  int* d_dx_dead = nullptr;                          // its device twin: later ticks see it without a trip over PCIe
  bool fail_next = false;                            // fault injection (TBNAV_MPPI_OPT_FAULT_INJECT, tests): the next sharded tick's local half fails
  bool wide_combine = true;                          // TBNAV_MPPI_OPT_WIDE_COMBINE: four waves per time step when a step has more than 256 records
  int sampler = 1;                                   // TBNAV_MPPI_OPT_SAMPLER: 1 (default) = fp64 Box-Muller on 52-bit uniforms, 0 = fp32 on 24-bit uniforms
  // noise ahead (TBNAV_MPPI_OPT_NOISE_AHEAD): the combine of a device-noise tick draws the next tick's perturbations in blocks of its
  // own, into d_ahead; the next fused kernel takes them from there when d_ahead_tag says they are its own (RngArgs).  Kept apart from
  // d_duL / d_duR (tbnav_mppi_get_noise, the sample-then-tick path).  Allocated where it is used: 8 rollouts per workgroup, noise drawn inside
  bool noise_ahead = true;
  double* d_ahead = nullptr;       // [K][T] (dl, dr) pairs
  uint64_t* d_ahead_tag = nullptr; // [kTagWords]
  unsigned long long dx_budget = 200000000ull;       // 2 s of the 100 MHz clock (host-side skew between ranks is legitimate — a control loop's is milliseconds; longer: the peer has failed)
  bool dx_withhold = false;                          // fault injection (TBNAV_MPPI_OPT_DIRECT_EXCHANGE = 2, tests): this rank's records never reach its peers
  unsigned int dx_seq = 0;
  // set by the sharded tick round its call of the shard-partials entry point: if that ends in mppi_merge_records, the kernel
  // publishes the records itself (and clears this); otherwise the tick launches mppi_direct_publish
  bool pub_pending = false;
  DirectPub pub_next{nullptr, 0, 0, 0, 0u, 0};
  // cost field (tbnav_mppi.h, COST FIELD; mppi_field.hip): while field_on, every tick's rollout launch is mppi_rollout_field and the
  // handle takes neither the fused kernel nor the noise-ahead draw nor a captured graph (tbnav_mh::fused_dev / fused_rng below)
  bool field_on = false;
  tbnav_mppi_cost_field field{0, 0, 0.0, 0.0, 0.0, 0.0};
  float* d_field = nullptr;     // [nx][ny]
};

// One process driving several GPUs: the whole ensemble behind one object (what controller::MPPI built with n_gpus > 1 holds).
struct tbnav_mppi_group {
  int n = 0;
  std::vector<tbnav_mppi*> m;
  std::vector<tbnav_comm*> c;
  std::vector<hipStream_t> st;
  std::vector<double*> d_raw;  // per member: staging of its slice of host-order noise
  int K_global = 0;
};

namespace tbnav_mh {
using namespace tbnav_mk;

using tbnav::DeviceGuard;

// which ticks take the fused kernel (resident noise / noise drawn inside it): never a handle with a cost field
inline bool fused_dev(const tbnav_mppi* h) { return h->fused_dev && !h->field_on; }
inline bool fused_rng(const tbnav_mppi* h) { return h->fused_rng && !h->field_on; }
// the warm-start controls as the next launch reads them
inline USrc usrc_of(const tbnav_mppi* h) { return USrc{h->d_u[h->ucur], h->pending_shift ? 1 : 0, h->uinit[0], h->uinit[1]}; }
// (mppi_field.hip) the rollout launch of a handle with a cost field: the form plan_rollout named, over the field's list
int launch_rollout_field(tbnav_mppi* h, const RolloutPlan& p, const RolloutArgs& a, const USrc& usrc, const double* d_duL, const double* d_duR, hipStream_t st);
// the two halves of tbnav_mppi_set_cost_field, apart so that a group can stage every member's copy before any member changes:
// field_stage checks F1 and uploads the values (*d_new = nullptr for geom == nullptr); field_commit waits for the device and swaps
int field_stage(tbnav_mppi* h, const tbnav_mppi_cost_field* geom, const float* values_host, float** d_new);
int field_commit(tbnav_mppi* h, const tbnav_mppi_cost_field* geom, float* d_new);
// field_stage for values that are on a device already (nav.hip: tbnav_nav_apply_to_mppi): d_values, nx*ny floats on src_device and
// finite by the caller's construction, are copied device to device (a peer copy when src_device is not the handle's)
int field_stage_device(tbnav_mppi* h, const tbnav_mppi_cost_field& geom, const float* d_values, int src_device, float** d_new);
// (mppi.hip)
Lam lam_of(double lambda);
inline Lam lam_of(const tbnav_mppi* h) { return lam_of(h->p.lambda); }
// next: a single-GPU combine also draws these perturbations (noise ahead; ignored by the other forms)
int launch_combine(tbnav_mppi* h, const double* d_records, int G, hipStream_t st, int S = -1, const DirectSrc* direct = nullptr,
                   const RngArgs* next = nullptr);
// (mppi_sharded.hip)
int sharded_tick(tbnav_mppi* h, const double x0[3], const double* d_duL, const double* d_duR, const uint64_t* seed, uint64_t tick, void* stream);
void direct_teardown(tbnav_mppi* h);
void exchange_words_free(tbnav_mppi* h);
// a latched error of the attached exchange (the stream has been waited for, or the caller accepts an earlier tick's): TBNAV_OK or
// TBNAV_ERR_HIP with the text set
int exchange_error(const tbnav_mppi* h);

}  // namespace tbnav_mh
#endif

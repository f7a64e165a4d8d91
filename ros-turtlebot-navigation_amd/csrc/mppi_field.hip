// mppi_field.hip — the cost field of include/tbnav_mppi.h (section COST FIELD, F1-F5): a map term in the rollout loss, an OPTION the
// reference does not have (its loss is quadratic only, controller/include/controller/mppi.hpp:87-105).  Here: the lookup (F2), the
// rollout kernel of a handle with a field (mppi_rollout_field: mppi_rollout_cost's shape — one lane per rollout, groups of kGroup
// steps, the noise ring, the losses staged in LDS / J, the backward suffix sum — with the field's gathers issued between a group's
// integration and its quadratic losses), its launch, and the setters.  The shared rollout arithmetic is mppi_device.hpp's; no
// existing kernel, argument struct or file of kernels changes for it: the field travels as a kernel argument of its own.
#include <cmath>
#include <vector>

#include "mppi_host.hpp"

namespace tbnav_mk {

// F1 as the kernels take it; inv = 1.0 / resolution is formed on the host
struct FieldArgs {
  const float* v;  // [nx][ny]
  double xmin, ymin, inv, weight;
  int nx, ny;
};

// F2, first half: one axis' cell and fraction.  The clamps come BEFORE the index is formed, so no position — NaN, +-inf, 1e300 —
// gives an index outside 0 .. n-2.  (gx >= 0 here, so the conversion's truncation is the floor.)
__device__ __forceinline__ void field_axis(double p, double pmin, double inv, int n, int& i, double& f) {
  double g = ((p - pmin) * inv) - 0.5;
  g = g > 0.0 ? g : 0.0;   // (a NaN fails the comparison and goes to 0)
  g = g < (double)(n - 1) ? g : (double)(n - 1);
  const int c = (int)g;
  i = c < n - 2 ? c : n - 2;
  f = g - (double)i;
}
// The four neighbouring values of a position, requested (the loads are issued here and waited for where the values are first used)
struct FieldTap { float c00, c01, c10, c11; double fx, fy; };
__device__ __forceinline__ void field_gather(const FieldArgs& f, double x, double y, FieldTap& t) {
  int ix, iy;
  field_axis(x, f.xmin, f.inv, f.nx, ix, t.fx);
  field_axis(y, f.ymin, f.inv, f.ny, iy, t.fy);
  const float* p = f.v + (ix * f.ny + iy);   // <= (nx-2)*ny + ny-2; the far corner is nx*ny - 1
  t.c00 = p[0]; t.c01 = p[1]; t.c10 = p[f.ny]; t.c11 = p[f.ny + 1];
}
// F2, second half: the three lerps in fp64
__device__ __forceinline__ double field_lerp(const FieldTap& t) {
  const double c00 = (double)t.c00, c01 = (double)t.c01, c10 = (double)t.c10, c11 = (double)t.c11;
  const double a = c00 + t.fy * (c01 - c00);
  const double b = c10 + t.fy * (c11 - c10);
  return a + t.fx * (b - a);
}

// One group of G steps: integrate (mppi_device.hpp), then form all G cells and issue all 4 G gathers, and only then the quadratic
// losses — one wave per SIMD has nothing else to hide an L2 hit under — and last the lerps and the field's share (F3).
template <int TRIG, int G, bool TO_LDS>
__device__ __forceinline__ void field_group(const RolloutArgs& a, const FieldArgs& f, int i0, int lane, int k, double& x, double& y, double& th,
                                            const double (&dl)[G], const double (&dr)[G], const double* __restrict__ u,
                                            double* __restrict__ lds_loss, double* __restrict__ J) {
  const int T = a.T, K = a.K;
  double ul[G], ur[G], thq[G], xq[G], yq[G], l[G];
  FieldTap tap[G];
#pragma unroll
  for (int q = 0; q < G; ++q) {
    ul[q] = u[i0 + q] + dl[q];        // mppi.cpp:93 — rollout controls are not clamped
    ur[q] = u[T + i0 + q] + dr[q];
  }
  if constexpr (TRIG == 4) arc_steps<G>(a, x, y, th, ul, ur, thq, xq, yq);
  else rk4_steps<TRIG, G>(a, x, y, th, ul, ur, thq, xq, yq);
#pragma unroll
  for (int q = 0; q < G; ++q) field_gather(f, xq[q], yq[q], tap[q]);
#pragma unroll
  for (int q = 0; q < G; ++q)
    l[q] = (i0 + q == T - 1) ? terminal_loss(a, xq[q], yq[q], thq[q])  // mppi.cpp:105 overwrites, not adds
                             : lqr_loss(a, xq[q], yq[q], thq[q], ul[q], ur[q]);
#pragma unroll
  for (int q = 0; q < G; ++q) {
    const int i = i0 + q;
    const double lf = l[q] + f.weight * field_lerp(tap[q]);
    if (TO_LDS) lds_loss[(i - a.lds_from) * kWave + lane] = lf;
    else J[(size_t)i * K + k] = lf;
  }
}

constexpr int kFieldAhead = 3;  // groups of noise requested ahead of the one being integrated (mppi_rollout_cost's kAhead)
// LDS carve (dynamic), as mppi_rollout_cost: u_lds [2*T], then the losses of steps lds_from .. T-1, [T - lds_from][64]
template <int TRIG>
__global__ __launch_bounds__(kWave) void mppi_rollout_field(RolloutArgs a, FieldArgs f, const double* __restrict__ duL, const double* __restrict__ duR,
                                                            USrc u, double* __restrict__ J) {
  extern __shared__ __attribute__((aligned(16))) double lds_all[];
  const int lane = threadIdx.x;
  const int T = a.T, K = a.K;
  double* u_lds = lds_all;
  double* lds_loss = lds_all + 2 * T;
  for (int t = lane; t < 2 * T; t += kWave) u_lds[t] = u.get(t >= T, t >= T ? t - T : t, T);
  __syncthreads();
  const int k = blockIdx.x * kWave + lane;
  if (k >= K) return;
  double x = a.x0[0], y = a.x0[1], th = a.x0[2];
  const int n_full = T / kGroup;
  const double* pl = duL + k;
  const double* pr = duR + k;
  double nl[kFieldAhead][kGroup], nr[kFieldAhead][kGroup];
#pragma unroll
  for (int r = 0; r < kFieldAhead; ++r) {
    if (r < n_full) {
#pragma unroll
      for (int q = 0; q < kGroup; ++q) {
        const size_t off = (size_t)(r * kGroup + q) * K;
        nl[r][q] = pl[off];
        nr[r][q] = pr[off];
      }
    }
  }
  for (int g0 = 0; g0 < n_full; g0 += kFieldAhead) {
#pragma unroll
    for (int r = 0; r < kFieldAhead; ++r) {   // ring slot r holds group g0 + r
      const int g = g0 + r;
      if (g < n_full) {
        double dl[kGroup], dr[kGroup];
#pragma unroll
        for (int q = 0; q < kGroup; ++q) { dl[q] = nl[r][q]; dr[q] = nr[r][q]; }
        if (g + kFieldAhead < n_full) {
#pragma unroll
          for (int q = 0; q < kGroup; ++q) {
            const size_t off = (size_t)((g + kFieldAhead) * kGroup + q) * K;
            nl[r][q] = pl[off];
            nr[r][q] = pr[off];
          }
        }
        if (g * kGroup >= a.lds_from) field_group<TRIG, kGroup, true>(a, f, g * kGroup, lane, k, x, y, th, dl, dr, u_lds, lds_loss, J);
        else field_group<TRIG, kGroup, false>(a, f, g * kGroup, lane, k, x, y, th, dl, dr, u_lds, lds_loss, J);
      }
    }
  }
  for (int i = n_full * kGroup; i < T; ++i) {  // ragged tail, one step at a time
    const double dl[1] = {pl[(size_t)i * K]}, dr[1] = {pr[(size_t)i * K]};
    if (i >= a.lds_from) field_group<TRIG, 1, true>(a, f, i, lane, k, x, y, th, dl, dr, u_lds, lds_loss, J);
    else field_group<TRIG, 1, false>(a, f, i, lane, k, x, y, th, dl, dr, u_lds, lds_loss, J);
  }
  // cumSumCost (mppi.cpp:15-25): J(i) = loss(i) + J(i+1), from the end, eight staged losses at a time with the next eight in flight
  double* Jk = J + k;
  const int lds_from = a.lds_from;
  auto staged = [&](int t) -> double { return t >= lds_from ? lds_loss[(t - lds_from) * kWave + lane] : Jk[(size_t)t * K]; };
  constexpr int kB = 8;
  double acc = 0.0;
  int i = T - 1;
  double cur[kB], nxt[kB];
  if (i >= kB - 1) {
#pragma unroll
    for (int q = 0; q < kB; ++q) cur[q] = staged(i - q);
  }
  for (; i >= kB - 1; i -= kB) {
    const bool more = (i - kB) >= kB - 1;
    if (more) {
#pragma unroll
      for (int q = 0; q < kB; ++q) nxt[q] = staged(i - kB - q);
    }
#pragma unroll
    for (int q = 0; q < kB; ++q) {
      acc = (i - q == T - 1) ? cur[q] : cur[q] + acc;
      Jk[(size_t)(i - q) * K] = acc;
    }
    if (more) {
#pragma unroll
      for (int q = 0; q < kB; ++q) cur[q] = nxt[q];
    }
  }
  for (; i >= 0; --i) {
    const double l = staged(i);
    acc = (i == T - 1) ? l : l + acc;
    Jk[(size_t)i * K] = acc;
  }
}
// (mppi_plan.hpp's list of forms: TRIG 2 takes the three-evaluation form here, as in the time-parallel kernel)
#define TBNAV_X(TR) template __global__ void mppi_rollout_field<TR>(RolloutArgs, FieldArgs, const double* __restrict__, const double* __restrict__, USrc, double* __restrict__);
TBNAV_MPPI_FIELD_FORMS(TBNAV_X)
#undef TBNAV_X

// the test hook's kernel: F2 through the rollout kernel's own two functions
__global__ void mppi_field_lookup(FieldArgs f, int n, const double* __restrict__ xy, double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  FieldTap t;
  field_gather(f, xy[2 * i], xy[2 * i + 1], t);
  out[i] = field_lerp(t);
}

}  // namespace tbnav_mk

using namespace tbnav_mh;

namespace {
FieldArgs field_args(const tbnav_mppi* h) {
  return FieldArgs{h->d_field, h->field.xmin, h->field.ymin, 1.0 / h->field.resolution, h->field.weight, h->field.nx, h->field.ny};
}
bool geom_ok(const tbnav_mppi_cost_field& g) {
  return g.nx >= 2 && g.nx <= TBNAV_MPPI_FIELD_MAX_SIDE && g.ny >= 2 && g.ny <= TBNAV_MPPI_FIELD_MAX_SIDE && std::isfinite(g.xmin) &&
         std::isfinite(g.ymin) && std::isfinite(g.resolution) && g.resolution > 0.0 && std::isfinite(g.weight);
}
}  // namespace

int tbnav_mh::launch_rollout_field(tbnav_mppi* h, const RolloutPlan& p, const RolloutArgs& a, const USrc& usrc, const double* d_duL, const double* d_duR, hipStream_t st) {
#define TBNAV_X(TR)                                                                                                                         \
  if (p.form.is(kField, TR)) {                                                                                                              \
    hipLaunchKernelGGL((mppi_rollout_field<TR>), dim3(p.grid), dim3(kWave), p.lds, st, a, field_args(h), d_duL, d_duR, usrc, h->d_J);       \
    TBNAV_HIP(hipGetLastError());                                                                                                           \
    return TBNAV_OK;                                                                                                                        \
  }
  TBNAV_MPPI_FIELD_FORMS(TBNAV_X)
#undef TBNAV_X
  return TBNAV_ERR_UNSUPPORTED;  // (a form the plan names and the list does not have: never another form in its place)
}

namespace {
// what both stagings share: the kernel's dynamic LDS allowed for this handle, and room for the values on its device (current here)
int field_alloc(tbnav_mppi* h, size_t n, float** d) {
  // the kernel's dynamic LDS, as tbnav_mppi_create allows it for mppi_rollout_cost (lds_from only ever grows afterwards)
  const int lds_max = (int)staged_lds_bytes(h->T, h->lds_from);
#define TBNAV_X(TR) TBNAV_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&mppi_rollout_field<TR>), hipFuncAttributeMaxDynamicSharedMemorySize, lds_max));
  TBNAV_MPPI_FIELD_FORMS(TBNAV_X)
#undef TBNAV_X
  TBNAV_HIP(hipMalloc((void**)d, n * sizeof(float)));
  return TBNAV_OK;
}
}  // namespace

int tbnav_mh::field_stage(tbnav_mppi* h, const tbnav_mppi_cost_field* geom, const float* values_host, float** d_new) {
  if (!h || !d_new) return TBNAV_ERR_INVALID_ARG;
  *d_new = nullptr;
  if (!geom) return TBNAV_OK;
  if (!values_host || !geom_ok(*geom)) return TBNAV_ERR_INVALID_ARG;
  const size_t n = (size_t)geom->nx * geom->ny;
  for (size_t i = 0; i < n; ++i) if (!std::isfinite(values_host[i])) return TBNAV_ERR_INVALID_ARG;
  DeviceGuard guard(h->device);
  if (!guard.ok) return TBNAV_ERR_NO_DEVICE;
  float* d = nullptr;
  const int rc = field_alloc(h, n, &d);
  if (rc != TBNAV_OK) return rc;
  const hipError_t e = hipMemcpy(d, values_host, n * sizeof(float), hipMemcpyHostToDevice);
  if (e != hipSuccess) { (void)hipFree(d); TBNAV_HIP(e); }
  *d_new = d;
  return TBNAV_OK;
}

int tbnav_mh::field_stage_device(tbnav_mppi* h, const tbnav_mppi_cost_field& geom, const float* d_values, int src_device, float** d_new) {
  if (!h || !d_new || !d_values || !geom_ok(geom)) return TBNAV_ERR_INVALID_ARG;
  *d_new = nullptr;
  const size_t n = (size_t)geom.nx * geom.ny;
  DeviceGuard guard(h->device);
  if (!guard.ok) return TBNAV_ERR_NO_DEVICE;
  float* d = nullptr;
  const int rc = field_alloc(h, n, &d);
  if (rc != TBNAV_OK) return rc;
  const hipError_t e = src_device == h->device ? hipMemcpy(d, d_values, n * sizeof(float), hipMemcpyDeviceToDevice)
                                               : hipMemcpyPeer(d, h->device, d_values, src_device, n * sizeof(float));
  if (e != hipSuccess) { (void)hipFree(d); TBNAV_HIP(e); }
  *d_new = d;
  return TBNAV_OK;
}

int tbnav_mh::field_commit(tbnav_mppi* h, const tbnav_mppi_cost_field* geom, float* d_new) {
  DeviceGuard guard(h->device);
  const hipError_t e = hipDeviceSynchronize();   // (a queued tick may still read the old values)
  if (e != hipSuccess) { (void)hipFree(d_new); TBNAV_HIP(e); }
  (void)hipFree(h->d_field);
  h->d_field = d_new;
  h->field_on = geom != nullptr;
  if (geom) h->field = *geom;
  ++h->cfg_epoch;   // (a graph of ticks captured before is rebuilt, never replayed)
  return TBNAV_OK;
}

extern "C" {

int tbnav_mppi_set_cost_field(tbnav_mppi* h, const tbnav_mppi_cost_field* geom, const float* values_host) {
  if (!h) return TBNAV_ERR_INVALID_ARG;
  float* d_new = nullptr;
  const int rc = field_stage(h, geom, values_host, &d_new);
  return rc != TBNAV_OK ? rc : field_commit(h, geom, d_new);
}

int tbnav_mppi_get_cost_field(const tbnav_mppi* h, int32_t* on, tbnav_mppi_cost_field* geom) {
  if (!h) return TBNAV_ERR_INVALID_ARG;
  if (on) *on = h->field_on ? 1 : 0;
  if (geom && h->field_on) *geom = h->field;
  return TBNAV_OK;
}

int tbnav_mppi_cost_field_lookup(tbnav_mppi* h, const double* xy, int32_t n, double* out) {
  if (!h || !xy || !out || n <= 0 || !h->field_on) return TBNAV_ERR_INVALID_ARG;
  DeviceGuard guard(h->device);
  double *dxy = nullptr, *dout = nullptr;
  hipError_t e = hipMalloc((void**)&dxy, sizeof(double) * 2 * (size_t)n);
  if (e == hipSuccess) e = hipMalloc((void**)&dout, sizeof(double) * (size_t)n);
  if (e == hipSuccess) e = hipMemcpy(dxy, xy, sizeof(double) * 2 * (size_t)n, hipMemcpyHostToDevice);
  if (e == hipSuccess) { hipLaunchKernelGGL(mppi_field_lookup, dim3((n + 255) / 256), dim3(256), 0, nullptr, field_args(h), n, dxy, dout); e = hipGetLastError(); }
  if (e == hipSuccess) e = hipMemcpy(out, dout, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost);
  (void)hipFree(dxy); (void)hipFree(dout);
  TBNAV_HIP(e);
  return TBNAV_OK;
}

}  // extern "C"

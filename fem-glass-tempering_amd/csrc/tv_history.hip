// Process schedules and on-device run histories of a single-problem context
// (tv_set_boundary, tv_set_schedule, tv_step_count, tv_history_open / _read),
// gfx950.  The ensembles' counterpart lives inside their step kernel
// (tv_ensemble_step.h); here a step is many launches, so the schedule is host
// state applied between steps and the history is three small launches queued
// behind a step's end:
//
//   k_history_gather    one thread per recorded probe value: T, Tf at the
//                       probes' T dofs, the bs = dim^2 components of sigma at
//                       their sigma dofs (device dof numbers, translated once
//                       at tv_history_open by k_history_map);
//   k_history_extrema   min / max over the owned dofs of T and of each sigma
//                       component: 1 + bs value streams (blockIdx.y), each read
//                       once by a grid-stride loop (four independent 8-byte
//                       loads per lane and trip, a wave's load one contiguous
//                       512-byte run), then a wave reduction (__shfl_xor) and
//                       LDS across the four waves; one (min, max) pair per
//                       workgroup;
//   k_history_finish    one workgroup per stream reduces its pairs into the
//                       record.
//
// min and max do not depend on the order of their operands once the order of
// the two zeros is fixed (-0 < +0) and NaNs are skipped, so the result is the
// same whatever the grid: bitwise np.nanmin / np.nanmax (an all-NaN stream
// gives NaN).  The records are written by ordinary vector stores; the second
// launch orders itself behind the first on the stream, so no arrival counter
// and no fence is needed.  Nothing here is read by the solve: a context without
// a schedule and without a history runs none of this file's kernels.
#include "tv_ctx.h"

namespace tv {
namespace {

constexpr int kHistBlocks = 192;  // workgroups per stream of the extrema pass (x up to 10 streams ~ 2K workgroups)
constexpr int kHistUnroll = 4;    // loads in flight per lane

// host dof number -> device index of one space (transfer()'s map: a DG space is
// [l][cell] on the device and cell-major on the host, a CG space is offset by
// the ghost planes below the owned ones)
struct DofMap {
  int nl;          // 2^dim for a DG space, 0 for CG
  int64_t ncell;   // owned cells (DG)
  int64_t off;     // first owned dof (CG)
};
__device__ __forceinline__ int64_t device_dof(const DofMap& m, int64_t dof) {
  return m.nl > 0 ? (dof % m.nl) * m.ncell + dof / m.nl : m.off + dof;
}

__global__ __launch_bounds__(kBlock) void k_history_map(int64_t* __restrict__ dofs, int n_probes, DofMap mT, DofMap mS) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < 2 * n_probes) dofs[i] = device_dof(i < n_probes ? mT : mS, dofs[i]);
}

struct HistFields {
  const double* T;      // component 0 of each field, local dof 0
  const double* Tf;
  const double* sigma;
  int64_t sS;           // component stride of sigma
  int bs;
  // the owned ranges (the extrema's streams)
  int64_t offT, nT, offS, nS;
};

__global__ __launch_bounds__(kBlock) void k_history_gather(HistFields f, const int64_t* __restrict__ dofs,
                                                           int n_probes, double* __restrict__ rec) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  const int P = n_probes;
  if (i >= P * (2 + f.bs)) return;
  double v;
  if (i < P) v = f.T[dofs[i]];
  else if (i < 2 * P) v = f.Tf[dofs[i - P]];
  else {
    const int j = i - 2 * P, p = j / f.bs, q = j - p * f.bs;
    v = f.sigma[(int64_t)q * f.sS + dofs[P + p]];
  }
  rec[i] = v;
}

// NaN-skipping min / max with -0 < +0 (fmin / fmax leave the zeros' order open)
__device__ __forceinline__ double nan_min(double a, double b) {
  if (b != b) return a;
  if (a != a) return b;
  if (a == b) return signbit(a) ? a : b;
  return a < b ? a : b;
}
__device__ __forceinline__ double nan_max(double a, double b) {
  if (b != b) return a;
  if (a != a) return b;
  if (a == b) return signbit(a) ? b : a;
  return a > b ? a : b;
}

// (mn, mx) over the workgroup; valid in thread 0
__device__ __forceinline__ void block_minmax(double& mn, double& mx) {
  __shared__ double smn[kBlock / 64], smx[kBlock / 64];
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    mn = nan_min(mn, __shfl_xor(mn, o, 64));
    mx = nan_max(mx, __shfl_xor(mx, o, 64));
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    smn[wave] = mn;
    smx[wave] = mx;
  }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < kBlock / 64; ++w) {
      mn = nan_min(mn, smn[w]);
      mx = nan_max(mx, smx[w]);
    }
}

__device__ __forceinline__ const double* stream_of(const HistFields& f, int s, int64_t& n) {
  n = s == 0 ? f.nT : f.nS;
  return s == 0 ? f.T + f.offT : f.sigma + (int64_t)(s - 1) * f.sS + f.offS;
}

// part[(s gridDim.x + b) 2 + {0, 1}] = (min, max) of workgroup b's share of stream s
__global__ __launch_bounds__(kBlock) void k_history_extrema(HistFields f, double* __restrict__ part) {
  int64_t n;
  const double* __restrict__ v = stream_of(f, blockIdx.y, n);
  const double nan = __longlong_as_double(-1LL);
  double mn = nan, mx = nan;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  int64_t t = blockIdx.x * (int64_t)kBlock + threadIdx.x;
  for (; t + (kHistUnroll - 1) * stride < n; t += kHistUnroll * stride) {
    double x[kHistUnroll];
#pragma unroll
    for (int u = 0; u < kHistUnroll; ++u) x[u] = v[t + u * stride];
#pragma unroll
    for (int u = 0; u < kHistUnroll; ++u) {
      mn = nan_min(mn, x[u]);
      mx = nan_max(mx, x[u]);
    }
  }
  for (; t < n; t += stride) {
    const double x = v[t];
    mn = nan_min(mn, x);
    mx = nan_max(mx, x);
  }
  block_minmax(mn, mx);
  if (threadIdx.x == 0) {
    double* p = part + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 2;
    p[0] = mn;
    p[1] = mx;
  }
}

// workgroup s: the nblk pairs of stream s -> ext = T_min T_max sigma_min[bs] sigma_max[bs]
__global__ __launch_bounds__(kBlock) void k_history_finish(const double* __restrict__ part, int nblk, int bs,
                                                           double* __restrict__ ext) {
  const int s = blockIdx.x;
  const double nan = __longlong_as_double(-1LL);
  double mn = nan, mx = nan;
  for (int b = threadIdx.x; b < nblk; b += kBlock) {
    const double* p = part + ((int64_t)s * nblk + b) * 2;
    mn = nan_min(mn, p[0]);
    mx = nan_max(mx, p[1]);
  }
  block_minmax(mn, mx);
  if (threadIdx.x == 0) {
    ext[s == 0 ? 0 : 2 + (s - 1)] = mn;
    ext[s == 0 ? 1 : 2 + bs + (s - 1)] = mx;
  }
}

int hist_blocks(const Ctx* c) {
  const int64_t n = std::max(c->ownT_n, c->ownS_n), per = (int64_t)kBlock * kHistUnroll;
  return (int)std::min<int64_t>(kHistBlocks, std::max<int64_t>(1, (n + per - 1) / per));
}

DofMap dof_map(const Ctx* c, int space) {
  const bool dg = (space == 0 ? c->fam_T : c->fam_S) == TV_DG;
  const int64_t n = space == 0 ? c->ownT_n : c->ownS_n;
  DofMap m{};
  m.nl = dg ? 1 << c->dim : 0;
  m.ncell = dg ? n / m.nl : 0;
  m.off = space == 0 ? c->ownT_off : c->ownS_off;
  return m;
}

// the stage (row of sch_val) of the 1-based step s: the first whose end is not before it
int stage_of(const Ctx* c, int64_t s) {
  int j = 0;
  while (j + 1 < c->sch_n && s > c->sch_end[(size_t)j]) ++j;
  return j;
}

const char* boundary_error(double htc, double Ta, double eps) {
  if (!std::isfinite(htc) || !std::isfinite(Ta) || !std::isfinite(eps)) return "htc, T_ambient and epsilon must be finite";
  if (htc < 0.0) return "htc must not be negative";
  if (eps < 0.0) return "epsilon must not be negative";
  return nullptr;
}

}  // namespace

void apply_boundary(Ctx* c, double htc, double T_ambient, double epsilon) {
  c->P.htc = htc;
  c->P.T_ambient = T_ambient;
  c->P.epsilon = epsilon;
  boundary_constants(c->cg, c->P);
  boundary_constants(c->dg, c->P);
  boundary_constants(c->umg, c->P);
  boundary_constants(c->udg.rb, c->P);
  for (MgLevel& L : c->mg) boundary_constants(L.g, c->P);  // distributed and replicated levels alike
}

int history_step_begin(Ctx* c) {
  const int64_t s = c->steps_done + 1;
  if (const History* h = c->hist)
    if (s > (int64_t)h->max_records * h->every)
      return c->fail(TV_ERR_STATE, "tv_step: step " + std::to_string(s) + " lies past the open history (max_records " +
                                       std::to_string(h->max_records) + " x every " + std::to_string(h->every) +
                                       "); nothing has advanced");
  if (c->sch_n > 0) {
    const size_t j = (size_t)stage_of(c, s);
    const double v[3] = {c->sch_val[0][j], c->sch_val[1][j], c->sch_val[2][j]};
    if (v[0] != c->P.htc || v[1] != c->P.T_ambient || v[2] != c->P.epsilon) apply_boundary(c, v[0], v[1], v[2]);
  }
  return TV_OK;
}

int history_step_end(Ctx* c, bool ended) {
  const int64_t s = ++c->steps_done;
  const History* h = c->hist;
  if (!h || !ended || s % h->every != 0) return TV_OK;
  const int64_t r = s / h->every - 1;
  if (r >= h->max_records) return TV_OK;  // (history_step_begin refused such a step)
  HistFields f{};
  f.T = c->f[TV_F_T].ptr;
  f.Tf = c->f[TV_F_TF].ptr;
  f.sigma = c->f[TV_F_SIGMA].ptr;
  f.sS = field_stride(c, 1);
  f.bs = h->bs;
  f.offT = c->ownT_off; f.nT = c->ownT_n;
  f.offS = c->ownS_off; f.nS = c->ownS_n;
  double* rec = h->rec + r * h->rec_len;
  const int nval = h->n_probes * (2 + h->bs), nblk = hist_blocks(c);
  hipLaunchKernelGGL(k_history_gather, dim3((nval + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream, f, h->dofs,
                     h->n_probes, rec);
  hipLaunchKernelGGL(k_history_extrema, dim3(nblk, 1 + h->bs), dim3(kBlock), 0, c->stream, f, h->part);
  hipLaunchKernelGGL(k_history_finish, dim3(1 + h->bs), dim3(kBlock), 0, c->stream, h->part, nblk, h->bs, rec + nval);
  HIPC(hipGetLastError());
  return TV_OK;
}

void history_free(Ctx* c) {
  History* h = c->hist;
  if (!h) return;
  if (h->rec) tv_dev_free(h->rec);
  if (h->part) tv_dev_free(h->part);
  if (h->dofs) tv_dev_free(h->dofs);
  delete h;
  c->hist = nullptr;
}

int history_reset(Ctx* c) {
  c->steps_done = 0;
  if (const History* h = c->hist)  // all bits set is a NaN: what a record reads until its step has written it
    HIPC(hipMemsetAsync(h->rec, 0xFF, sizeof(double) * (size_t)h->max_records * h->rec_len, c->stream));
  return TV_OK;
}

}  // namespace tv

using namespace tv;

extern "C" {

int tv_set_boundary(void* ctx, double htc, double T_ambient, double epsilon) {
  Ctx* c = static_cast<Ctx*>(ctx);
  if (!c) return TV_ERR_ARG;
  if (const char* e = boundary_error(htc, T_ambient, epsilon)) return c->fail(TV_ERR_ARG, std::string("tv_set_boundary: ") + e);
  apply_boundary(c, htc, T_ambient, epsilon);
  return TV_OK;
}


int tv_set_schedule(void* ctx, const tv_schedule* s) {
  Ctx* c = static_cast<Ctx*>(ctx);
  if (!c) return TV_ERR_ARG;
  if (!s) {  // back to the creation values
    c->sch_n = 0;
    c->sch_end.clear();
    for (auto& v : c->sch_val) v.clear();
    if (c->bnd0[0] != c->P.htc || c->bnd0[1] != c->P.T_ambient || c->bnd0[2] != c->P.epsilon)
      apply_boundary(c, c->bnd0[0], c->bnd0[1], c->bnd0[2]);
    return TV_OK;
  }
  auto bad = [&](const std::string& m) { return c->fail(TV_ERR_ARG, "tv_set_schedule: " + m); };
  const int nst = s->n_stages;
  if (nst < 1) return bad("n_stages must be at least 1");
  if ((nst == 1) != (s->stage_end == nullptr)) return bad("stage_end is NULL if and only if n_stages == 1");
  for (int j = 0, prev = 0; j + 1 < nst; ++j) {
    const int e = s->stage_end[j];
    if (e < 0) return bad("stage_end of stage " + std::to_string(j) + " is negative");
    if (e < prev) return bad("stage_end decreases at stage " + std::to_string(j));
    prev = e;
  }
  const double* tab[3] = {s->htc, s->T_ambient, s->epsilon};
  std::vector<double> val[3];
  for (int q = 0; q < 3; ++q) {
    val[q].resize((size_t)nst);
    for (int j = 0; j < nst; ++j) val[q][(size_t)j] = tab[q] ? tab[q][j] : c->bnd0[q];
  }
  for (int j = 0; j < nst; ++j)
    if (const char* e = boundary_error(val[0][(size_t)j], val[1][(size_t)j], val[2][(size_t)j]))
      return bad("stage " + std::to_string(j) + ": " + e);
  c->sch_n = nst;
  c->sch_end.assign(s->stage_end, s->stage_end + (nst - 1));
  for (int q = 0; q < 3; ++q) c->sch_val[q] = std::move(val[q]);
  return TV_OK;
}


int tv_step_count(void* ctx, int64_t* n) {
  Ctx* c = static_cast<Ctx*>(ctx);
  if (!c || !n) return TV_ERR_ARG;
  *n = c->steps_done;
  return TV_OK;
}


int tv_history_open(void* ctx, int n_probes, const int64_t* T_dofs, const int64_t* sigma_dofs, int every,
                    int max_records) {
  Ctx* c = static_cast<Ctx*>(ctx);
  if (!c) return TV_ERR_ARG;
  hipSetDevice(c->device);
  auto bad = [&](const std::string& m) { return c->fail(TV_ERR_ARG, "tv_history_open: " + m); };
  if (n_probes < 0) return bad("n_probes is negative");
  if (n_probes == 0) {  // close: the records go, the step cap with them
    HIPC(hipStreamSynchronize(c->stream));  // a queued record may still be writing
    history_free(c);
    return TV_OK;
  }
  if (!T_dofs || !sigma_dofs) return bad("T_dofs and sigma_dofs are both required");
  if (every < 1) return bad("every must be at least 1");
  if (max_records < 1) return bad("max_records must be at least 1");
  if ((int64_t)max_records * every > INT32_MAX - 1) return bad("max_records x every exceeds the step range");
  for (int p = 0; p < n_probes; ++p) {
    if (T_dofs[p] < 0 || T_dofs[p] >= c->ownT_n)
      return bad("probe " + std::to_string(p) + " (T dof " + std::to_string(T_dofs[p]) + ") lies outside [0, " +
                 std::to_string(c->ownT_n) + ")");
    if (sigma_dofs[p] < 0 || sigma_dofs[p] >= c->ownS_n)
      return bad("probe " + std::to_string(p) + " (sigma dof " + std::to_string(sigma_dofs[p]) + ") lies outside [0, " +
                 std::to_string(c->ownS_n) + ")");
  }
  auto h = std::make_unique<History>();
  h->n_probes = n_probes;
  h->every = every;
  h->max_records = max_records;
  h->bs = c->f[TV_F_SIGMA].bs;
  h->rec_len = (int64_t)n_probes * (2 + h->bs) + 2 + 2 * h->bs;
  if ((double)max_records * (double)h->rec_len > (double)(INT64_C(1) << 34)) return bad("history too large");
  const size_t rec_bytes = sizeof(double) * (size_t)max_records * (size_t)h->rec_len;
  const size_t part_bytes = sizeof(double) * 2 * (size_t)kHistBlocks * (size_t)(1 + h->bs);
  std::vector<int64_t> dofs(T_dofs, T_dofs + n_probes);
  dofs.insert(dofs.end(), sigma_dofs, sigma_dofs + n_probes);
  hipError_t e = tv_dev_alloc(&h->rec, rec_bytes, kMemDoubles);
  if (e == hipSuccess) e = tv_dev_alloc(&h->part, part_bytes, kMemDoubles);
  if (e == hipSuccess) e = tv_dev_alloc(&h->dofs, sizeof(int64_t) * dofs.size(), kMemOther);
  // all bits set is a NaN: what a record reads until its step has written it
  if (e == hipSuccess) e = hipMemsetAsync(h->rec, 0xFF, rec_bytes, c->stream);
  if (e == hipSuccess) e = hipMemsetAsync(h->part, 0xFF, part_bytes, c->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(h->dofs, dofs.data(), sizeof(int64_t) * dofs.size(), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(k_history_map, dim3((2 * n_probes + kBlock - 1) / kBlock), dim3(kBlock), 0, c->stream, h->dofs,
                       n_probes, dof_map(c, 0), dof_map(c, 1));
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);  // also: no record of the previous history in flight
  if (e != hipSuccess) {
    for (void* p : {(void*)h->rec, (void*)h->part, (void*)h->dofs})
      if (p) tv_dev_free(p);
    return c->fail(TV_ERR_HIP, std::string("tv_history_open: device setup failed: ") + hipGetErrorString(e));
  }
  history_free(c);
  c->hist = h.release();
  return TV_OK;
}


int tv_history_read(void* ctx, double* host, size_t n_values, int* n_records) {
  Ctx* c = static_cast<Ctx*>(ctx);
  if (!c) return TV_ERR_ARG;
  hipSetDevice(c->device);
  const History* h = c->hist;
  if (!h) return c->fail(TV_ERR_STATE, "tv_history_read: no history is open");
  const int nrec = (int)std::min<int64_t>(c->steps_done / h->every, h->max_records);
  if (n_records) *n_records = nrec;
  if (!host) {
    if (n_records) return TV_OK;  // a query of the record count
    return c->fail(TV_ERR_ARG, "tv_history_read: host and n_records are both null");
  }
  if (n_values < (size_t)nrec * (size_t)h->rec_len)
    return c->fail(TV_ERR_ARG, "tv_history_read: host holds fewer than n_records x rec_len values");
  if (nrec == 0) return TV_OK;
  HIPC(hipMemcpyAsync(host, h->rec, sizeof(double) * (size_t)nrec * (size_t)h->rec_len, hipMemcpyDeviceToHost,
                      c->stream));
  HIPC(hipStreamSynchronize(c->stream));
  return TV_OK;
}

}  // extern "C"

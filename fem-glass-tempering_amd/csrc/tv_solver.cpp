// The Newton + Krylov drivers of the heat solve and the viscoelastic step.
//   newton               dolfinx NewtonSolver::solve, incremental criterion,
//                        configured at ThermoViscoProblem.py:330-346 [3P]
//   krylov_drive         the queue-and-poll loop of the five Krylov solves:
//     pcg_solve              PETSc KSPSolve_CG + PCJACOBI restated on the device (here)
//     pcg_solve_cgs          its single-reduction (Chronopoulos-Gear) form (here)
//     pcg_solve_mg           GMG / AMG preconditioned, one partition (tv_mgsolve.cpp)
//     pcg_solve_mg_dist      distributed GMG, KSPCG form (tv_mgdist.cpp)
//     pcg_solve_mg_dist_cgs  distributed GMG, single-reduction form (tv_mgdist.cpp)
//   visco                _solve_Tf .. _solve_stress (ThermoViscoProblem.py:393-595)
#include <cstdlib>

#include "tv_ctx.h"

namespace tv {
// --------------------------------------------------------------------------------------
// operators
// --------------------------------------------------------------------------------------
void op_residual(Ctx* c, const double* T, const double* Tp, double* F) {
  if (c->um_dg) launch_umdg_residual(c->udg, T, Tp, F, c->stream);
  else if (c->um) launch_um_residual(c->umg, T, Tp, F, c->stream);
  else if (c->fam_T == TV_CG) launch_cg_residual(c->cg, T, Tp, F, c->stream);
  else launch_dg_residual(c->dg, T, Tp, F, c->stream);
}
void op_diag(Ctx* c, const double* T, double* d, int invert) {
  // Jacobian "assembly": the diagonal for the Jacobi PC (J(T) itself is matrix-free)
  if (c->um_dg) launch_umdg_diag(c->udg, T, d, invert, c->stream);
  else if (c->um) launch_um_diag(c->umg, T, d, invert, c->stream);
  else if (c->fam_T == TV_CG) launch_cg_diag(c->cg, T, d, invert, c->stream);
  else launch_dg_diag(c->dg, T, d, invert, c->stream);
}
void op_japply(Ctx* c, const double* T, const double* x, double* y, double* partials, int* np) {
  if (c->um_dg) launch_umdg_japply(c->udg, T, x, y, c->stream);
  else if (c->um) {  // (structured topology: the Robin terms at this T folded into the stencil first)
    launch_um_robin_fold(c->umg, T, c->stream);
    launch_um_japply(c->umg, T, x, y, c->stream);
  }
  else if (c->fam_T == TV_CG) launch_cg_japply(c->cg, T, x, y, partials, np, c->stream);
  else launch_dg_japply(c->dg, T, x, y, partials, np, c->stream);
}
bool op_japply_fused(Ctx* c, const double* T, int* np, const RedTail* tail, int it) {
  if (c->um_dg) {
    *np = launch_umdg_japply_fused(c->udg, T, c->z, c->pA, c->pB, c->w, c->st, c->partials, it, tail, c->stream);
    return tail && tail->counter;
  }
  if (c->um) {  // p <- z + b p, w <- J p, p.w and the reduction tail in one launch
    *np = launch_um_japply_fused(c->umg, T, c->z, c->pA, c->pB, c->w, c->st, c->partials, it, tail, c->stream);
    return tail && tail->counter;
  }
  if (c->fam_T == TV_CG)
    return launch_cg_japply_fused(c->cg, T, c->z, c->pA, c->pB, c->w, c->st, c->partials, np, c->stream, tail, it);
  return launch_dg_japply_fused(c->dg, T, c->z, c->pA, c->pB, c->w, c->st, c->partials, np, c->stream, tail);
}

// --------------------------------------------------------------------------------------
// Jacobi-PCG for J(T) dx = r  (PETSc KSPCG restated; see tv_pcg.hip)
// --------------------------------------------------------------------------------------
// it: index of this iteration within the solve (the device counter st->it
// equals it until convergence, after which every kernel exits at once)

// the scalars of a Krylov solve at its start (PETSc KSPSetTolerances); with
// ksp_fixed_its the solve runs exactly that many iterations (no convergence
// test: KSP_NORM_NONE), which newton() accepts
PcgState pcg_state_init(const Ctx* c) {
  PcgState h{};
  h.rtol = c->O.ksp_rtol;
  h.atol = c->O.ksp_atol;
  h.dtol = c->O.ksp_dtol;
  h.max_it = c->O.ksp_max_it;
  if (c->O.ksp_fixed_its > 0) {
    h.rtol = 0.0;
    h.atol = 0.0;
    h.dtol = 1e300;
    h.max_it = c->O.ksp_fixed_its;
    h.accept_its = 1;
    h.relaxed = c->comm_stub ? 1 : 0;
  }
  return h;
}

void solve_begin(Ctx* c, const double* gate) {
  const PcgState h = pcg_state_init(c);
  // from pinned memory (an asynchronous upload; a pageable source is staged by
  // the runtime -- no step-time change measured at C2 / C3 / C4)
  c->h_st[2] = h;
  launch_set_state(c->st, h, c->stream, gate);
}

// reads the pending timestamp slots back and adds them to the stats
int ts_flush(Ctx* c) {
  if (!c->d_ts) return TV_OK;
  if (!c->ts_pending.empty()) {
    std::vector<uint64_t> h((size_t)4 * c->ts_next);
    HIPC(hipMemcpyAsync(h.data(), c->d_ts, h.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    for (int sl : c->ts_pending) {
      const uint64_t* t = &h[(size_t)4 * sl];
      for (int k = 0; k < 2; ++k) {
        if (t[2 * k] == 0 || t[2 * k + 1] < t[2 * k]) continue;  // launch without a timed tail
        c->ksum[k] += (double)(t[2 * k + 1] - t[2 * k]) / c->ts_khz;
        c->kcnt[k] += 1;
      }
    }
    c->ts_pending.clear();
  }
  c->ts_next = 0;
  HIPC(hipMemsetAsync(c->d_ts, 0, (size_t)4 * kTsCap * sizeof(uint64_t), c->stream));
  return TV_OK;
}

uint64_t* iter_stamp(const Ctx* c, int it) {
  const int slot = c->ts_next + it;
  return (it >= 0 && c->ktime && (it % c->kstride) == 0 && slot < kTsCap) ? c->d_ts + 4 * slot : nullptr;
}

// The first batch goes into the stream right behind the solve's init, with no
// host wait in between; an init that already converged (or a solve gated off)
// makes every queued launch exit at its first instruction.  Each batch ends
// with the device state published to a pinned slot and an event, which the
// host polls.  Two disciplines (KrylovPolicy::ahead):
//   ahead   batches are queued one ahead of the convergence poll: while the
//           host waits for the state copied at the end of batch k, batch k + 1
//           is already in the stream (slots / events k & 1), so the GPU never
//           idles on the host's turnaround.  The batch queued behind the
//           converged one exits early; stream order covers it.
//   else    poll, then queue the next batch (slot 0 only).
// The first batch is sized by the count this Newton index took in the last
// step (the counts repeat from step to step, and decrease along a step's Newton
// iterations, so the previous solve's count -- pcg_hint, the fallback for an
// index not seen yet -- over-queues).  hipGetLastError is checked once per batch.
int krylov_drive(Ctx* c, const KrylovPolicy& p, KrylovIterate iterate, void* fi, KrylovPublished published, void* fp,
                 int* its, int* reason) {
  if (c->ktime && c->ts_next + p.ts_reserve > kTsCap)
    if (int e = ts_flush(c)) return e;
  int launched = 0;
  auto enqueue = [&](int nb, int k) -> int {
    for (int b = 0; b < nb; ++b)
      if (int e = iterate(fi, launched + b, b, nb)) return e;
    launched += nb;
    HIPC(hipGetLastError());
    if (int e = publish(c, &c->h_st[k], c->st, sizeof(PcgState))) return e;
    HIPC(hipEventRecord(c->evp[k], c->stream));
    return published(fp);
  };
  const int hk = std::min(c->newton_k, 15);
  const int hint = p.hints[hk] > 0 ? p.hints[hk] : c->pcg_hint;
  if (int e = enqueue(p.init_its + (hint > p.hint_min ? hint : p.first_default), 0)) return e;
  int slot = 0;
  for (;;) {
    if (p.ahead)
      if (int e = enqueue(p.next, slot ^ 1)) return e;
    HIPC(hipEventSynchronize(c->evp[slot]));
    if (c->h_st[slot].done) break;
    if (launched > p.guard) return c->fail(TV_ERR_KSP, "PCG: iteration guard exceeded");
    if (p.ahead) slot ^= 1;
    else if (int e = enqueue(p.next, 0)) return e;
  }
  *its = c->h_st[slot].it;
  *reason = c->h_st[slot].reason;
  // a solve gated off by the Newton test says nothing of the count (only the
  // multigrid solves are gated)
  if (*reason != R_SKIPPED) c->pcg_hint = p.hints[hk] = std::max(p.hint_floor, *its);
  if (c->ktime) {  // productive iterations only (launches queued behind convergence exit at once)
    for (int it = p.init_its; it < p.init_its + *its; it += c->kstride)
      if (c->ts_next + it < kTsCap) c->ts_pending.push_back(c->ts_next + it);
    c->ts_next = std::min(kTsCap, c->ts_next + launched);
  }
  return TV_OK;
}

// lag3: the beta / convergence logic of the previous closing group runs lagged
// inside this iteration's fused matvec (box march only); defer3: this
// iteration's closing logic is left to the next one the same way.  The alpha
// logic of a multi-rank iteration runs lagged inside the update.
int pcg_iteration(Ctx* c, const double* T, int it, bool lag3, bool defer3) {
  const int64_t off = c->ownT_off, n = c->ownT_n;
  // the matvec launchers without a reduction tail (DG, 1D/2D CG) leave their stamps at 0
  uint64_t* ts = iter_stamp(c, it);
  const bool multi = multi_rank(c);
  // single GPU: the last-arriving workgroup of each launch reduces the partial
  // records and runs the KSPCG scalar logic in-kernel (no separate reduce
  // launch); multi-GPU: it only reduces, RCCL all-reduces, then the logic runs.
  RedTail t1{c->counters, c->partials, c->sums, c->st, multi ? 0 : 2, ts};
  if (lag3) {
    t1.lag = c->sums;
    t1.lag_kind = 3;
  }
  int np = 0;
  const bool fused1 = op_japply_fused(c, T, &np, &t1, it);  // p <- z + b p ; w <- J p ; p.w
  RedTail t2{c->counters + kTailCounters, c->partials, c->sums, c->st, multi ? 0 : 3, ts ? ts + 2 : nullptr};
  if (!fused1) {
    if (lag3) return c->fail(TV_ERR_STATE, "lagged PCG logic without the fused march");
    if (int e = reduce_logic(c, np, 1, 2, 1)) return e;  // dpi, a
  } else if (multi) {
    if (int e = allreduce(c, c->sums, 1)) return e;
    t2.lag = c->sums;  // alpha, inside the update
    t2.lag_kind = 2;
  }
  const FaceAdd fa = (c->fam_T == TV_CG && !c->um) ? cg_face_add(c->cg, off) : FaceAdd{};
  launch_pcg_update(n, c->st, c->pA + off, c->pB + off, c->w + off, c->dinv + off, c->f[TV_F_DX].ptr + off,
                    c->z + off, c->partials, c->stream, &t2, &fa, it);
  if (multi) {  // dp, beta, convergence; the ghosts of z in the same RCCL group
    if (int e = allreduce_halo(c, c->sums, 2, c->z)) return e;
    if (!defer3) launch_logic(c->st, c->sums, 3, c->stream);
  }
  return TV_OK;
}

int pcg_solve(Ctx* c, const double* T, int* its, int* reason) {
  const int64_t off = c->ownT_off, n = c->ownT_n;
  solve_begin(c);
  launch_pcg_init(n, c->r + off, c->dinv + off, c->z + off, c->f[TV_F_DX].ptr + off, c->partials, c->stream);
  if (int e = reduce_logic(c, pcg_vec_blocks(n), 2, 1, 0)) return e;
  if (int e = halo(c, c->z)) return e;
  KrylovPolicy p{};
  p.ahead = true;
  // first batch: this Newton index's count in the last step (measured: previous
  // count - 3 C2 0.97-0.99 ms, this index's count - 1 0.90-0.92, its count
  // 0.88-0.89); a hint of 4 or less gives way to pcg_batch
  p.hints = c->jac_hint;
  p.hint_min = 4;
  p.first_default = std::max(1, c->O.pcg_batch);
  // batches queued behind the first: pcg_batch / 8 iterations (1 by default);
  // the host's turnaround (~30 us) is well inside one iteration (~130 us at C4),
  // and every iteration queued past convergence costs two early-exit launches
  p.next = std::max(1, c->O.pcg_batch / 8);
  p.guard = c->O.ksp_max_it + 2 * p.next + 2;
  p.ts_reserve = c->O.ksp_max_it + 4 * c->O.pcg_batch + 8;
  // multi-rank box march: the closing logic of an iteration runs lagged in the
  // next one's fused matvec, except after a batch's last iteration (polled)
  const bool fold = multi_rank(c) && !c->um && c->fam_T == TV_CG && cg_cgs_supported(c->cg);
  auto iterate = [&](int it, int b, int nb) { return pcg_iteration(c, T, it, fold && b > 0, fold && b + 1 < nb); };
  if (int e = krylov_drive(c, p, iterate, [] { return TV_OK; }, its, reason)) return e;
  launch_pcg_dx_tail(n, c->st, c->pA + off, c->pB + off, c->f[TV_F_DX].ptr + off, *its, c->stream);
  return TV_OK;
}

CgsBuffers cgs_buffers(Ctx* c, const double* T, int it) {
  // iteration it reads parity (it - 1) & 1 and writes it & 1; r_0 is the Newton
  // residual (c->r), read by iterations 0 and 1
  CgsBuffers v{};
  const int o = (it + 1) & 1, w = it & 1;
  double* W[2] = {c->w, c->cw1};
  v.T = T;
  v.rin = (it <= 1) ? c->r : c->cr[o];
  v.rout = c->cr[w];
  v.sin = c->cs[o];
  v.sout = c->cs[w];
  v.win = W[o];
  v.wout = W[w];
  v.fin = c->cg.ffbuf[o];
  v.fout = c->cg.ffbuf[w];
  v.p = c->pA;
  v.x = c->f[TV_F_DX].ptr;
  v.dinv = c->dinv;
  return v;
}

int cgs_iteration(Ctx* c, const double* T, int it) {
  const bool multi = multi_rank(c);
  const int kind = multi ? 0 : (it == 0 ? 4 : 5);
  RedTail rt{c->counters, c->partials, c->sums, c->st, kind, iter_stamp(c, it)};
  const CgsBuffers v = cgs_buffers(c, T, it);
  launch_cg_cgs(c->cg, it == 0, v, c->st, c->partials, c->stream, &rt, it, (multi && it > 0) ? c->sums : nullptr);
  if (multi)
    if (int e = cgs_exchange(c, v.wout, v.fout)) return e;
  return TV_OK;
}

int pcg_solve_cgs(Ctx* c, const double* T, int* its, int* reason) {
  solve_begin(c);
  // ghost planes of r_0 and diag^-1 (the halo rows recompute z there)
  if (int e = halo(c, c->r)) return e;
  if (int e = halo(c, c->dinv)) return e;
  // as pcg_solve, but iteration 0 is the init launch: it goes with the first
  // batch, then one more iteration is queued behind every poll; multi-rank the
  // state lags one launch
  KrylovPolicy p{};
  p.ahead = true;
  p.hints = c->jac_hint;
  p.hint_min = 4;
  p.first_default = std::max(1, c->O.pcg_batch);
  p.init_its = 1;
  p.next = 1 + (multi_rank(c) ? 1 : 0);
  p.guard = c->O.ksp_max_it + 2 * p.next + 4;
  p.ts_reserve = c->O.ksp_max_it + 4 * c->O.pcg_batch + 8;
  auto iterate = [&](int it, int, int) { return cgs_iteration(c, T, it); };
  return krylov_drive(c, p, iterate, [] { return TV_OK; }, its, reason);
}

const char* reason_str(int r) {
  switch (r) {
    case R_DIV_ITS: return "DIVERGED_ITS";
    case R_DIV_DTOL: return "DIVERGED_DTOL";
    case R_DIV_INDEF_PC: return "DIVERGED_INDEFINITE_PC";
    case R_DIV_NANINF: return "DIVERGED_NANORINF";
    case R_DIV_INDEF_MAT: return "DIVERGED_INDEFINITE_MAT";
    default: return "UNKNOWN";
  }
}

// ---- Dirichlet mode ----------------------------------------------------------
struct BndTest {
  CgGrid g;
  const unsigned char* mask;  // unstructured: boundary vertices (else nullptr)
};
__device__ __forceinline__ bool cg_on_boundary(const CgGrid& g, int64_t n);
__device__ __forceinline__ bool on_boundary(const BndTest& b, int64_t n) {
  return b.mask ? b.mask[n] != 0 : cg_on_boundary(b.g, n);
}
__device__ __forceinline__ bool cg_on_boundary(const CgGrid& g, int64_t n) {
  const int64_t plane = (int64_t)g.n0 * g.n1;
  const int k = (int)(n / plane);
  const int64_t rem = n - (int64_t)k * plane;
  const int j = (int)(rem / g.n0), i = (int)(rem - (int64_t)j * g.n0);
  return (i == 0 && g.bnd[0][0]) || (i == g.n0 - 1 && g.bnd[0][1]) || (j == 0 && g.bnd[1][0]) ||
         (j == g.n1 - 1 && g.bnd[1][1]) || (k == 0 && g.bnd[2][0]) || (k == g.n2 - 1 && g.bnd[2][1]);
}
// dB = T - value on constrained nodes, 0 elsewhere (every local node)
__global__ __launch_bounds__(kBlock) void k_bc_dvec(BndTest b, const double* __restrict__ T, double value,
                                                    double* __restrict__ dB, int64_t n) {
  for (int64_t t = blockIdx.x * (int64_t)kBlock + threadIdx.x; t < n; t += (int64_t)gridDim.x * kBlock)
    dB[t] = on_boundary(b, t) ? T[t] - value : 0.0;
}
// F -= J dB (lifting; the constrained rows are never read: diag^-1 = 0 there)
// and diag^-1 = 0 on constrained nodes, so z = B r and every Krylov vector
// stay in the free subspace: PCG on P J P with the Jacobi preconditioner P B P
__global__ __launch_bounds__(kBlock) void k_bc_lift(BndTest b, double* __restrict__ F, const double* __restrict__ JdB,
                                                    double* __restrict__ dinv, int64_t n) {
  for (int64_t t = blockIdx.x * (int64_t)kBlock + threadIdx.x; t < n; t += (int64_t)gridDim.x * kBlock) {
    F[t] -= JdB[t];
    if (on_boundary(b, t)) dinv[t] = 0.0;
  }
}
// dinv = 0 on the constrained rows only (tv_precond_apply: the solve's preconditioner)
__global__ __launch_bounds__(kBlock) void k_bc_mask(BndTest b, double* __restrict__ dinv, int64_t n) {
  for (int64_t t = blockIdx.x * (int64_t)kBlock + threadIdx.x; t < n; t += (int64_t)gridDim.x * kBlock)
    if (on_boundary(b, t)) dinv[t] = 0.0;
}
// dx += dB (the constrained part of the Newton step: x - dx lands on the value)
__global__ __launch_bounds__(kBlock) void k_bc_step(double* __restrict__ dx, const double* __restrict__ dB, int64_t n) {
  for (int64_t t = blockIdx.x * (int64_t)kBlock + threadIdx.x; t < n; t += (int64_t)gridDim.x * kBlock) dx[t] += dB[t];
}

void launch_bc_mask(Ctx* c, double* dinv) {
  const int64_t n = c->nT;
  const BndTest bt{c->cg, c->um ? c->um_bmask : nullptr};
  hipLaunchKernelGGL(k_bc_mask, dim3((int)std::min<int64_t>(4096, (n + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                     c->stream, bt, dinv, n);
}

int dirichlet_pre(Ctx* c, const double* T) {
  const int64_t n = c->nT;
  const int blocks = (int)std::min<int64_t>(4096, (n + kBlock - 1) / kBlock);
  const BndTest bt{c->cg, c->um ? c->um_bmask : nullptr};
  hipLaunchKernelGGL(k_bc_dvec, dim3(blocks), dim3(kBlock), 0, c->stream, bt, T, c->dir_value, c->dB, n);
  // ghosts from their owners (a partitioned unstructured mesh marks only its
  // owned boundary vertices; the box's ghost planes agree either way)
  if (int e = halo(c, c->dB)) return e;
  op_japply(c, T, c->dB, c->dtmp, nullptr, nullptr);
  hipLaunchKernelGGL(k_bc_lift, dim3(blocks), dim3(kBlock), 0, c->stream, bt, c->r, c->dtmp, c->dinv, n);
  HIPC(hipGetLastError());
  return TV_OK;
}

// Host-visible copies of the solver's scalars (the PCG state for the convergence
// polls, ||dx||^2 and the Newton decision) written by a one-wave kernel with
// system-scope stores straight into the pinned host slot, instead of a
// hipMemcpyAsync: a copy in the stream left the GPU idle ~5 us each (C4 trace:
// the gaps before the post-solve group and before every residual), a launch
// costs ~1.5 us (profiles/r06_launch_audit.json).  TVFEM_PUBLISH=0: the copies.
__global__ void k_publish(const uint32_t* __restrict__ src, uint32_t* dst, int n) {
  const int t = threadIdx.x;
  if (t < n) __hip_atomic_store(dst + t, src[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

int publish(Ctx* c, void* host_dst, const void* dev_src, size_t bytes) {
  static const bool on = [] {
    const char* e = std::getenv("TVFEM_PUBLISH");
    return e == nullptr || std::atoi(e) != 0;
  }();
  if (!on || bytes % 4 != 0 || bytes > 4 * 256) {
    HIPC(hipMemcpyAsync(host_dst, dev_src, bytes, hipMemcpyDeviceToHost, c->stream));
    return TV_OK;
  }
  hipLaunchKernelGGL(k_publish, dim3(1), dim3(256), 0, c->stream, static_cast<const uint32_t*>(dev_src),
                     static_cast<uint32_t*>(host_dst), (int)(bytes / 4));
  HIPC(hipGetLastError());
  return TV_OK;
}

// the Newton test on the device (one thread): the only place the decision is
// taken -- the gated step-end launches and a solve queued ahead of the host's
// read (k_set_state) read out[1], the host copies it.  Iteration 1 records
// r0^2 = ||dx_1||^2 (no test there, dolfinx's incremental criterion)
__global__ void k_newton_test(const double* __restrict__ nrm2, double* __restrict__ r0sq, int first, double rtol,
                              double atol, double* __restrict__ out) {
  if (threadIdx.x == 0) {
    const double v = *nrm2;
    out[0] = v;
    if (first) {
      *r0sq = v;
      out[1] = 0.0;
    } else {
      const double rn = sqrt(v), r0 = sqrt(*r0sq);
      out[1] = ((rn / r0 < rtol) || (rn < atol)) ? 1.0 : 0.0;
    }
  }
}

int queue_newton_norm(Ctx* c, const double* nrm2) {
  c->nrm_dev = nrm2;
  const int sl = c->newton_slot;
  double* out = c->ngate + 2 * sl;
  hipLaunchKernelGGL(k_newton_test, dim3(1), dim3(64), 0, c->stream, nrm2, c->ngate + 4, c->newton_first ? 1 : 0,
                     c->O.newton_rtol, c->O.newton_atol, out);
  if (int e = publish(c, c->h_sums + 2 * sl, out, 2 * sizeof(double))) return e;
  c->gate_dev = c->newton_first ? nullptr : out + 1;
  HIPC(hipEventRecord(c->evn[sl], c->stream));
  return TV_OK;
}

// the end of a time step (tv_step): the visco update with T_prev <- T, or the
// copy alone (thermal only), optionally gated on the device's Newton test; the
// visco update's HIP events bracket it (the previous pair is read first: it is
// long done by now, and reading it at the step's start made the host wait for
// the previous update -- an 18 us gap before the step's first residual)
int queue_step_end(Ctx* c, int step_end, const NewtonGate& gate) {
  if (step_end == 2) {
    if (gate.flag) launch_copy_gated(c->f[TV_F_T_PREV].ptr, c->f[TV_F_T].ptr, c->nT, gate, c->stream);
    else launch_copy(c->f[TV_F_T_PREV].ptr, c->f[TV_F_T].ptr, c->nT, c->stream);
    return TV_OK;
  }
  if (int e = visco_timing_flush(c)) return e;
  if (c->ktime) HIPC(hipEventRecord(c->vev[0], c->stream));
  if (int e = visco(c, true, gate)) return e;  // includes T_prev <- T (ThermoViscoProblem.py:378-379)
  if (c->ktime) {
    HIPC(hipEventRecord(c->vev[1], c->stream));
    c->vev_pending = true;  // read at the next step / tv_kernel_stats (no host wait here)
  }
  return TV_OK;
}

// dolfinx NewtonSolver::solve, convergence_criterion = "incremental"
int newton(Ctx* c, int* out_its, int* out_kits, int* out_conv, int step_end, bool* end_queued) {
  if (end_queued) *end_queued = false;
  if (int e = require_comm(c, "Newton solve")) return e;
  if (int e = refresh_dirty_ghosts(c)) return e;
  if (c->um && c->n_parts > 1 && c->O.preconditioner == TV_PC_AMG && !c->amg_on)
    if (int e = amg_setup_part(c)) return e;
  double* T = c->f[TV_F_T].ptr;
  const double* Tp = c->f[TV_F_T_PREV].ptr;
  // NonlinearProblem.form: ghost update of the state before the first F
  // (ThermoViscoProblem.py:351 scatter_forward); every rank enters it, every step
  if (int e = halo(c, T)) return e;
  if (int e = halo(c, c->f[TV_F_T_PREV].ptr)) return e;
  const int64_t off = c->ownT_off, n = c->ownT_n;
  int its = 0, kits = 0;  // its: Newton iterations whose test the host has read
  bool conv = false;
  double rn = 0.0;
  c->gate_dev = nullptr;
  c->solve_gate = nullptr;
  // F(u); on the CG march path the residual's boundary pass also rewrites the
  // boundary rows of dinv for the same u once the interior is in place
  auto residual = [&]() -> bool {
    if (!c->um && c->fam_T == TV_CG && c->dinv_interior)
      if (launch_cg_residual_diag(c->cg, T, Tp, c->r, c->dinv, c->stream)) return true;
    op_residual(c, T, Tp, c->r);
    return false;
  };
  // the host's read of Newton iteration q's test (its slot's event has fired
  // once a later launch's poll returned): ||dx||, the device's decision
  auto read_test = [&](int q) -> int {
    HIPC(hipEventSynchronize(c->evn[q & 1]));
    rn = std::sqrt(c->h_sums[2 * (q & 1)]);
    ++its;
    conv = q > 0 && c->h_sums[2 * (q & 1) + 1] != 0.0;  // no test at the first iteration
    return TV_OK;
  };
  bool dinv_fresh = residual();
  int q = 0;          // Newton iterations queued
  int pending = -1;   // a queued iteration whose test the host has not read yet
  for (;;) {
    level0_setup(c, T, dinv_fresh);  // the preconditioner's B at u
    if (c->um && !c->um_dg) launch_um_robin_fold(c->umg, T, c->stream);  // J(u) of the solve (structured topology)
    dinv_fresh = false;
    const bool dir = c->dir_on && c->fam_T == TV_CG;
    if (dir)
      if (int e = dirichlet_pre(c, T)) return e;
    int k = 0, reason = 0;
    c->newton_k = q;  // the multigrid solves queue the count this Newton index took last step
    c->newton_slot = q & 1;
    c->newton_first = q == 0;
    // multigrid (one partition or distributed): the post-solve group (dx,
    // u <- u - dx, ||dx||) is queued behind every batch and runs behind the
    // one that ends the solve, and only if it ended well (post_gate)
    const bool post_in_solve = c->mg_on && !dir;
    // a solve queued before the host read the previous iteration's test runs
    // only if that test did not end the Newton solve (iteration 1 has no test)
    c->solve_gate = pending >= 1 ? c->ngate + 2 * (pending & 1) + 1 : nullptr;
    const int e_solve = c->mg_on ? (c->n_parts > 1 ? pcg_solve_mg_dist(c, T, &k, &reason, post_in_solve)
                                                   : pcg_solve_mg(c, T, &k, &reason, post_in_solve))
                                 : (c->cgs ? pcg_solve_cgs(c, T, &k, &reason) : pcg_solve(c, T, &k, &reason));
    c->solve_gate = nullptr;
    if (e_solve) return e_solve;
    if (pending >= 0) {
      if (int e = read_test(pending)) return e;
      pending = -1;
      if ((reason == R_SKIPPED) != conv)
        return c->fail(TV_ERR_STATE, "Newton: a solve queued ahead disagrees with the Newton test (internal)");
      if (conv) break;  // that solve was gated off on the device: T is the converged iterate
    }
    kits += k;
    if (reason < 0 && !(reason == R_DIV_ITS && c->O.ksp_fixed_its > 0))
      return c->fail(TV_ERR_KSP, std::string("Krylov solver did not converge (") + reason_str(reason) + ")");
    if (dir)
      hipLaunchKernelGGL(k_bc_step, dim3((int)std::min<int64_t>(4096, (c->nT + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                         c->stream, c->f[TV_F_DX].ptr, c->dB, c->nT);
    // u <- u - dx; ||dx||^2 by a separate one-block reduce (a reduction tail on
    // the update's 1024 workgroups measured 7 us slower: 1024 serialised arrivals)
    if (!post_in_solve) {
      launch_newton_update(n, T + off, c->f[TV_F_DX].ptr + off, c->partials, c->stream);
      if (int e = reduce_logic(c, pcg_vec_blocks(n), 1, 0, 0)) return e;
      if (int e = queue_newton_norm(c, c->sums)) return e;
    }
    if (int e = halo(c, T)) return e;
    ++q;
    // the next F queued before the host reads ||dx|| when the previous step
    // took more Newton iterations than this one has so far (the counts repeat
    // from step to step): the GPU does not idle through the host's turnaround.
    // A wrong guess costs one residual, whose result is simply not used.
    const bool spec = q < c->newton_pred && q < c->O.newton_max_it;
    if (spec) dinv_fresh = residual();
    // ... and on the multigrid paths the next iteration's solve too, gated on
    // the device's test of this one (k_set_state): the host reads this test
    // after that solve's first poll, so it never waits at a Newton boundary
    // with the GPU drained (the C4 trace showed the GPU catching up with the
    // host's enqueue of the next solve's first V-cycle there).  A wrong guess
    // costs one batch of launches that exit at once.
    if (spec && post_in_solve && c->newton_ahead) {
      pending = q - 1;
      continue;
    }
    // at (or past) the iteration the last step ended with, the step's end is
    // queued now, gated on the device's test of this iteration (k_newton_test);
    // the host below takes the SAME decision (the flag copied with ||dx||^2), so
    // a gated-off launch is simply not used.  A solve that ends unconverged never
    // runs the step end (_solve_T's assert(converged), ThermoViscoProblem.py:390,
    // fires before _solve_Tf and the stress updates)
    bool end_q = false;
    if (step_end && !spec && q >= 2 && q >= c->newton_pred && c->gate_dev) {
      if (int e = queue_step_end(c, step_end, NewtonGate{c->gate_dev})) return e;
      end_q = true;
    }
    // the host waits for ||dx|| only, not for the queued residual: it decides
    // and queues the next Newton iteration while the GPU computes F (the C4
    // trace showed the GPU idle ~27 us per Newton iteration behind a stream sync)
    if (int e = read_test(q - 1)) return e;
    if (end_q) {
      if (conv) *end_queued = true;
      else c->vev_pending = false;  // gated off: its events bracket nothing
    }
    if (conv || its >= c->O.newton_max_it) break;
    // dolfinx assembles F after every update; in the incremental criterion that
    // last F is never read, so it is assembled only when another iteration follows.
    if (!spec) dinv_fresh = residual();
  }
  HIPC(hipGetLastError());
  c->newton_pred = its;
  c->last_newton = its;
  c->last_krylov = kits;
  c->last_dx = rn;
  c->last_conv = conv ? 1 : 0;
  if (out_its) *out_its = its;
  if (out_kits) *out_kits = kits;
  if (out_conv) *out_conv = conv ? 1 : 0;
  if (!conv && c->O.error_on_nonconvergence)
    return c->fail(TV_ERR_NOT_CONVERGED, "Newton solver did not converge because maximum number of iterations reached");
  return TV_OK;
}

// --------------------------------------------------------------------------------------
// viscoelastic update
// --------------------------------------------------------------------------------------
// the visco update's HIP-event timing of the last step, once its events have fired
int visco_timing_flush(Ctx* c) {
  if (!c->vev_pending) return TV_OK;
  HIPC(hipEventSynchronize(c->vev[1]));
  float a = 0.f;
  HIPC(hipEventElapsedTime(&a, c->vev[0], c->vev[1]));
  c->ksum[2] += a;
  c->kcnt[2] += 1;
  c->vev_pending = false;
  return TV_OK;
}

void fill_visco_const(ViscoConst& k, const tv_params& P, int dim, int model) {
  k.H_over_Rg = P.H / P.Rg;
  k.inv_Tb = 1.0 / P.Tb;
  k.dt = P.dt;
  k.half_dt = P.dt / 2;
  k.alpha_s = P.alpha_solid;
  k.dalpha = P.alpha_liquid - P.alpha_solid;
  k.inv_dim = 1.0 / dim;
  k.chi = 0.5;  // ViscoelasticModel.py:15
  k.paper = model;
  for (int i = 0; i < 6; ++i) {
    k.lambda_m[i] = P.lambda_m[i]; k.m_n[i] = P.m_n[i];
    k.lambda_g[i] = P.lambda_g[i]; k.g_n[i] = P.g_n[i];
    k.lambda_k[i] = P.lambda_k[i]; k.k_n[i] = P.k_n[i];
  }
}

void visco_setup(Ctx* c, ViscoConst& k, ViscoFields& v) {
  // model id (ViscoConst::paper): tv_set_relaxation admits TV_RELAX_EXACT on paper contexts only
  const int model = (c->O.model_mode == TV_MODEL_PAPER) ? (c->relaxation == TV_RELAX_EXACT ? 2 : 1) : 0;
  fill_visco_const(k, c->P, c->dim, model);
  std::memset(&v, 0, sizeof(v));
  v.sT = field_stride(c, 0);
  v.sS = field_stride(c, 1);
  v.T = c->f[TV_F_T].ptr; v.Tp = c->f[TV_F_T_PREV].ptr; v.Tn = c->f[TV_F_T_NEXT].ptr;
  v.phi = c->f[TV_F_PHI].ptr; v.phin = c->f[TV_F_PHI_NEXT].ptr; v.xi = c->f[TV_F_XI].ptr;
  v.Tf = c->f[TV_F_TF].ptr; v.Tfp = c->f[TV_F_TF_PARTIAL].ptr;
  v.th = c->f[TV_F_THERMAL_STRAIN].ptr; v.tot = c->f[TV_F_TOTAL_STRAIN].ptr; v.dev = c->f[TV_F_DEVIATORIC_STRAIN].ptr;
  v.ds = c->f[TV_F_DS_PARTIAL].ptr; v.dsig = c->f[TV_F_DSIGMA_PARTIAL].ptr;
  v.st = c->f[TV_F_S_TILDE].ptr; v.sgt = c->f[TV_F_SIGMA_TILDE].ptr;
  v.sp = c->f[TV_F_S_PARTIAL].ptr; v.sgp = c->f[TV_F_SIGMA_PARTIAL].ptr;
  v.sigma = c->f[TV_F_SIGMA].ptr;
  v.tflag = c->tflag;
  v.Tfo = c->Tfo;
}

int visco(Ctx* c, bool copy_Tprev, const NewtonGate& gate) {
  ViscoConst k;
  ViscoFields v;
  visco_setup(c, k, v);
  v.gate = gate;
  auto copy = [&](double* d, const double* s, int64_t n) {
    if (gate.flag) launch_copy_gated(d, s, n, gate, c->stream);
    else launch_copy(d, s, n, c->stream);
  };
  const int all = c->O.materialize ? 1 : 0;
  if (c->um && c->n_parts > 1) {
    // partitioned unstructured mesh: every local vertex, ghosts included (their
    // T is exchanged after each Newton update and the update is pointwise, so
    // they evolve exactly as on their owners: the output writes the local cells'
    // vertices without a further exchange)
    v.n = c->nT;
    v.off_T = v.off_S = 0;
    v.copy_Tprev = copy_Tprev ? 1 : 0;
    launch_visco(c->dim, all, k, v, c->stream);
  } else if (c->fam_T == c->fam_S) {
    v.n = c->ownT_n;
    v.off_T = c->ownT_off;
    v.off_S = c->ownS_off;
    v.copy_Tprev = copy_Tprev ? 1 : 0;
    launch_visco(c->dim, all, k, v, c->stream);
    if (copy_Tprev && c->ownT_off > 0) {  // ghost planes of T_prev
      copy(v.Tp, v.T, c->ownT_off);
    }
    if (copy_Tprev && c->nT > c->ownT_off + c->ownT_n) {
      const int64_t o = c->ownT_off + c->ownT_n;
      copy(v.Tp + o, v.T + o, c->nT - o);
    }
  } else {
    // mixed families; on a slab partition (setup_mixed_part) the T pass covers
    // the ghost dofs too (the sigma pass reads them at the slab's upper plane)
    // and the sigma pass every local sigma dof
    v.n = c->mixed_part ? c->nT : c->ownT_n;
    v.off_T = c->mixed_part ? 0 : c->ownT_off;
    launch_visco_Tpass(c->dim, all, k, v, c->stream);
    v.n = c->mixed_part ? c->nS : c->ownS_n;
    v.off_S = c->mixed_part ? 0 : c->ownS_off;
    v.map = c->map;
    launch_visco_Spass(c->dim, all, k, v, c->stream);
    if (copy_Tprev) copy(v.Tp, v.T, c->nT);
  }
  HIPC(hipGetLastError());
  return TV_OK;
}

}  // namespace tv

using namespace tv;

extern "C" {

int tv_residual(void* ctx, const double* T_dev, double* F_dev) {
  Ctx* c = static_cast<Ctx*>(ctx);
  if (!c || !T_dev || !F_dev) return TV_ERR_ARG;
  hipSetDevice(c->device);
  HIPC(hipDeviceSynchronize());  // inputs written on other streams (header)
  op_residual(c, T_dev, c->f[TV_F_T_PREV].ptr, F_dev);
  HIPC(hipGetLastError());
  HIPC(hipStreamSynchronize(c->stream));
  return TV_OK;
}


int tv_jacobian_apply(void* ctx, const double* x_dev, double* y_dev) {
  Ctx* c = static_cast<Ctx*>(ctx);
  if (!c || !x_dev || !y_dev) return TV_ERR_ARG;
  hipSetDevice(c->device);
  HIPC(hipDeviceSynchronize());  // inputs written on other streams (header)
  op_japply(c, c->f[TV_F_T].ptr, x_dev, y_dev, nullptr, nullptr);
  HIPC(hipGetLastError());
  HIPC(hipStreamSynchronize(c->stream));
  return TV_OK;
}


int tv_jacobian_diag(void* ctx, double* d_dev) {
  Ctx* c = static_cast<Ctx*>(ctx);
  if (!c || !d_dev) return TV_ERR_ARG;
  hipSetDevice(c->device);
  HIPC(hipDeviceSynchronize());  // inputs written on other streams (header)
  op_diag(c, c->f[TV_F_T].ptr, d_dev, 0);
  HIPC(hipGetLastError());
  HIPC(hipStreamSynchronize(c->stream));
  return TV_OK;
}


int tv_solve_T(void* ctx, int* newton_its, int* krylov_its, int* converged) {
  Ctx* c = static_cast<Ctx*>(ctx);
  if (!c) return TV_ERR_ARG;
  hipSetDevice(c->device);
  return newton(c, newton_its, krylov_its, converged);
}


int tv_visco_update(void* ctx) {
  Ctx* c = static_cast<Ctx*>(ctx);
  if (!c) return TV_ERR_ARG;
  hipSetDevice(c->device);
  if (int e = visco(c, false)) return e;
  HIPC(hipStreamSynchronize(c->stream));
  return TV_OK;
}


int tv_step(void* ctx, int thermal_only, int* newton_its, int* krylov_its) {
  Ctx* c = static_cast<Ctx*>(ctx);
  if (!c) return TV_ERR_ARG;
  hipSetDevice(c->device);
  int conv = 0;
  bool done = false;
  const int step_end = thermal_only ? 2 : 1;
  // the schedule's stage of this step, before its first evaluation: nothing of a
  // step is queued before the previous tv_step has returned (the Newton-ahead
  // queue and the speculative residual work inside newton(), within one step)
  if (int e = history_step_begin(c)) return e;
  if (int e = newton(c, newton_its, krylov_its, &conv, step_end, &done)) return e;
  // an unconverged solve (error_on_nonconvergence = False) stops here, as the
  // reference's _solve_T assert does (ThermoViscoProblem.py:390): T holds the
  // last Newton iterate, T_prev and the viscoelastic state keep the previous step.
  // Timing runs with fixed iteration counts (ksp_fixed_its > 0, bench.py --share:
  // Newton tolerances 0, so never "converged") end every step as a solve would.
  if (!done && (conv || c->O.ksp_fixed_its > 0)) {
    if (int e = queue_step_end(c, step_end, NewtonGate{})) return e;
    done = true;
  }
  // the step is counted; one that ended is recorded behind its end where a history is open
  // (an unconverged solve with error_on_nonconvergence = 0 took the step's number and wrote nothing)
  if (int e = history_step_end(c, done)) return e;
  HIPC(hipGetLastError());
  // no stream synchronisation: the visco update (and T_prev <- T) finishes
  // behind the host, which queues the next step's residual meanwhile (the
  // step boundary was a ~120 us idle gap).  Every host transfer and operator
  // call orders itself on the context's stream; tv_sync waits explicitly.
  return TV_OK;
}

}  // extern "C"

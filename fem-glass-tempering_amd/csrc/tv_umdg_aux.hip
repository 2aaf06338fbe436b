// Auxiliary-space multigrid for DG1 temperature on UNSTRUCTURED quadrilateral /
// hexahedral meshes (options.preconditioner = TV_PC_AUX), gfx950: the level-0
// kernels.  The reference preconditions its DG1 / CG1 pairing with PCGAMG
// (ThermoViscoProblem.py:343-346); here
//   level 0   the DG space, smoothed by cell-block Jacobi: B_e = the diagonal
//             block of J(T) of cell e (slot 0 of UmDgGrid::J + the Robin
//             Jacobian of its exterior facets), inverted once per cell and
//             stored as a packed symmetric inverse (NL (NL + 1) / 2 doubles per
//             cell, entry-major with stride ncs: a wave's loads are 512-byte
//             runs; the inverse, not the factor: no dependent triangular solves
//             in the apply);
//   level 1   the CG1 space of the same mesh (tv_amg.cpp aux_setup), reached by
//             index arithmetic: P copies a vertex value into each of its DG
//             copies, P^T sums the copies of a vertex through a padded
//             vertex -> dof incidence table (atomic-free, fixed order);
//   below     the aggregation hierarchy of tv_amg.cpp, unchanged.
// The cycle is additive at level 0, z = omega0 B^-1 r + P V_1(P^T r): no fine
// J x inside the preconditioner.  Every kernel is one lane per cell (or vertex),
// a wave a contiguous range of 64-cell groups, XCD-remapped blocks, as
// k_umdg_cells; every kernel of a solve exits at once when the solve is done.
#include <algorithm>

#include "tv_device.h"
#include "tv_um_elem.h"

namespace tv {
using namespace umk;
namespace {

constexpr int kAuxBlocksMax = 2048;  // grid cap (partial records of the prolongation)

// the contiguous range of 64-item groups of this wave (XCD-remapped blocks)
__device__ __forceinline__ void group_range(int64_t ngrp, int64_t& g0, int64_t& g1) {
  constexpr int WPB = kBlock / 64;
  const int wave = threadIdx.x >> 6;
  const int blk = xcd_remap(blockIdx.x, gridDim.x);
  const int64_t nw = (int64_t)gridDim.x * WPB;
  const int64_t gw = (int64_t)blk * WPB + wave;
  const int64_t chunk = (ngrp + nw - 1) / nw;
  g0 = gw * chunk;
  g1 = std::min<int64_t>(g0 + chunk, ngrp);
}

// packed lower triangle: entry (i, j), j <= i
__device__ __forceinline__ constexpr int pk(int i, int j) { return i >= j ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i; }

// ---- 1. block inverse ----------------------------------------------------------------
// One lane per cell: B_e gathered (lower triangle), the Robin Jacobian of the
// cell's exterior facets added (robin_row's quadrature: 3^(d-1) points, weights
// fw; the FULL facet block, not its diagonal), Cholesky in registers, L^-1, B^-1 = L^-T L^-1.
// all = 1: every cell (creation, T = 0), a non-positive pivot raises *flag;
// all = 0: the cells of the list bcell (exterior facets: per Newton iteration;
// the Robin part is positive semi-definite, so no check).
template <int D>
__global__ __launch_bounds__(kBlock) void k_umdg_binv(UmDgGrid g, UmDgAux a, const double* __restrict__ T, int all) {
  constexpr int NL = 1 << D, NQ = (D == 2) ? 3 : 9;
  const int64_t n = all ? g.nc : a.nbc;
  const int64_t t = blockIdx.x * (int64_t)kBlock + threadIdx.x;
  if (t >= n) return;
  const int64_t e = all ? t : (int64_t)a.bcell[t];
  const int64_t nc = g.nc, ncs = g.ncs;
  double B[NL][NL];
#pragma unroll
  for (int i = 0; i < NL; ++i)
#pragma unroll
    for (int j = 0; j <= i; ++j) B[i][j] = g.J[(int64_t)(i * NL + j) * ncs + e];
  double Tc[NL];
#pragma unroll
  for (int l = 0; l < NL; ++l) Tc[l] = T[(int64_t)l * nc + e];
#pragma unroll 1
  for (int lf = 0; lf < 2 * D; ++lf) {
    const int f = a.cfac[(int64_t)lf * ncs + e];
    if (f < 0) continue;
    const int ax = lf >> 1, side = lf & 1;
#pragma unroll 1
    for (int q = 0; q < NQ; ++q) {
      // the facet point (tangential axes increasing, q = i0 + 3 i1: fphi's order); the cell's Q1 basis
      // there is the facet-local basis on the facet's dofs and exactly 0 on the others
      double xi[D];
      int k = 0;
#pragma unroll
      for (int c = 0; c < D; ++c) {
        const bool nrm = c == ax;
        xi[c] = nrm ? (double)side : kUX[k == 0 ? q % 3 : q / 3];
        k += nrm ? 0 : 1;
      }
      double ph[NL], Tq = 0.0;
#pragma unroll
      for (int l = 0; l < NL; ++l) {
        double v = 1.0;
#pragma unroll
        for (int c = 0; c < D; ++c) v *= ((l >> c) & 1) ? xi[c] : 1.0 - xi[c];
        ph[l] = v;
        Tq += v * Tc[l];
      }
      const double cq = g.rb.dt * (g.rb.fw[(int64_t)q * g.rb.nf + f] * um_dg(g.rb, Tq));
#pragma unroll
      for (int i = 0; i < NL; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) B[i][j] += cq * (ph[i] * ph[j]);
    }
  }
  // Cholesky B = L L^T in place (the diagonal holds 1 / L_jj)
  bool bad = false;
#pragma unroll
  for (int j = 0; j < NL; ++j) {
    double d = B[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) d -= B[j][k] * B[j][k];
    if (!(d > 0.0)) bad = true;
    const double inv = 1.0 / sqrt(d);
    B[j][j] = inv;
#pragma unroll
    for (int i = j + 1; i < NL; ++i) {
      double s = B[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) s -= B[i][k] * B[j][k];
      B[i][j] = s * inv;
    }
  }
  if (all && bad) *a.flag = 1;
  // Li = L^-1 (lower)
  double Li[NL][NL];
#pragma unroll
  for (int j = 0; j < NL; ++j) {
    Li[j][j] = B[j][j];
#pragma unroll
    for (int i = j + 1; i < NL; ++i) {
      double s = 0.0;
#pragma unroll
      for (int k = j; k < i; ++k) s += B[i][k] * Li[k][j];
      Li[i][j] = -B[i][i] * s;
    }
  }
#pragma unroll
  for (int i = 0; i < NL; ++i)
#pragma unroll
    for (int j = 0; j <= i; ++j) {
      double s = 0.0;
#pragma unroll
      for (int k = i; k < NL; ++k) s += Li[k][i] * Li[k][j];
      a.binv[(int64_t)pk(i, j) * ncs + e] = s;
    }
}

// y = B_e^-1 v from the packed inverse, read once per iteration (non-temporal)
template <int NL>
__device__ __forceinline__ void binv_load(const double* __restrict__ binv, int64_t ncs, int64_t e,
                                          double (&b)[NL * (NL + 1) / 2]) {
#pragma unroll
  for (int k = 0; k < NL * (NL + 1) / 2; ++k) b[k] = __builtin_nontemporal_load(&binv[(int64_t)k * ncs + e]);
}
template <int NL>
__device__ __forceinline__ void binv_mul(const double (&b)[NL * (NL + 1) / 2], const double (&v)[NL],
                                         double (&y)[NL]) {
#pragma unroll
  for (int i = 0; i < NL; ++i) {
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < NL; ++j) s += b[pk(i, j)] * v[j];
    y[i] = s;
  }
}

// ---- 2. KSPCG update with the pre-smoothing ---------------------------------------------
// As k_mg_update / k_dg_bupdate: r <- r - a w, x0 <- omega B^-1 r, dx moved in
// pairs of iterations (DXU: dx <- (dx + a_prev p_prev) + a p on odd iterations,
// FIRST assigns it; launch_mg_dx_finish ends the solve).  INIT: x0 <- omega
// B^-1 r only (st may be null; x0 may be r itself: a lane reads its cell's
// values before it writes them).  Each lane holds its cell's NL values; every
// load of the cell is issued before the first store.
template <int D, bool INIT, bool DXU, bool FIRST>
__global__ __launch_bounds__(kBlock) void k_umdg_aux_update(int64_t nc, int64_t ncs, const double* __restrict__ binv,
                                                            const PcgState* __restrict__ st,
                                                            const double* __restrict__ pA,
                                                            const double* __restrict__ pB,
                                                            const double* __restrict__ w, double omega, double* r,
                                                            double* __restrict__ dx, double* x0, int it_host) {
  constexpr int NL = 1 << D;
  if (st != nullptr && st->done) return;
  const double a = INIT ? 0.0 : st->a;
  const double ap = DXU ? st->a_prev : 0.0;
  const double* __restrict__ p = (it_host & 1) ? pB : pA;
  const double* __restrict__ pp = (it_host & 1) ? pA : pB;
  const int lane = threadIdx.x & 63;
  int64_t g0, g1;
  group_range(ncs >> 6, g0, g1);
  for (int64_t grp = g0; grp < g1; ++grp) {
    const int64_t e = grp * 64 + lane;
    if (e >= nc) continue;  // padding lanes of the last group: nothing read, nothing written
    double b[NL * (NL + 1) / 2], v[NL], y[NL], wv[NL], dv[NL], ppv[NL], pv[NL];
    binv_load<NL>(binv, ncs, e, b);
#pragma unroll
    for (int l = 0; l < NL; ++l) {
      const int64_t o = (int64_t)l * nc + e;
      v[l] = r[o];
      if (!INIT) wv[l] = __builtin_nontemporal_load(&w[o]);
      if (DXU) {
        dv[l] = FIRST ? 0.0 : __builtin_nontemporal_load(&dx[o]);
        ppv[l] = __builtin_nontemporal_load(&pp[o]);
        pv[l] = __builtin_nontemporal_load(&p[o]);
      }
    }
    if (!INIT) {
#pragma unroll
      for (int l = 0; l < NL; ++l) {
        const int64_t o = (int64_t)l * nc + e;
        v[l] -= a * wv[l];
        r[o] = v[l];
        if (DXU) __builtin_nontemporal_store((dv[l] + ap * ppv[l]) + a * pv[l], &dx[o]);
      }
    }
    binv_mul<NL>(b, v, y);
#pragma unroll
    for (int l = 0; l < NL; ++l) x0[(int64_t)l * nc + e] = omega * y[l];
  }
}

// ---- 3. restriction DG -> CG -----------------------------------------------------------
// One lane per vertex: b_1 = the sum of r over the vertex's DG copies (table
// vinc[k vs + v], ascending dof, -1 padded), x_1 = omega_1 D_1^-1 b_1 (the CG
// level's pre-smoothing from 0, as launch_amg_restrict fuses it)
__global__ __launch_bounds__(kBlock) void k_umdg_aux_restrict(UmDgAux a, const PcgState* __restrict__ st,
                                                              const double* __restrict__ r,
                                                              const double* __restrict__ dinv1, double omega1,
                                                              double* __restrict__ b1, double* __restrict__ x1) {
  if (st != nullptr && st->done) return;
  const int lane = threadIdx.x & 63;
  int64_t g0, g1;
  group_range(a.vs >> 6, g0, g1);
  constexpr int U = 8;
  for (int64_t grp = g0; grp < g1; ++grp) {
    const int64_t v = grp * 64 + lane;
    if (v >= a.nv) continue;
    const double di = dinv1[v];
    double s = 0.0;
    for (int k0 = 0; k0 < a.nval; k0 += U) {
      int id[U];
      double rv[U];
#pragma unroll
      for (int j = 0; j < U; ++j)
        id[j] = (k0 + j < a.nval) ? __builtin_nontemporal_load(&a.vinc[(int64_t)(k0 + j) * a.vs + v]) : -1;
#pragma unroll
      for (int j = 0; j < U; ++j) rv[j] = id[j] >= 0 ? r[id[j]] : 0.0;
#pragma unroll
      for (int j = 0; j < U; ++j) s += rv[j];
    }
    b1[v] = s;
    x1[v] = omega1 * di * s;
  }
}

// ---- 4. prolongation with the KSPCG tail -----------------------------------------------
// z(e, l) = x0(e, l) + x_1[vertex(e, l)]; the (z.z, z.r) partial records and the
// reduction tail, as launch_amg_prolong0
template <int D>
__global__ __launch_bounds__(kBlock) void k_umdg_aux_prolong0(int64_t nc, int64_t ncs, const int* __restrict__ cellv,
                                                              const PcgState* __restrict__ st,
                                                              const double* __restrict__ x1,
                                                              const double* __restrict__ x0,
                                                              const double* __restrict__ r, double* __restrict__ z,
                                                              double* __restrict__ partials, RedTail rt) {
  constexpr int NL = 1 << D, WPB = kBlock / 64;
  if (st != nullptr && st->done) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int64_t g0, g1;
  group_range(ncs >> 6, g0, g1);
  double zz = 0.0, zb = 0.0;
  for (int64_t grp = g0; grp < g1; ++grp) {
    const int64_t e = grp * 64 + lane;
    if (e >= nc) continue;
    int vt[NL];
    double xv[NL], rv[NL], cv[NL];
#pragma unroll
    for (int l = 0; l < NL; ++l) vt[l] = __builtin_nontemporal_load(&cellv[(int64_t)l * ncs + e]);
#pragma unroll
    for (int l = 0; l < NL; ++l) {
      const int64_t o = (int64_t)l * nc + e;
      xv[l] = __builtin_nontemporal_load(&x0[o]);
      rv[l] = r[o];
      cv[l] = x1[vt[l]];
    }
#pragma unroll
    for (int l = 0; l < NL; ++l) {
      const double zv = xv[l] + cv[l];
      z[(int64_t)l * nc + e] = zv;
      zz += zv * zv;
      zb += zv * rv[l];
    }
  }
  __shared__ double red[2][WPB];
  const double s_zz = wave_sum64(zz), s_zb = wave_sum64(zb);
  if (lane == 0) {
    red[0][wave] = s_zz;
    red[1][wave] = s_zb;
  }
  __syncthreads();
  if (threadIdx.x < 2)
    store_partial(&partials[2 * (int64_t)blockIdx.x + threadIdx.x],
                  (red[threadIdx.x][0] + red[threadIdx.x][1]) + (red[threadIdx.x][2] + red[threadIdx.x][3]));
  fused_reduce_tail<2>(rt, gridDim.x);
}

// ---- setup: the CG1 cell operator of the mesh ------------------------------------------
// One thread per vertex: V = M + dt alpha K of the CG1 space, row r summed from
// the element rows (elem_row, the CG path's row assembly: k_um_assemble) of the
// cells around the vertex into the row's CSR entries (columns sorted; val
// zeroed before).  Only V: the level has no residual, no Robin terms.
template <int D>
__global__ __launch_bounds__(kBlock) void k_aux_assemble_v(UmDgAux a, int64_t nc, int64_t ncs,
                                                           const double* __restrict__ X0,
                                                           const double* __restrict__ X1,
                                                           const double* __restrict__ X2,
                                                           const int64_t* __restrict__ ptr,
                                                           const int* __restrict__ col, double dt_alpha,
                                                           double* __restrict__ val) {
  constexpr int NL = 1 << D;
  const int64_t r = blockIdx.x * (int64_t)kBlock + threadIdx.x;
  if (r >= a.nv) return;
  const double* const Xa[3] = {X0, X1, X2};
  const int64_t base = ptr[r];
  const int nz = (int)(ptr[r + 1] - base);
  for (int k = 0; k < a.nval; ++k) {
    const int id = a.vinc[(int64_t)k * a.vs + r];
    if (id < 0) break;
    const int l = (int)(id / nc);
    const int64_t e = id - (int64_t)l * nc;
    int nd[NL];
    double X[NL][D];
#pragma unroll
    for (int m = 0; m < NL; ++m) {
      nd[m] = a.cellv[(int64_t)m * ncs + e];
#pragma unroll
      for (int c = 0; c < D; ++c) X[m][c] = Xa[c][nd[m]];
    }
    double Ml[NL], Kl[NL];
    elem_row<D>(X, l, Ml, Kl);
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      int lo = 0, hi = nz;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (col[base + mid] < nd[j]) lo = mid + 1;
        else hi = mid;
      }
      val[base + lo] += Ml[j] + dt_alpha * Kl[j];
    }
  }
}

int group_blocks(int64_t n64) {  // n64: the item count rounded up to 64
  return (int)std::max<int64_t>(1, std::min<int64_t>(((n64 >> 6) + 3) / 4, kAuxBlocksMax));
}

}  // namespace

void launch_aux_assemble_v(int dim, const UmDgAux& a, int64_t nc, int64_t ncs, const double* X0, const double* X1,
                           const double* X2, const int64_t* ptr, const int* col, double dt_alpha, double* val,
                           hipStream_t s) {
  const dim3 grid((unsigned)((a.nv + kBlock - 1) / kBlock)), block(kBlock);
  if (dim == 2) hipLaunchKernelGGL(k_aux_assemble_v<2>, grid, block, 0, s, a, nc, ncs, X0, X1, X2, ptr, col, dt_alpha, val);
  else hipLaunchKernelGGL(k_aux_assemble_v<3>, grid, block, 0, s, a, nc, ncs, X0, X1, X2, ptr, col, dt_alpha, val);
}

void launch_umdg_binv(const UmDgGrid& g, const UmDgAux& a, const double* T, int all, hipStream_t s) {
  const int64_t n = all ? g.nc : a.nbc;
  if (n < 1) return;
  const dim3 grid((unsigned)((n + kBlock - 1) / kBlock)), block(kBlock);
  if (g.dim == 2) hipLaunchKernelGGL(k_umdg_binv<2>, grid, block, 0, s, g, a, T, all);
  else hipLaunchKernelGGL(k_umdg_binv<3>, grid, block, 0, s, g, a, T, all);
}

void launch_umdg_aux_update(const UmDgGrid& g, const UmDgAux& a, const PcgState* st, const double* pA,
                            const double* pB, const double* w, double omega, double* r, double* dx, double* x0,
                            int it_host, int init, hipStream_t s) {
  const dim3 grid(group_blocks(g.ncs)), block(kBlock);
  const bool odd = (it_host & 1) != 0, first = it_host == 1;
#define TV_AUXU(D, I, X, F)                                                                                       \
  hipLaunchKernelGGL((k_umdg_aux_update<D, I, X, F>), grid, block, 0, s, g.nc, g.ncs, a.binv, st, pA, pB, w, omega, \
                     r, dx, x0, it_host)
#define TV_AUXD(D)                                    \
  do {                                                \
    if (init) TV_AUXU(D, true, false, false);         \
    else if (first) TV_AUXU(D, false, true, true);    \
    else if (odd) TV_AUXU(D, false, true, false);     \
    else TV_AUXU(D, false, false, false);             \
  } while (0)
  if (g.dim == 2) TV_AUXD(2);
  else TV_AUXD(3);
#undef TV_AUXD
#undef TV_AUXU
}

void launch_umdg_aux_restrict(const UmDgAux& a, const PcgState* st, const double* r, const double* dinv1,
                              double omega1, double* b1, double* x1, hipStream_t s) {
  hipLaunchKernelGGL(k_umdg_aux_restrict, dim3(group_blocks(a.vs)), dim3(kBlock), 0, s, a, st, r, dinv1, omega1, b1,
                     x1);
}

int launch_umdg_aux_prolong0(const UmDgGrid& g, const UmDgAux& a, const PcgState* st, const double* x1,
                             const double* x0, const double* r, double* z, double* partials, const RedTail* tail,
                             hipStream_t s) {
  const int nb = group_blocks(g.ncs);
  const RedTail rt = tail ? *tail : RedTail{};
  if (g.dim == 2)
    hipLaunchKernelGGL(k_umdg_aux_prolong0<2>, dim3(nb), dim3(kBlock), 0, s, g.nc, g.ncs, a.cellv, st, x1, x0, r, z,
                       partials, rt);
  else
    hipLaunchKernelGGL(k_umdg_aux_prolong0<3>, dim3(nb), dim3(kBlock), 0, s, g.nc, g.ncs, a.cellv, st, x1, x0, r, z,
                       partials, rt);
  return nb;
}

}  // namespace tv

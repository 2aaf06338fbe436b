// DG1 temperature (SIPG) on UNSTRUCTURED quadrilateral / hexahedral meshes, gfx950:
// the reference's own discretisation (main.py: DG1 temperature, CG1 stress) on
// meshes that are not tensor-product grids.
//
// Replaces, for such meshes, the FFCx kernels of F dx, of the interior-facet
// terms dS (ThermoViscoProblem.py:313-325) and of the Robin terms ds (:302-304),
// their Jacobian, and the assembled PETSc matrix behind KSP (:331-343) [3P].
//
// The T-independent operator V = M + dt alpha (K + SIPG) couples a cell's 2^d
// dofs to its own and to those of its <= 2 d facet neighbours, so it is stored
// as 1 + 2 d dense blocks per cell (UmDgGrid, tv_internal.h): 8 B per entry and
// one int32 per neighbour, no column indices.  It is assembled once, at context
// creation; J x runs one lane per cell (k_umdg_cells), the residual and the
// diagonal one lane per row (k_umdg_rows); either way a wave covers 64 cells, so
// every matrix load of a wave is a 512-byte run.  Every row is owned by one
// lane: no atomics, a fixed summation order (bitwise reproducible).
//  * J x  (japply / the fused PCG matvec): blocks of V, + Robin'(T) on the fly;
//  * F(T) (residual): M (T - T_prev) + S T - dt f int phi + Robin(T), with M and
//    S = dt alpha (K + SIPG) apart so T - T_prev is formed before the product;
//  * diag J: the diagonal of slot 0 + the Robin diagonal.
// Interior facets (oracle/tv_oracle.py HeatForm._prep_interior, _sipg_matrix):
// 3^(d-1) Gauss points on the '+' facet ('+' = the lower cell index), weight
// w_q |det J+| |J+^-T e_axis|, normal n+, h = the largest vertex distance of the
// '+' cell, penalty 5.  The '-' reference point of a '+' Gauss point follows
// from the vertex correspondence of the two facets (um_facets' orient): the
// trace of a Q1 map on a facet is the bilinear map of the facet's own vertices.
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "tv_device.h"
#include "tv_um_elem.h"

namespace tv {
using namespace umk;

struct UmDgDevice {
  std::vector<void*> bufs;  // freed by umdg_free
};

// ---- host: facet analysis -----------------------------------------------------------
int um_facets(int dim, int64_t nv, int64_t nc, const int64_t* cells, std::vector<int64_t>& exterior2,
              std::vector<int64_t>& interior5, std::string& err) {
  if ((dim != 2 && dim != 3) || nc < 1 || !cells) {
    err = "facets: a quadrilateral (dim 2) or hexahedral (dim 3) mesh with at least one cell";
    return 1;
  }
  const int nl = 1 << dim, nfv = nl / 2;
  for (int64_t k = 0; k < nc * nl; ++k)
    if (cells[k] < 0 || cells[k] >= nv) {
      err = "cell vertex index out of range";
      return 1;
    }
  struct F {
    int64_t v[4];
    int64_t cell;
    int lf;
  };
  std::vector<F> fs;
  fs.reserve((size_t)nc * 2 * dim);
  for (int64_t e = 0; e < nc; ++e)
    for (int lf = 0; lf < 2 * dim; ++lf) {
      F f{{-1, -1, -1, -1}, e, lf};
      int k = 0;
      for (int l = 0; l < nl; ++l)
        if (((l >> (lf >> 1)) & 1) == (lf & 1)) f.v[k++] = cells[e * nl + l];
      std::sort(f.v, f.v + nfv);
      fs.push_back(f);
    }
  auto cmp = [&](const F& a, const F& b) {  // -1, 0, 1 on the vertex sets
    for (int k = 0; k < nfv; ++k)
      if (a.v[k] != b.v[k]) return a.v[k] < b.v[k] ? -1 : 1;
    return 0;
  };
  std::sort(fs.begin(), fs.end(), [&](const F& a, const F& b) {
    const int c = cmp(a, b);
    if (c != 0) return c < 0;
    return a.cell != b.cell ? a.cell < b.cell : a.lf < b.lf;
  });
  struct I {
    int64_t cp, cm;
    int lfp, lfm, orient;
  };
  std::vector<std::pair<int64_t, int>> ext;
  std::vector<I> in;
  for (size_t i = 0; i < fs.size();) {
    size_t j = i + 1;
    while (j < fs.size() && cmp(fs[i], fs[j]) == 0) ++j;
    if (j - i > 2) {
      err = "non-manifold mesh: a facet shared by more than two cells";
      return 1;
    }
    if (j - i == 1) {
      ext.emplace_back(fs[i].cell, fs[i].lf);
    } else {
      const F &p = fs[i], &m = fs[i + 1];  // '+' = the lower cell index
      if (p.cell == m.cell) {
        err = "degenerate cell: two of its facets have the same vertices";
        return 1;
      }
      // facet-local tensor order of both sides (tangential axes increasing)
      int64_t vp[4], vm[4];
      int kp = 0, km = 0;
      for (int l = 0; l < nl; ++l) {
        if (((l >> (p.lf >> 1)) & 1) == (p.lf & 1)) vp[kp++] = cells[p.cell * nl + l];
        if (((l >> (m.lf >> 1)) & 1) == (m.lf & 1)) vm[km++] = cells[m.cell * nl + l];
      }
      auto pos = [&](int64_t v) {
        for (int q = 0; q < nfv; ++q)
          if (vm[q] == v) return q;
        return -1;
      };
      const int p0 = pos(vp[0]);
      int orient = 0, axm[2] = {0, 0};
      bool ok = p0 >= 0;
      for (int k = 0; k < dim - 1 && ok; ++k) {
        const int pk = pos(vp[1 << k]);
        const int d = pk ^ p0;
        if (pk < 0 || (d != 1 && d != 2) || d >= nfv) {
          ok = false;
          break;
        }
        axm[k] = d >> 1;  // d = 1 << axis
        orient |= (axm[k] | (((p0 >> axm[k]) & 1) << 1)) << (2 * k);
      }
      if (ok && dim == 3 && axm[0] == axm[1]) ok = false;
      for (int q = 0; q < nfv && ok; ++q) {
        int want = p0;
        for (int k = 0; k < dim - 1; ++k)
          if ((q >> k) & 1) want ^= 1 << axm[k];
        if (pos(vp[q]) != want) ok = false;
      }
      if (!ok) {
        err = "non-conforming mesh: a shared vertex set that is not a facet of both cells";
        return 1;
      }
      in.push_back(I{p.cell, m.cell, p.lf, m.lf, orient});
    }
    i = j;
  }
  std::sort(ext.begin(), ext.end());
  std::sort(in.begin(), in.end(), [](const I& a, const I& b) { return a.cp != b.cp ? a.cp < b.cp : a.lfp < b.lfp; });
  exterior2.clear();
  interior5.clear();
  for (const auto& e : ext) {
    exterior2.push_back(e.first);
    exterior2.push_back(e.second);
  }
  for (const I& f : in)
    for (int64_t v : {f.cp, (int64_t)f.lfp, f.cm, (int64_t)f.lfm, (int64_t)f.orient}) interior5.push_back(v);
  return 0;
}

namespace {

constexpr int kUmDgBlocksMax = 2048;  // grid cap of the row and cell kernels (partial records of the fused launch)
constexpr double kPenalty = 5.0;      // ThermoViscoProblem.py:313

// ---- setup kernels -------------------------------------------------------------------
template <int D>
__device__ __forceinline__ void load_cell(const int* __restrict__ cell, int64_t nc, int64_t e,
                                          const double* const (&Xa)[3], double (&X)[1 << D][D]) {
#pragma unroll
  for (int l = 0; l < (1 << D); ++l) {
    const int v = cell[(int64_t)l * nc + e];
#pragma unroll
    for (int a = 0; a < D; ++a) X[l][a] = Xa[a][v];
  }
}

// xi[idx] = val without dynamic indexing of a private array
__device__ __forceinline__ void set3(double (&xi)[3], int idx, double val) {
#pragma unroll
  for (int a = 0; a < 3; ++a)
    if (a == idx) xi[a] = val;
}
// k-th tangential axis (increasing) of a facet with normal axis ax
template <int D>
__device__ __forceinline__ int tang_axis(int ax, int k) {
  if (D == 2) return 1 - ax;
  return k == 0 ? (ax == 0 ? 1 : 0) : (ax == 2 ? 1 : 2);
}

// the traces at reference point xi of a cell with vertices X: phi, the physical
// gradients' normal components dn[j] = grad phi_j . n.  own = true: xi lies on
// the facet xi_ax = side of THIS cell, n is computed here (outward unit normal)
// and *meas = |det J| |J^-T e_ax|; else n is given.
template <int D>
__device__ __forceinline__ void facet_trace(const double (&X)[1 << D][D], const double (&xi)[3], bool own, int ax,
                                            int side, double (&n)[D], double* meas, double (&phi)[1 << D],
                                            double (&dn)[1 << D]) {
  constexpr int NL = 1 << D;
  double dphi[NL][D];
  q1<D>(xi, phi, dphi);
  double J[D][D];
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = 0; b < D; ++b) {
      double s = 0.0;
#pragma unroll
      for (int l = 0; l < NL; ++l) s += X[l][a] * dphi[l][b];
      J[a][b] = s;
    }
  double Ji[D][D];
  const double det = fabs(inv_det<D>(J, Ji));
  if (own) {
    double gr[D], gn = 0.0;  // row ax of J^-1 = grad xi_ax
#pragma unroll
    for (int b = 0; b < D; ++b) {
      double v = 0.0;
#pragma unroll
      for (int a = 0; a < D; ++a)
        if (a == ax) v = Ji[a][b];
      gr[b] = v;
      gn += v * v;
    }
    gn = sqrt(gn);
    const double sg = side ? 1.0 : -1.0;
#pragma unroll
    for (int b = 0; b < D; ++b) n[b] = sg * (gr[b] / gn);
    *meas = det * gn;
  }
#pragma unroll
  for (int l = 0; l < NL; ++l) {
    double s = 0.0;
#pragma unroll
    for (int a = 0; a < D; ++a) {
      double ga = 0.0;  // (J^-T dphi_l)_a
#pragma unroll
      for (int b = 0; b < D; ++b) ga += Ji[b][a] * dphi[l][b];
      s += ga * n[a];
    }
    dn[l] = s;
  }
}

// One thread per DG row r = i nc + e: row i of the cell blocks of cell e (mass,
// dt alpha K) and, facet by facet in the order lf = 0 .. 2 d - 1, row i of the
// SIPG blocks (e, e) and (e, neighbour).  Both cells of a facet recompute the
// facet's quadrature data; the '+' cell's geometry rules on both sides.
//   finfo[lf ncs + e] = (the neighbour's local facet) | orient << 3, orient as
//   in um_facets (how the '-' tangential coordinates follow the '+' ones)
template <int D>
__global__ __launch_bounds__(kBlock) void k_umdg_assemble(int64_t nc, int64_t ncs, const int* __restrict__ cell,
                                                          const double* __restrict__ X0, const double* __restrict__ X1,
                                                          const double* __restrict__ X2, const int* __restrict__ nbr,
                                                          const unsigned char* __restrict__ finfo, double dt_alpha,
                                                          double* __restrict__ Jb, double* __restrict__ S0,
                                                          double* __restrict__ M0, double* __restrict__ bvec) {
  constexpr int NL = 1 << D;
  constexpr int NQ = (D == 2) ? 3 : 9;
  const int64_t r = blockIdx.x * (int64_t)kBlock + threadIdx.x;
  if (r >= nc * NL) return;
  const int i = (int)(r / nc);
  const int64_t e = r - (int64_t)i * nc;
  const double* const Xa[3] = {X0, X1, X2};
  double s0[NL], Ml[NL];
  {
    double X[NL][D], Kl[NL];
    load_cell<D>(cell, nc, e, Xa, X);
    elem_row<D>(X, i, Ml, Kl);
    double b = 0.0;
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      s0[j] = dt_alpha * Kl[j];
      b += Ml[j];
    }
    bvec[r] = b;
  }
#pragma unroll 1
  for (int lf = 0; lf < 2 * D; ++lf) {
    const int64_t nb = nbr[(int64_t)lf * ncs + e];
    if (nb == e) continue;  // exterior facet: its block stays 0
    const int info = finfo[(int64_t)lf * ncs + e];
    const int nlf = info & 7, orient = info >> 3;
    const bool plus = e < nb;
    const int lfp = plus ? lf : nlf, lfm = plus ? nlf : lf;
    const int axp = lfp >> 1, sdp = lfp & 1, axm = lfm >> 1, sdm = lfm & 1;
    double Xp[NL][D], Xm[NL][D];
    load_cell<D>(cell, nc, plus ? e : nb, Xa, Xp);
    load_cell<D>(cell, nc, plus ? nb : e, Xa, Xm);
    double h2 = 0.0;  // ufl.CellDiameter('+')^2: the largest vertex distance
#pragma unroll
    for (int a = 0; a < NL; ++a)
#pragma unroll
      for (int b = a + 1; b < NL; ++b) {
        double d2 = 0.0;
#pragma unroll
        for (int c = 0; c < D; ++c) d2 += (Xp[a][c] - Xp[b][c]) * (Xp[a][c] - Xp[b][c]);
        h2 = fmax(h2, d2);
      }
    const double pen = kPenalty / sqrt(h2);
    double cc[NL], cn[NL];
#pragma unroll
    for (int j = 0; j < NL; ++j) cc[j] = cn[j] = 0.0;
#pragma unroll 1
    for (int q = 0; q < NQ; ++q) {
      double xp[3] = {0.0, 0.0, 0.0}, xm[3] = {0.0, 0.0, 0.0}, w = 1.0;
      set3(xp, axp, (double)sdp);
      set3(xm, axm, (double)sdm);
#pragma unroll
      for (int k = 0; k < D - 1; ++k) {
        const int qk = (k == 0) ? q % 3 : q / 3;
        const double t = kUX[qk];
        w *= kUW[qk];
        set3(xp, tang_axis<D>(axp, k), t);
        const int o = (orient >> (2 * k)) & 3;
        set3(xm, tang_axis<D>(axm, o & 1), (o & 2) ? 1.0 - t : t);
      }
      double n[D], meas = 0.0, php[NL], dnp[NL], phm[NL], dnm[NL];
      facet_trace<D>(Xp, xp, true, axp, sdp, n, &meas, php, dnp);
      facet_trace<D>(Xm, xm, false, axm, sdm, n, nullptr, phm, dnm);
      const double wq = w * meas;
      // jump(phi_j, n) = a_j n, avg(grad phi_j) . n = b_j:  '+' a = phi, '-' a = -phi; b = grad phi . n / 2
      double ai = 0.0, bi = 0.0;
#pragma unroll
      for (int j = 0; j < NL; ++j)
        if (j == i) {
          ai = plus ? php[j] : -phm[j];
          bi = 0.5 * (plus ? dnp[j] : dnm[j]);
        }
#pragma unroll
      for (int j = 0; j < NL; ++j) {
        const double ap = php[j], bp = 0.5 * dnp[j], am = -phm[j], bm = 0.5 * dnm[j];
        const double ao = plus ? ap : am, bo = plus ? bp : bm;  // own cell's dof j
        const double an = plus ? am : ap, bn = plus ? bm : bp;  // the neighbour's dof j
        cc[j] += wq * (pen * (ai * ao) - bi * ao - ai * bo);
        cn[j] += wq * (pen * (ai * an) - bi * an - ai * bn);
      }
    }
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      s0[j] += dt_alpha * cc[j];
      Jb[(((int64_t)(1 + lf) * NL + i) * NL + j) * ncs + e] = dt_alpha * cn[j];
    }
  }
#pragma unroll
  for (int j = 0; j < NL; ++j) {
    const int64_t o = ((int64_t)i * NL + j) * ncs + e;
    M0[o] = Ml[j];
    S0[o] = s0[j];
    Jb[o] = Ml[j] + s0[j];
  }
}

// one thread per exterior facet: w_q |J_s|(q) at its 3^(d-1) points, point
// index q = i0 + 3 i1 over the tangential axes in increasing order (fphi)
template <int D>
__global__ __launch_bounds__(kBlock) void k_umdg_facet_w(int64_t nf, int64_t nc, const int* __restrict__ fcell,
                                                         const signed char* __restrict__ flf,
                                                         const int* __restrict__ cell, const double* __restrict__ X0,
                                                         const double* __restrict__ X1, const double* __restrict__ X2,
                                                         double* __restrict__ fw) {
  constexpr int NL = 1 << D;
  constexpr int NQ = (D == 2) ? 3 : 9;
  const int64_t f = blockIdx.x * (int64_t)kBlock + threadIdx.x;
  if (f >= nf) return;
  const int lf = flf[f], ax = lf >> 1, side = lf & 1;
  const double* const Xa[3] = {X0, X1, X2};
  double X[NL][D];
  load_cell<D>(cell, nc, fcell[f], Xa, X);
#pragma unroll 1
  for (int q = 0; q < NQ; ++q) {
    double xi[3] = {0.0, 0.0, 0.0}, w = 1.0;
    set3(xi, ax, (double)side);
#pragma unroll
    for (int k = 0; k < D - 1; ++k) {
      const int qk = (k == 0) ? q % 3 : q / 3;
      set3(xi, tang_axis<D>(ax, k), kUX[qk]);
      w *= kUW[qk];
    }
    double n[D], meas = 0.0, phi[NL], dn[NL];
    facet_trace<D>(X, xi, true, ax, side, n, &meas, phi, dn);
    fw[(int64_t)q * nf + f] = w * meas;
  }
}

// ---- the row kernels -----------------------------------------------------------------
// The residual and the diagonal, once per Newton iteration: one lane per row; a
// wave's work item is (cell group of 64, local row i), the 2^d items of a group
// consecutive, each wave a contiguous range of items (XCD-remapped blocks: a
// contiguous cell range per XCD, so the 2^d waves of a group and the
// neighbouring groups gather from one L2).
//   UM_RES:   out = M (u - up) + S u - dt f b            (u = T, up = T_prev; the
//             Robin terms follow in k_umdg_robin_res)
//   UM_DIAG:  out = diag V + Robin diagonal (inverted if `invert`)
template <int D, int MODE>
__global__ __launch_bounds__(kBlock) void k_umdg_rows(UmDgGrid g, const double* __restrict__ u,
                                                      const double* __restrict__ up, double* __restrict__ out,
                                                      int invert) {
  static_assert(MODE == UM_RES || MODE == UM_DIAG, "J x runs k_umdg_cells");
  constexpr int NL = 1 << D, NS = 1 + 2 * D;
  auto xget = [&](int64_t c) -> double { return u[c]; };
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  constexpr int WPB = kBlock / 64;
  const int blk = xcd_remap(blockIdx.x, gridDim.x);
  const int64_t nw = (int64_t)gridDim.x * WPB;
  const int64_t gw = (int64_t)blk * WPB + wave;
  const int64_t nitem = (g.ncs >> 6) * NL;
  const int64_t chunk = (nitem + nw - 1) / nw;
  const int64_t w0 = gw * chunk, w1 = std::min<int64_t>(w0 + chunk, nitem);
  const int64_t nc = g.nc, ncs = g.ncs;
  for (int64_t it = w0; it < w1; ++it) {
    const int i = (int)(it % NL);
    const int64_t e = (it / NL) * 64 + lane;
    const bool ok = e < nc;
    const int64_t ec = ok ? e : nc - 1;  // padding lanes of the last group: in-range gathers, zero blocks
    const int64_t r = (int64_t)i * nc + ec;
    double val = 0.0;
    if (MODE == UM_DIAG) {
      val = g.J[((int64_t)i * NL + i) * ncs + e];
    } else {
      // the matrix is read once per product: non-temporal, so the stream does
      // not evict the gathered vector from L2 (as k_um_rows)
      double acc = 0.0, acc2 = 0.0;
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const int64_t cb = (s == 0) ? ec : (int64_t)__builtin_nontemporal_load(&g.nbr[(int64_t)(s - 1) * ncs + e]);
        if (s == 0) {
          const double* __restrict__ am = g.M0 + (int64_t)i * NL * ncs + e;
          const double* __restrict__ as = g.S0 + (int64_t)i * NL * ncs + e;
#pragma unroll
          for (int j = 0; j < NL; ++j) {
            const double xc = u[(int64_t)j * nc + cb];
            acc += __builtin_nontemporal_load(&am[(int64_t)j * ncs]) * (xc - up[(int64_t)j * nc + cb]);
            acc2 += __builtin_nontemporal_load(&as[(int64_t)j * ncs]) * xc;
          }
        } else {
          const double* __restrict__ a = g.J + ((int64_t)s * NL + i) * NL * ncs + e;
          double m[NL], x[NL];
#pragma unroll
          for (int j = 0; j < NL; ++j) {
            m[j] = __builtin_nontemporal_load(&a[(int64_t)j * ncs]);
            x[j] = u[(int64_t)j * nc + cb];
          }
#pragma unroll
          for (int j = 0; j < NL; ++j) acc2 += m[j] * x[j];
        }
      }
      val = (acc + acc2) - g.rb.dt_f * g.bvec[r];
    }
    if (ok) {
      if (MODE == UM_DIAG) {
        val += robin_row<D, UM_DIAG>(g.rb, r, u, xget);  // u = T
        if (invert) val = 1.0 / val;
      }
      out[r] = val;
    }
  }
}

// J x as the solves run it (UM_JAC and UM_FUSED): one lane per CELL with 2^d
// accumulators.  Every matrix entry is still loaded once, in the same 512-byte
// runs, but the x values of a neighbour are gathered once per cell instead of
// once per row.  Measured on a distorted plate of 221K hexahedra against one
// lane per row, k_umdg_rows' shape: 187 against 315 us
// per J x; the lane-per-row J x was taken out after that measurement.
template <int D, int MODE>
__global__ __launch_bounds__(kBlock) void k_umdg_cells(UmDgGrid g, const double* __restrict__ T,
                                                       const double* __restrict__ u, double* __restrict__ out,
                                                       const PcgState* __restrict__ st,
                                                       double* __restrict__ partials, RedTail rt) {
  constexpr int NL = 1 << D, NS = 1 + 2 * D;
  if (MODE == UM_FUSED && st->done) return;
  auto xget = [&](int64_t c) -> double { return u[c]; };
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  constexpr int WPB = kBlock / 64;
  const int blk = xcd_remap(blockIdx.x, gridDim.x);
  const int64_t nw = (int64_t)gridDim.x * WPB;
  const int64_t gw = (int64_t)blk * WPB + wave;
  const int64_t ngrp = g.ncs >> 6;
  const int64_t chunk = (ngrp + nw - 1) / nw;
  const int64_t w0 = gw * chunk, w1 = std::min<int64_t>(w0 + chunk, ngrp);
  const int64_t nc = g.nc, ncs = g.ncs;
  double pw = 0.0;
  for (int64_t grp = w0; grp < w1; ++grp) {
    const int64_t e = grp * 64 + lane;
    const bool ok = e < nc;
    const int64_t ec = ok ? e : nc - 1;
    double acc[NL];
#pragma unroll
    for (int i = 0; i < NL; ++i) acc[i] = 0.0;
#pragma unroll 1
    for (int s = 0; s < NS; ++s) {
      const int64_t cb = (s == 0) ? ec : (int64_t)g.nbr[(int64_t)(s - 1) * ncs + e];
      const double* __restrict__ a = g.J + (int64_t)s * NL * NL * ncs + e;
      double x[NL];
#pragma unroll
      for (int j = 0; j < NL; ++j) x[j] = u[(int64_t)j * nc + cb];
#pragma unroll
      for (int i = 0; i < NL; ++i)
#pragma unroll
        for (int j = 0; j < NL; ++j) acc[i] += __builtin_nontemporal_load(&a[(int64_t)(i * NL + j) * ncs]) * x[j];
    }
    if (ok) {
#pragma unroll
      for (int i = 0; i < NL; ++i) {
        const int64_t r = (int64_t)i * nc + e;
        const double val = acc[i] + robin_row<D, MODE>(g.rb, r, T, xget);
        if (MODE == UM_FUSED) pw += u[r] * val;
        out[r] = val;
      }
    }
  }
  if (MODE == UM_FUSED) {
    __shared__ double red[WPB];
    const double sw = wave_sum64(pw);
    if (lane == 0) red[wave] = sw;
    __syncthreads();
    if (threadIdx.x == 0) store_partial(&partials[blockIdx.x], (red[0] + red[1]) + (red[2] + red[3]));
    fused_reduce_tail<1>(rt, gridDim.x);
  }
}

// the residual's Robin terms on the rows of the boundary cells' facet dofs,
// added to the cell and SIPG part k_umdg_rows<UM_RES> wrote
template <int D>
__global__ __launch_bounds__(kBlock) void k_umdg_robin_res(UmGrid g, const double* __restrict__ u,
                                                           double* __restrict__ F) {
  auto xget = [&](int64_t c) -> double { return u[c]; };
  for (int64_t b = blockIdx.x * (int64_t)kBlock + threadIdx.x; b < g.nbr; b += (int64_t)gridDim.x * kBlock) {
    const int64_t r = g.brow[b];
    F[r] += robin_row<D, UM_RES>(g, r, u, xget);
  }
}

int row_blocks(const UmDgGrid& g) {
  const int64_t nitem = (g.ncs >> 6) << g.dim;
  return (int)std::max<int64_t>(1, std::min<int64_t>((nitem + 3) / 4, kUmDgBlocksMax));
}

int cell_blocks(const UmDgGrid& g) {
  return (int)std::max<int64_t>(1, std::min<int64_t>(((g.ncs >> 6) + 3) / 4, kUmDgBlocksMax));
}
// returns the number of workgroups (= partial records of UM_FUSED)
template <int MODE>
int launch_cells(const UmDgGrid& g, const double* T, const double* u, double* out, const PcgState* st,
                 double* partials, const RedTail& rt, hipStream_t s) {
  const dim3 grid(cell_blocks(g)), block(kBlock);
  if (g.dim == 2) hipLaunchKernelGGL((k_umdg_cells<2, MODE>), grid, block, 0, s, g, T, u, out, st, partials, rt);
  else hipLaunchKernelGGL((k_umdg_cells<3, MODE>), grid, block, 0, s, g, T, u, out, st, partials, rt);
  return (int)grid.x;
}

template <int MODE>
void launch_rows(const UmDgGrid& g, const double* u, const double* up, double* out, int invert, hipStream_t s) {
  const dim3 grid(row_blocks(g)), block(kBlock);
  if (g.dim == 2) hipLaunchKernelGGL((k_umdg_rows<2, MODE>), grid, block, 0, s, g, u, up, out, invert);
  else hipLaunchKernelGGL((k_umdg_rows<3, MODE>), grid, block, 0, s, g, u, up, out, invert);
}

}  // namespace

int umdg_num_blocks(const UmDgGrid& g) { return cell_blocks(g); }

double umdg_matvec_bytes(const UmDgGrid& g) {
  const double nl = (double)(1 << g.dim), ns = 1.0 + 2.0 * g.dim;
  return (8.0 * ns * nl * nl + 4.0 * (ns - 1.0)) * (double)g.nc;  // the blocks and the neighbour table, once per cell
}

void launch_umdg_residual(const UmDgGrid& g, const double* T, const double* Tp, double* F, hipStream_t s) {
  launch_rows<UM_RES>(g, T, Tp, F, 0, s);
  if (g.rb.nbr == 0) return;
  const dim3 gr((unsigned)std::max<int64_t>(1, std::min<int64_t>((g.rb.nbr + kBlock - 1) / kBlock, 4096)));
  if (g.dim == 2) hipLaunchKernelGGL(k_umdg_robin_res<2>, gr, dim3(kBlock), 0, s, g.rb, T, F);
  else hipLaunchKernelGGL(k_umdg_robin_res<3>, gr, dim3(kBlock), 0, s, g.rb, T, F);
}

void launch_umdg_japply(const UmDgGrid& g, const double* T, const double* x, double* y, hipStream_t s) {
  launch_cells<UM_JAC>(g, T, x, y, nullptr, nullptr, RedTail{}, s);
}

void launch_umdg_diag(const UmDgGrid& g, const double* T, double* d, int invert, hipStream_t s) {
  launch_rows<UM_DIAG>(g, T, nullptr, d, invert, s);
}

int launch_umdg_japply_fused(const UmDgGrid& g, const double* T, const double* z, double* pA, double* pB, double* w,
                             const PcgState* st, double* partials, int it_host, const RedTail* tail, hipStream_t s) {
  const RedTail rt = tail ? *tail : RedTail{};
  launch_um_pvec(g.nc << g.dim, st, z, pA, pB, it_host, rt, s);
  const double* p = (it_host & 1) ? pB : pA;
  return launch_cells<UM_FUSED>(g, T, p, w, st, partials, rt, s);
}

// ---- host: device setup ----------------------------------------------------------------
#define UMC(x)                                                              \
  do {                                                                      \
    if ((x) != hipSuccess) {                                                \
      err = std::string("HIP error in unstructured DG setup: ") + #x;       \
      return 1;                                                             \
    }                                                                       \
  } while (0)

template <class T>
static int dg_upload(UmDgDevice* d, const std::vector<T>& h, T** out, std::string& err) {
  void* p = nullptr;
  UMC(tv_dev_alloc(&p, sizeof(T) * std::max<size_t>(1, h.size()), mem_kind<T>()));
  d->bufs.push_back(p);
  if (!h.empty()) UMC(hipMemcpy(p, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice));
  *out = static_cast<T*>(p);
  return 0;
}

// zero-filled: the padding lanes of the last cell group read zero blocks
static int dg_zeros(UmDgDevice* d, size_t n, double** out, hipStream_t s, std::string& err) {
  void* p = nullptr;
  const size_t bytes = sizeof(double) * std::max<size_t>(1, n);
  UMC(tv_dev_alloc(&p, bytes, kMemDoubles));
  d->bufs.push_back(p);
  UMC(hipMemsetAsync(p, 0, bytes, s));
  *out = static_cast<double*>(p);
  return 0;
}

static void dg_release(UmDgDevice* d, void* p) {
  auto it = std::find(d->bufs.begin(), d->bufs.end(), p);
  if (it != d->bufs.end()) {
    tv_dev_free(p);
    d->bufs.erase(it);
  }
}

void umdg_free(UmDgDevice* d) {
  if (!d) return;
  for (void* p : d->bufs) tv_dev_free(p);
  delete d;
}

int umdg_setup(int dim, int64_t nv, const double* xyz, int64_t nc, const int64_t* cells, UmDgGrid& g,
               UmDgDevice*& dev, hipStream_t s, std::string& err) {
  const int nl = 1 << dim, nfv = nl / 2, nlf = 2 * dim;
  const int64_t nT = nc * nl;
  if (nT >= (int64_t)INT32_MAX / 4) {  // int32 dof ids (fv, the interpolation map) and 4 f + m incidence codes
    err = "unstructured DG: < 2^29 temperature dofs";
    return 1;
  }
  std::vector<int64_t> ext, in;
  if (um_facets(dim, nv, nc, cells, ext, in, err)) return 1;
  dev = new UmDgDevice();
  UmDgDevice* d = dev;
  const int64_t ncs = (nc + 63) / 64 * 64;
  const int64_t nf = (int64_t)ext.size() / 2, ni = (int64_t)in.size() / 5;
  // -- neighbour table (an exterior facet: the cell itself; padding lanes: cell 0) and the facet codes
  std::vector<int> nbr((size_t)nlf * ncs, 0);
  std::vector<unsigned char> finfo((size_t)nlf * ncs, 0);
  for (int lf = 0; lf < nlf; ++lf)
    for (int64_t e = 0; e < nc; ++e) nbr[(size_t)(lf * ncs + e)] = (int)e;
  for (int64_t k = 0; k < ni; ++k) {
    const int64_t cp = in[5 * k], lfp = in[5 * k + 1], cm = in[5 * k + 2], lfm = in[5 * k + 3], o = in[5 * k + 4];
    nbr[(size_t)(lfp * ncs + cp)] = (int)cm;
    nbr[(size_t)(lfm * ncs + cm)] = (int)cp;
    finfo[(size_t)(lfp * ncs + cp)] = (unsigned char)(lfm | (o << 3));
    finfo[(size_t)(lfm * ncs + cm)] = (unsigned char)(lfp | (o << 3));
  }
  // -- exterior facets: the facet's dofs in facet-local tensor order and the
  // incidences of the DG rows (robin_row's tables over DG dofs)
  std::vector<int> fcell((size_t)nf), fv((size_t)nfv * nf), boff((size_t)nT + 1, 0);
  std::vector<signed char> flf((size_t)nf);
  for (int64_t f = 0; f < nf; ++f) {
    const int64_t e = ext[2 * f];
    const int lf = (int)ext[2 * f + 1];
    fcell[(size_t)f] = (int)e;
    flf[(size_t)f] = (signed char)lf;
    int m = 0;
    for (int l = 0; l < nl; ++l)
      if (((l >> (lf >> 1)) & 1) == (lf & 1)) {
        const int64_t r = (int64_t)l * nc + e;
        fv[(size_t)((int64_t)(m++) * nf + f)] = (int)r;
        boff[(size_t)r + 1]++;
      }
  }
  for (int64_t r = 0; r < nT; ++r) boff[(size_t)r + 1] += boff[(size_t)r];
  std::vector<int> binc((size_t)boff[(size_t)nT]);
  std::vector<int64_t> brow;
  {
    std::vector<int> fill(boff.begin(), boff.end() - 1);
    for (int64_t f = 0; f < nf; ++f)
      for (int m = 0; m < nfv; ++m) binc[(size_t)fill[(size_t)fv[(size_t)((int64_t)m * nf + f)]]++] = (int)(4 * f + m);
    for (int64_t r = 0; r < nT; ++r)
      if (boff[(size_t)r + 1] > boff[(size_t)r]) brow.push_back(r);
  }
  // -- uploads
  std::vector<double> Xh((size_t)nv);
  double* Xd[3];
  for (int a = 0; a < 3; ++a) {
    for (int64_t v = 0; v < nv; ++v) Xh[(size_t)v] = xyz[3 * v + a];
    if (dg_upload(d, Xh, &Xd[a], err)) return 1;
  }
  std::vector<int> cell_h((size_t)nl * nc);
  for (int64_t e = 0; e < nc; ++e)
    for (int l = 0; l < nl; ++l) cell_h[(size_t)l * nc + e] = (int)cells[e * nl + l];
  int *cell_d, *nbr_d, *fcell_d, *fv_d, *boff_d, *binc_d;
  unsigned char* finfo_d;
  signed char* flf_d;
  int64_t* brow_d = nullptr;
  if (dg_upload(d, cell_h, &cell_d, err) || dg_upload(d, nbr, &nbr_d, err) || dg_upload(d, finfo, &finfo_d, err) ||
      dg_upload(d, fcell, &fcell_d, err) || dg_upload(d, flf, &flf_d, err) || dg_upload(d, fv, &fv_d, err) ||
      dg_upload(d, boff, &boff_d, err) || dg_upload(d, binc, &binc_d, err) || dg_upload(d, brow, &brow_d, err))
    return 1;
  const size_t blk = (size_t)nl * nl * ncs;
  const int nq = dim == 2 ? 3 : 9;
  double *Jb, *S0, *M0, *bvec, *fw;
  if (dg_zeros(d, (size_t)(1 + nlf) * blk, &Jb, s, err) || dg_zeros(d, blk, &S0, s, err) ||
      dg_zeros(d, blk, &M0, s, err) || dg_zeros(d, (size_t)nT, &bvec, s, err) ||
      dg_zeros(d, (size_t)nq * nf, &fw, s, err))
    return 1;
  const double dt_alpha = g.rb.dt_alpha;
  const dim3 bl(kBlock), gr_r((unsigned)((nT + kBlock - 1) / kBlock)),
      gr_f((unsigned)std::max<int64_t>(1, (nf + kBlock - 1) / kBlock));
  if (dim == 2) {
    hipLaunchKernelGGL((k_umdg_assemble<2>), gr_r, bl, 0, s, nc, ncs, cell_d, Xd[0], Xd[1], Xd[2], nbr_d, finfo_d,
                       dt_alpha, Jb, S0, M0, bvec);
    if (nf) hipLaunchKernelGGL((k_umdg_facet_w<2>), gr_f, bl, 0, s, nf, nc, fcell_d, flf_d, cell_d, Xd[0], Xd[1],
                               Xd[2], fw);
  } else {
    hipLaunchKernelGGL((k_umdg_assemble<3>), gr_r, bl, 0, s, nc, ncs, cell_d, Xd[0], Xd[1], Xd[2], nbr_d, finfo_d,
                       dt_alpha, Jb, S0, M0, bvec);
    if (nf) hipLaunchKernelGGL((k_umdg_facet_w<3>), gr_f, bl, 0, s, nf, nc, fcell_d, flf_d, cell_d, Xd[0], Xd[1],
                               Xd[2], fw);
  }
  UMC(hipGetLastError());
  UMC(hipStreamSynchronize(s));
  for (void* p : {(void*)Xd[0], (void*)Xd[1], (void*)Xd[2], (void*)cell_d, (void*)finfo_d, (void*)fcell_d,
                  (void*)flf_d})
    dg_release(d, p);
  g.dim = dim;
  g.nc = nc;
  g.ncs = ncs;
  g.J = Jb;
  g.S0 = S0;
  g.M0 = M0;
  g.nbr = nbr_d;
  g.bvec = bvec;
  UmGrid& rb = g.rb;  // the Robin tables, rows = DG dofs
  rb.dim = dim;
  rb.nv = rb.nrow = nT;
  rb.nc = nc;
  rb.nf = nf;
  rb.fv = fv_d;
  rb.fw = fw;
  rb.boff = boff_d;
  rb.binc = binc_d;
  rb.brow = brow_d;
  rb.nbr = (int64_t)brow.size();
  return 0;
}
#undef UMC

}  // namespace tv

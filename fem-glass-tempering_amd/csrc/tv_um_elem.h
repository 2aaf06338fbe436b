// Element-local device pieces shared by the general-mesh kernels: the Q1
// reference element and its 3-point Gauss rule, the rows of the isoparametric
// element matrices, and the Robin terms of one row evaluated from per-facet
// quadrature weights.  Used by the CG1 operators (tv_um.hip) and the DG1
// operators (tv_umdg.hip): the Robin rows of both run the same code, over
// vertex dofs there and over the boundary cells' own dofs here.
#pragma once
#include "tv_device.h"

namespace tv {
namespace umk {

enum { UM_RES = 0, UM_JAC = 1, UM_DIAG = 2, UM_FUSED = 3 };

__device__ constexpr double kUX[3] = {0.11270166537925831148, 0.5, 0.88729833462074168852};
__device__ constexpr double kUW[3] = {5.0 / 18.0, 8.0 / 18.0, 5.0 / 18.0};

__device__ __forceinline__ double um_g(const UmGrid& g, double T) {
  const double T2 = T * T;
  return g.a_rad * (T2 * T2 - g.T_amb4) + g.a_conv * (T - g.T_amb);
}
__device__ __forceinline__ double um_dg(const UmGrid& g, double T) { return g.a_rad * 4.0 * (T * T * T) + g.a_conv; }

// Q1 basis and reference gradients at xi (tensor order l = a + 2b + 4c)
template <int D>
__device__ __forceinline__ void q1(const double (&xi)[3], double (&phi)[1 << D], double (&dphi)[1 << D][D]) {
#pragma unroll
  for (int l = 0; l < (1 << D); ++l) {
    double f[3], df[3];
#pragma unroll
    for (int a = 0; a < D; ++a) {
      const int b = (l >> a) & 1;
      f[a] = b ? xi[a] : 1.0 - xi[a];
      df[a] = b ? 1.0 : -1.0;
    }
    double p = 1.0;
#pragma unroll
    for (int a = 0; a < D; ++a) p *= f[a];
    phi[l] = p;
#pragma unroll
    for (int a = 0; a < D; ++a) {
      double q = df[a];
#pragma unroll
      for (int e = 0; e < D; ++e)
        if (e != a) q *= f[e];
      dphi[l][a] = q;
    }
  }
}

// inverse and determinant of a D x D matrix
template <int D>
__device__ __forceinline__ double inv_det(const double (&J)[D][D], double (&Ji)[D][D]) {
  if constexpr (D == 2) {
    const double det = J[0][0] * J[1][1] - J[0][1] * J[1][0];
    const double id = 1.0 / det;
    Ji[0][0] = J[1][1] * id;
    Ji[0][1] = -J[0][1] * id;
    Ji[1][0] = -J[1][0] * id;
    Ji[1][1] = J[0][0] * id;
    return det;
  } else {
    double c[3][3];
    c[0][0] = J[1][1] * J[2][2] - J[1][2] * J[2][1];
    c[0][1] = J[0][2] * J[2][1] - J[0][1] * J[2][2];
    c[0][2] = J[0][1] * J[1][2] - J[0][2] * J[1][1];
    c[1][0] = J[1][2] * J[2][0] - J[1][0] * J[2][2];
    c[1][1] = J[0][0] * J[2][2] - J[0][2] * J[2][0];
    c[1][2] = J[0][2] * J[1][0] - J[0][0] * J[1][2];
    c[2][0] = J[1][0] * J[2][1] - J[1][1] * J[2][0];
    c[2][1] = J[0][1] * J[2][0] - J[0][0] * J[2][1];
    c[2][2] = J[0][0] * J[1][1] - J[0][1] * J[1][0];
    const double det = J[0][0] * c[0][0] + J[0][1] * c[1][0] + J[0][2] * c[2][0];
    const double id = 1.0 / det;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) Ji[a][b] = c[a][b] * id;
    return det;
  }
}

// row l of the element matrices of a cell: Ml[j] = int phi_l phi_j,
// Kl[j] = int grad phi_l . grad phi_j
template <int D>
__device__ __forceinline__ void elem_row(const double (&X)[1 << D][D], int l, double (&Ml)[1 << D],
                                         double (&Kl)[1 << D]) {
  constexpr int NL = 1 << D;
  constexpr int NQ = (D == 2) ? 9 : 27;
#pragma unroll
  for (int j = 0; j < NL; ++j) Ml[j] = Kl[j] = 0.0;
#pragma unroll 1
  for (int q = 0; q < NQ; ++q) {
    const int qi[3] = {q % 3, (q / 3) % 3, q / 9};
    double xi[3] = {0.0, 0.0, 0.0}, w = 1.0;
#pragma unroll
    for (int a = 0; a < D; ++a) {
      xi[a] = kUX[qi[a]];
      w *= kUW[qi[a]];
    }
    double phi[NL], dphi[NL][D];
    q1<D>(xi, phi, dphi);
    double J[D][D];
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
      for (int b = 0; b < D; ++b) {
        double s = 0.0;
#pragma unroll
        for (int m = 0; m < NL; ++m) s += X[m][a] * dphi[m][b];
        J[a][b] = s;
      }
    double Ji[D][D];
    const double wd = w * fabs(inv_det<D>(J, Ji));
    double gp[NL][D];  // grad phi = J^-T dphi
#pragma unroll
    for (int m = 0; m < NL; ++m)
#pragma unroll
      for (int a = 0; a < D; ++a) {
        double s = 0.0;
#pragma unroll
        for (int b = 0; b < D; ++b) s += Ji[b][a] * dphi[m][b];
        gp[m][a] = s;
      }
    double phil = 0.0, gl[D];
#pragma unroll
    for (int a = 0; a < D; ++a) gl[a] = 0.0;
#pragma unroll
    for (int m = 0; m < NL; ++m)
      if (m == l) {
        phil = phi[m];
#pragma unroll
        for (int a = 0; a < D; ++a) gl[a] = gp[m][a];
      }
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      double gg = 0.0;
#pragma unroll
      for (int a = 0; a < D; ++a) gg += gl[a] * gp[j][a];
      Ml[j] += wd * (phil * phi[j]);
      Kl[j] += wd * gg;
    }
  }
}

// facet-local Q1 basis at facet point q: tangential axes in increasing order,
// point index q = i0 + 3 i1 (the product order of q1<D> on the cell)
__device__ __forceinline__ double fphi(int m, int q, int D) {
  const double x0 = kUX[q % 3];
  const double f0 = (m & 1) ? x0 : 1.0 - x0;
  if (D == 2) return f0;
  const double x1 = kUX[q / 3];
  return f0 * ((m >> 1) ? x1 : 1.0 - x1);
}

// Robin terms of row r (ThermoViscoProblem.py:302-304 and their derivative)
template <int D, int MODE, class XGet>
__device__ __forceinline__ double robin_row(const UmGrid& g, int64_t r, const double* __restrict__ T, XGet xget) {
  constexpr int NF = 1 << (D - 1);
  constexpr int NQ = (D == 2) ? 3 : 9;
  double acc = 0.0;
  const int t1 = g.boff[r + 1];
  for (int t = g.boff[r]; t < t1; ++t) {
    const int code = g.binc[t];
    const int64_t f = code >> 2;
    const int m = code & 3;
    double Tn[NF], xn[NF];
#pragma unroll
    for (int n = 0; n < NF; ++n) {
      const int v = g.fv[(int64_t)n * g.nf + f];
      Tn[n] = T[v];
      xn[n] = (MODE == UM_JAC || MODE == UM_FUSED) ? xget(v) : 0.0;
    }
    double y = 0.0;
#pragma unroll 1
    for (int q = 0; q < NQ; ++q) {
      double Tq = 0.0, xq = 0.0, pm = 0.0;
#pragma unroll
      for (int n = 0; n < NF; ++n) {
        const double ph = fphi(n, q, D);
        Tq += ph * Tn[n];
        xq += ph * xn[n];
        if (n == m) pm = ph;
      }
      double v;
      if (MODE == UM_RES) v = um_g(g, Tq) * pm;
      else if (MODE == UM_DIAG) v = um_dg(g, Tq) * pm * pm;
      else v = um_dg(g, Tq) * xq * pm;
      y += g.fw[(int64_t)q * g.nf + f] * v;
    }
    acc += g.dt * y;
  }
  return acc;
}

}  // namespace umk
}  // namespace tv

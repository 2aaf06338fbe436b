// Ensemble of independent 1D bars with DG1 temperature and CG1 stress (the
// pairing of main.py's fe_config), gfx950: the whole time loop of thousands of
// bars in one launch.  This file holds the discretisation and its solver; the
// step, Newton and record logic, the failure contract and the mapping are
// csrc/tv_ensemble_step.h, shared with the CG1 / CG1 kernel (csrc/tv_ensemble.hip).
//
// EnsArgs' n_nodes counts the mesh nodes: nS = n_nodes sigma dofs and
// nT = 2 (n_nodes - 1) temperature dofs per bar.  T dofs are numbered 2 c + l
// (cell c, local vertex l), the oracle's DG dofmap.
//
// Per Newton iteration and lane (oracle/tv_oracle.py, HeatForm on a DG1 interval mesh),
// with a_c = T[2c], b_c = T[2c+1], cm = h_c / 6, ck = dt alpha / h_c:
//   cell     mass cm [2 1; 1 2] (T - T_prev), stiffness ck [1 -1; -1 1] T,
//            source -dt f h / 2 per dof;
//   Robin    at dof 0 and dof nT - 1, dt 0.001 (sigma eps (T^4 - Ta^4) + htc (T - Ta))
//            and its derivative on the diagonal (set_boundary);
//   SIPG     per interior node between cell c ('+', the lower index: penalty
//            5 / h_c) and cell c + 1, with j = b_c - a_{c+1} and G_c = ck_c (b_c - a_c)
//            (dt alpha times the cell's gradient):
//              row a_c      + ck_c j / 2
//              row b_c      + 5 ck_c j - ck_c j / 2 - (G_c + G_{c+1}) / 2
//              row a_{c+1}  - 5 ck_c j + ck_{c+1} j / 2 + (G_c + G_{c+1}) / 2
//              row b_{c+1}  - ck_{c+1} j / 2
//            so the two coefficient tables of the CG kernel are all it reads;
//   Jacobian the constant matrices of these terms plus the Robin derivative:
//            block tridiagonal, 2x2 blocks per cell, symmetric positive definite.
//            Solved per lane by block forward elimination without pivoting,
//              D'_c = D_c - L_c C_{c-1},  C_c = D'_c^-1 U_c,  d_c = D'_c^-1 (F_c - L_c d_{c-1}),
//            the 2x2 inverse by adjugate and determinant (one division per
//            cell), the rows assembled inside the sweep; C_c and d_c go to the
//            scratch [6][n_cells][bar]; the back sweep forms dx_c = d_c - C_c dx_{c+1},
//            rewrites T <- T - dx and accumulates ||dx||^2.
// The sigma <- T map is the oracle's, "last cell in cell order wins":
// src(i) = 2 i, src(n_cells) = 2 n_cells - 1.  So dof 2c feeds sigma node c,
// the last dof feeds node n_cells, and a probe (a mesh node) reads T and Tf at
// src(node).
//
// No address depends on the recurrences: the forward sweep walks the cells in
// chunks of kChunk, the back substitution in chunks of kChunkB, and each issues
// the loads of the next chunk before the chain of the current one.
#include "tv_ensemble_step.h"

namespace tv {
namespace {

// cells whose loads are in flight ahead of the recurrence: 12 loads per cell in the forward sweep, 8 in the
// back substitution (2 / 2 takes 252 VGPRs and, in the kExt instantiation, one wave per SIMD)
constexpr int kChunk = 2, kChunkB = 1;

struct Dg1 {
  static __device__ __forceinline__ int n_T(const EnsArgs& a) { return 2 * (a.n_nodes - 1); }
  // dof 2 c is the source of sigma node c, dof nT - 1 that of node n_cells; the other odd dofs feed no node
  static __device__ __forceinline__ int sigma_node(const EnsArgs& a, int i) {
    return (i & 1) == 0 ? i >> 1 : (i == n_T(a) - 1 ? a.n_nodes - 1 : -1);
  }
  static __device__ __forceinline__ int source_dof(const EnsArgs& a, int node) {
    return node < a.n_nodes - 1 ? 2 * node : n_T(a) - 1;
  }
  static __device__ __forceinline__ double newton_iteration(const EnsArgs& a, const Bar& b, int64_t bar);
};

// T, T_prev and the coefficients of cells base + 1 .. base + kChunk, the cell
// index clamped to the bar (what the clamp repeats is only ever used under a
// coefficient that is set to zero for the missing cell)
struct FwdChunk {
  double a[kChunk], b[kChunk], pa[kChunk], pb[kChunk], cm[kChunk], ck[kChunk];
};

__device__ __forceinline__ void load_fwd(const EnsArgs& a, int64_t bar, int base, FwdChunk& q) {
  const int nc = a.n_nodes - 1;
#pragma unroll
  for (int k = 0; k < kChunk; ++k) {
    const int ic = min(base + 1 + k, nc - 1);
    const int64_t t = (int64_t)(2 * ic) * a.nb_pad + bar;
    q.a[k] = a.T[t];
    q.b[k] = a.T[t + a.nb_pad];
    q.pa[k] = a.Tp[t];
    q.pb[k] = a.Tp[t + a.nb_pad];
    q.cm[k] = a.cm[(int64_t)ic * a.nb_pad + bar];
    q.ck[k] = a.ck[(int64_t)ic * a.nb_pad + bar];
  }
}

// C (row-major), d and the two T dofs of cells top .. top - kChunkB + 1
struct BackChunk {
  double C[kChunkB][4], d[kChunkB][2], a[kChunkB], b[kChunkB];
};

__device__ __forceinline__ void load_back(const EnsArgs& a, int64_t bar, int top, BackChunk& q) {
  const int64_t plane = (int64_t)(a.n_nodes - 1) * a.nb_pad;
#pragma unroll
  for (int k = 0; k < kChunkB; ++k) {
    const int ic = max(top - k, 0);
    const int64_t s = (int64_t)ic * a.nb_pad + bar;
#pragma unroll
    for (int m = 0; m < 4; ++m) q.C[k][m] = a.scr[m * plane + s];
    q.d[k][0] = a.scr[4 * plane + s];
    q.d[k][1] = a.scr[5 * plane + s];
    const int64_t t = (int64_t)(2 * ic) * a.nb_pad + bar;
    q.a[k] = a.T[t];
    q.b[k] = a.T[t + a.nb_pad];
  }
}

// One Newton iteration: assemble F(T) and J(T) cell by cell inside the block
// forward elimination, back-substitute, T <- T - dx.  Returns ||dx||^2.
__device__ __forceinline__ double Dg1::newton_iteration(const EnsArgs& a, const Bar& b, int64_t bar) {
  const int nc = a.n_nodes - 1;
  const int64_t plane = (int64_t)nc * a.nb_pad;
  // ---- forward sweep
  double bm = 0.0, ckm = 0.0, Gm = 0.0;  // cell c - 1 (c = 0: no such cell, every use is under ckm = 0)
  double a0 = a.T[bar], b0 = a.T[a.nb_pad + bar];
  double da = a0 - a.Tp[bar], db = b0 - a.Tp[a.nb_pad + bar];  // T - T_prev formed before the mass product
  double cm0 = a.cm[bar], ck0 = a.ck[bar];
  double G0 = ck0 * (b0 - a0);
  double c00 = 0.0, c01 = 0.0, c10 = 0.0, c11 = 0.0, d0 = 0.0, d1 = 0.0;  // C and d of cell c - 1
  FwdChunk cur, nxt;
  load_fwd(a, bar, 0, cur);
  nxt = cur;
  for (int base = 0; base < nc; base += kChunk) {
    if (base + kChunk < nc) load_fwd(a, bar, base + kChunk, nxt);
#pragma unroll
    for (int k = 0; k < kChunk; ++k) {
      const int c = base + k;
      if (c < nc) {
        const bool first = c == 0, last = c == nc - 1;
        const double a1 = cur.a[k], b1 = cur.b[k];
        const double Gn = cur.ck[k] * (b1 - a1);
        const double ck1 = last ? 0.0 : cur.ck[k];  // the facet above: none on the last cell
        const double G1 = last ? 0.0 : Gn;
        const double ckR = last ? 0.0 : ck0, GR = last ? 0.0 : G0;
        const double ckL = first ? 0.0 : ck0, GL = first ? 0.0 : G0;  // the facet below: none on the first
        const double jL = bm - a0, jR = b0 - a1;
        const double src = b.dtf * (3.0 * cm0);
        double Fa = (cm0 * (2.0 * da + db) - G0) - src;
        double Fb = (cm0 * (da + 2.0 * db) + G0) - src;
        Fa += ((0.5 * ckL) * jL - (5.0 * ckm) * jL + 0.5 * (Gm + GL)) + (0.5 * ckR) * jR;
        Fb += ((5.0 * ckR) * jR - (0.5 * ckR) * jR - 0.5 * (GR + G1)) - (0.5 * ckL) * jL;
        double D00 = (2.0 * cm0 + ck0) + (5.0 * ckm - ckL);
        const double D01 = (cm0 - ck0) + 0.5 * (ckL + ckR);
        double D11 = (2.0 * cm0 + ck0) + 4.0 * ckR;
        if (first) {
          const double T2 = a0 * a0;
          Fa += b.dt * (b.a_rad * (T2 * T2 - b.T_amb4) + b.a_conv * (a0 - b.T_amb));
          D00 += b.dt * (b.a_rad * (4.0 * (T2 * a0)) + b.a_conv);
        }
        if (last) {
          const double T2 = b0 * b0;
          Fb += b.dt * (b.a_rad * (T2 * T2 - b.T_amb4) + b.a_conv * (b0 - b.T_amb));
          D11 += b.dt * (b.a_rad * (4.0 * (T2 * b0)) + b.a_conv);
        }
        // U_c = [U00 0; U10 U11], L_c = U_{c-1}^T = [L00 L01; 0 L11]
        const double U00 = -0.5 * ckR, U10 = 0.5 * ck1 - 4.5 * ckR, U11 = -0.5 * ck1;
        const double L00 = -0.5 * ckm, L01 = 0.5 * ckL - 4.5 * ckm, L11 = -0.5 * ckL;
        const double E00 = D00 - (L00 * c00 + L01 * c10);
        const double E01 = D01 - (L00 * c01 + L01 * c11);
        const double E10 = D01 - L11 * c10;
        const double E11 = D11 - L11 * c11;
        const double r0 = Fa - (L00 * d0 + L01 * d1);
        const double r1 = Fb - L11 * d1;
        const double idet = 1.0 / (E00 * E11 - E01 * E10);
        const double i00 = E11 * idet, i01 = -(E01 * idet), i10 = -(E10 * idet), i11 = E00 * idet;
        c00 = i00 * U00 + i01 * U10;
        c01 = i01 * U11;
        c10 = i10 * U00 + i11 * U10;
        c11 = i11 * U11;
        d0 = i00 * r0 + i01 * r1;
        d1 = i10 * r0 + i11 * r1;
        const int64_t s = (int64_t)c * a.nb_pad + bar;
        a.scr[s] = c00;
        a.scr[plane + s] = c01;
        a.scr[2 * plane + s] = c10;
        a.scr[3 * plane + s] = c11;
        a.scr[4 * plane + s] = d0;
        a.scr[5 * plane + s] = d1;
        bm = b0; ckm = ck0; Gm = G0;
        a0 = a1; b0 = b1; da = a1 - cur.pa[k]; db = b1 - cur.pb[k];
        cm0 = cur.cm[k]; ck0 = cur.ck[k]; G0 = Gn;
      }
    }
    cur = nxt;
  }
  // ---- back substitution (the last cell has C = 0, so dx = d there)
  double x0 = 0.0, x1 = 0.0, nrm2 = 0.0;
  BackChunk bc, bn;
  load_back(a, bar, nc - 1, bc);
  bn = bc;
  for (int top = nc - 1; top >= 0; top -= kChunkB) {
    if (top - kChunkB >= 0) load_back(a, bar, top - kChunkB, bn);
#pragma unroll
    for (int k = 0; k < kChunkB; ++k) {
      const int c = top - k;
      if (c >= 0) {
        const double y0 = bc.d[k][0] - (bc.C[k][0] * x0 + bc.C[k][1] * x1);
        const double y1 = bc.d[k][1] - (bc.C[k][2] * x0 + bc.C[k][3] * x1);
        x0 = y0;
        x1 = y1;
        const int64_t t = (int64_t)(2 * c) * a.nb_pad + bar;
        a.T[t] = bc.a[k] - x0;
        a.T[t + a.nb_pad] = bc.b[k] - x1;
        nrm2 += x1 * x1 + x0 * x0;
      }
    }
    bc = bn;
  }
  return nrm2;
}

template <bool kExt, int kModel>
__global__ __launch_bounds__(kWave) void k_ensemble_dg(EnsArgs a, ViscoConst c, ViscoFields f,
                                                       const EnsExt* __restrict__ x) {
  ensemble_bar<Dg1, kExt, kModel>(a, c, f, x);
}

}  // namespace

// the model mode is the handle's (ViscoConst::paper: 0 reference, 1 paper, 2 paper with the exact
// relaxation), the scheduled instantiation runs when x is given
void launch_ensemble_dg(const EnsArgs& a, const ViscoConst& c, const ViscoFields& f, const EnsExt* x, hipStream_t s) {
  const dim3 grid(a.nb_pad / kWave), block(kWave);
  dispatch_ensemble(c.paper, x != nullptr, [&](auto ext, auto model) {
    hipLaunchKernelGGL((k_ensemble_dg<decltype(ext)::value, decltype(model)::value>), grid, block, 0, s, a, c, f, x);
  });
}

}  // namespace tv

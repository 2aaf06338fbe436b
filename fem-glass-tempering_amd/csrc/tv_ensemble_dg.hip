// Ensemble of independent 1D bars with DG1 temperature and CG1 stress (the
// pairing of main.py's fe_config), gfx950: the whole time loop of thousands of
// bars in one launch.  The CG1 / CG1 kernel is csrc/tv_ensemble.hip; this file
// keeps its mapping and restates its step, stage and record logic.
//
// Mapping: one lane per bar, a wave = 64 consecutive bars, one wave per
// workgroup.  No LDS, no barriers, no cross-lane operations: a bar computes the
// same bits alone or in any ensemble.  Layout: bar-fastest, [component][dof][bar]
// (EnsArgs; n_nodes counts the mesh nodes, nS = n_nodes sigma dofs and
// nT = 2 (n_nodes - 1) temperature dofs per bar), every load / store of a wave
// one contiguous 512-byte segment.  T dofs are numbered 2 c + l (cell c, local
// vertex l), the oracle's DG dofmap.
//
// Per step and lane (oracle/tv_oracle.py, HeatForm on a DG1 interval mesh),
// with a_c = T[2c], b_c = T[2c+1], cm = h_c / 6, ck = dt alpha / h_c:
//   cell     mass cm [2 1; 1 2] (T - T_prev), stiffness ck [1 -1; -1 1] T,
//            source -dt f h / 2 per dof;
//   Robin    at dof 0 and dof nT - 1, dt 0.001 (sigma eps (T^4 - Ta^4) + htc (T - Ta))
//            and its derivative on the diagonal (set_boundary of the CG kernel);
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
//            rewrites T <- T - dx and accumulates ||dx||^2;
//   Newton   as k_ensemble: iteration 1 records ||dx_1||, afterwards converged
//            iff ||dx|| / ||dx_1|| < rtol or ||dx|| < atol, at most max_it;
//   visco    t_part at dof 2c, s_part at sigma node c with that state; t_part
//            at dof 2c + 1, and for the last cell s_part at node n_cells with
//            it (the oracle's sigma <- T map, "last cell in cell order wins":
//            src(i) = 2 i, src(n_cells) = 2 n_cells - 1); then T_prev <- T.
// Failure contract, thermal_only, statistics, schedules and probe records are
// those of k_ensemble; a probe is a mesh node, T and Tf are recorded at its
// source dof and sigma at the node.
//
// No address depends on the recurrences: the forward sweep walks the cells in
// chunks of kChunk, the back substitution in chunks of kChunkB, and each issues
// the loads of the next chunk before the chain of the current one.
#include "tv_internal.h"
#include "tv_visco_point.h"

namespace tv {
namespace {

// cells whose loads are in flight ahead of the recurrence: 12 loads per cell in the forward sweep, 8 in the
// back substitution (2 / 2 takes 252 VGPRs and, in the kExt instantiation, one wave per SIMD)
constexpr int kChunk = 2, kChunkB = 1;

struct Bar {
  double a_rad, a_conv, T_amb, T_amb4, dt, dtf;
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
__device__ __forceinline__ double newton_iteration(const EnsArgs& a, const Bar& b, int64_t bar) {
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

// The bar's Robin coefficients from its (current stage's) htc, T_ambient, epsilon
__device__ __forceinline__ void set_boundary(Bar& b, double sigma_sb, double htc, double Ta, double eps) {
  const double Ta2 = Ta * Ta;
  b.a_rad = 0.001 * (sigma_sb * eps);
  b.a_conv = 0.001 * htc;
  b.T_amb = Ta;
  b.T_amb4 = Ta2 * Ta2;
}

// kExt as in k_ensemble: false = constant boundary values, final state only
// (x is not read); true = per-bar stage tables and / or probe records (EnsExt).
template <bool kExt>
__global__ __launch_bounds__(kWave) void k_ensemble_dg(EnsArgs a, ViscoConst c, ViscoFields f,
                                                       const EnsExt* __restrict__ x) {
  const int64_t bar = blockIdx.x * (int64_t)kWave + threadIdx.x;
  if (bar >= a.n_bars) return;          // tail lanes: no memory access
  if (a.failed_step[bar] != 0) return;  // frozen by an earlier failure
  const int nc = a.n_nodes - 1, nT = 2 * nc;
  Bar b;
  set_boundary(b, a.sigma_sb, a.htc[bar], a.T_amb[bar], a.eps[bar]);
  b.dt = a.dt;
  b.dtf = a.dt * a.f[bar];
  // kExt: the bar's stage and that stage's last step (the host has dropped the
  // empty stages of each bar and closed its list with INT32_MAX)
  int stage = 0, stage_last = INT32_MAX;
  if constexpr (kExt) {
    if (x->n_stages > 0) {
      stage_last = x->stage_end[bar];
      while (a.step_base + 1 > stage_last) {  // ends at the latest in the bar's last row (INT32_MAX)
        ++stage;
        stage_last = x->stage_end[(int64_t)stage * a.nb_pad + bar];
      }
      const int64_t t = (int64_t)stage * a.nb_pad + bar;
      set_boundary(b, a.sigma_sb, x->htc[t], x->T_amb[t], x->eps[t]);
    }
  }
  int its = 0, failed = 0;
  int64_t total = 0;
  for (int s = 0; s < a.n_steps; ++s) {
    if constexpr (kExt) {
      if (a.step_base + s + 1 > stage_last) {
        ++stage;
        const int64_t t = (int64_t)stage * a.nb_pad + bar;
        stage_last = x->stage_end[t];
        set_boundary(b, a.sigma_sb, x->htc[t], x->T_amb[t], x->eps[t]);
      }
    }
    its = 0;
    bool conv = false;
    double r0 = 0.0;
    while (!conv && its < a.max_it) {
      const double r = sqrt(newton_iteration(a, b, bar));
      ++its;
      if (its == 1) {
        r0 = r;
      } else {
        const double rel = r / r0;  // r0 == 0: NaN (r == 0) or inf, never < rtol
        conv = rel < a.rtol || r < a.atol;
      }
    }
    total += its;
    if (!conv) {  // the step does not end: T <- T_prev, visco state untouched
      for (int i = 0; i < nT; ++i) a.T[(int64_t)i * a.nb_pad + bar] = a.Tp[(int64_t)i * a.nb_pad + bar];
      failed = a.step_base + s + 1;
      break;
    }
    if (a.thermal_only) {
      for (int i = 0; i < nT; ++i) a.Tp[(int64_t)i * a.nb_pad + bar] = a.T[(int64_t)i * a.nb_pad + bar];
    } else {
      bool dirty = false;  // LEAN bookkeeping of s_part, unused here
      // dof 2 c is the source of sigma node c, dof nT - 1 that of node n_cells; the other odd dofs feed no node
      for (int i = 0; i < nT; ++i) {
        const int64_t t = (int64_t)i * a.nb_pad + bar;
        const TState ts = t_part<false, false>(c, f, t);
        const int node = (i & 1) == 0 ? i >> 1 : (i == nT - 1 ? nc : -1);  // wave-uniform
        if (node >= 0) s_part<1, false, false>(c, f, (int64_t)node * a.nb_pad + bar, ts, dirty);
        f.Tp[t] = ts.T;
      }
    }
    if constexpr (kExt) {
      // record step / every - 1 of [record][field][probe][bar]: T and Tf at the probe node's source dof,
      // sigma at the node (the host refuses steps past max_records * every; the bound here only keeps
      // the stores inside)
      const int step = a.step_base + s + 1;
      if (x->n_probes > 0 && step % x->every == 0 && step / x->every <= x->max_records) {
        const int64_t rec = (int64_t)(step / x->every - 1) * 3 * x->n_probes;
        for (int p = 0; p < x->n_probes; ++p) {
          const int node = x->probes[p];
          const int64_t t = (int64_t)(node < nc ? 2 * node : nT - 1) * a.nb_pad + bar;
          x->hist[(rec + p) * a.nb_pad + bar] = a.T[t];
          x->hist[(rec + x->n_probes + p) * a.nb_pad + bar] = f.Tf[t];
          x->hist[(rec + 2 * x->n_probes + p) * a.nb_pad + bar] = f.sigma[(int64_t)node * a.nb_pad + bar];
        }
      }
    }
  }
  a.its_last[bar] = its;
  a.newton_total[bar] += total;
  if (failed) a.failed_step[bar] = failed;
}

}  // namespace

void launch_ensemble_dg(const EnsArgs& a, const ViscoConst& c, const ViscoFields& f, const EnsExt* x, hipStream_t s) {
  if (x) hipLaunchKernelGGL(k_ensemble_dg<true>, dim3(a.nb_pad / kWave), dim3(kWave), 0, s, a, c, f, x);
  else hipLaunchKernelGGL(k_ensemble_dg<false>, dim3(a.nb_pad / kWave), dim3(kWave), 0, s, a, c, f, nullptr);
}

}  // namespace tv

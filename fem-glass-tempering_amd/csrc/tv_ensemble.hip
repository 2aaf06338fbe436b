// Ensemble of independent 1D CG1 tempering bars, gfx950: the whole time loop of
// thousands of bars in one launch.  This file holds the discretisation and its
// solver; the step, Newton and record logic, the failure contract and the
// mapping are csrc/tv_ensemble_step.h, shared with the DG1 kernel.
//
// Per Newton iteration and lane (oracle/tv_oracle.py on a CG1 interval mesh):
//   residual  F = M (T - T_prev) + dt alpha K T - dt f int v, consistent mass
//             h/6 [2 1; 1 2], stiffness 1/h [1 -1; -1 1], plus at the two end
//             nodes dt 0.001 (sigma eps (T^4 - Ta^4) + htc (T - Ta))
//             (HeatForm.residual; in 1D a facet is a point of measure 1);
//   Jacobian  tridiagonal M + dt alpha K, plus dt 0.001 (4 sigma eps T^3 + htc)
//             on the two end diagonals (HeatForm.jacobian): SPD and
//             diagonally dominant, solved by the Thomas algorithm, no pivoting.
// T dof i is mesh node i: it feeds sigma node i and a probe reads it.
//
// The Thomas recurrences are one dependent divide chain per bar, but no
// address depends on them: both sweeps walk the nodes in chunks of kChunk and
// issue the loads of the next chunk before the chain of the current one.
#include "tv_ensemble_step.h"

namespace tv {
namespace {

constexpr int kChunk = 4;  // nodes whose loads are in flight ahead of the recurrence

struct Cg1 {
  static __device__ __forceinline__ int n_T(const EnsArgs& a) { return a.n_nodes; }
  static __device__ __forceinline__ int sigma_node(const EnsArgs&, int i) { return i; }
  static __device__ __forceinline__ int source_dof(const EnsArgs&, int node) { return node; }
  static __device__ __forceinline__ double newton_iteration(const EnsArgs& a, const Bar& b, int64_t bar);
};

// T, T_prev of nodes base + 1 .. base + kChunk and the coefficients of cells
// base .. base + kChunk - 1, indices clamped to the bar (the clamped values are
// only ever multiplied by the zero coefficients of the missing cell)
struct FwdChunk {
  double T[kChunk], Tp[kChunk], cm[kChunk], ck[kChunk];
};

__device__ __forceinline__ void load_fwd(const EnsArgs& a, int64_t bar, int base, FwdChunk& q) {
  const int n = a.n_nodes;
#pragma unroll
  for (int k = 0; k < kChunk; ++k) {
    const int in = min(base + 1 + k, n - 1);
    const int ic = min(base + k, n - 2);
    q.T[k] = a.T[(int64_t)in * a.nb_pad + bar];
    q.Tp[k] = a.Tp[(int64_t)in * a.nb_pad + bar];
    q.cm[k] = a.cm[(int64_t)ic * a.nb_pad + bar];
    q.ck[k] = a.ck[(int64_t)ic * a.nb_pad + bar];
  }
}

// modified upper diagonal, right-hand side and T of nodes top .. top - kChunk + 1
struct BackChunk {
  double cp[kChunk], dp[kChunk], T[kChunk];
};

__device__ __forceinline__ void load_back(const EnsArgs& a, int64_t bar, int top, BackChunk& q) {
  const int64_t plane = (int64_t)a.n_nodes * a.nb_pad;
#pragma unroll
  for (int k = 0; k < kChunk; ++k) {
    const int i = max(top - k, 0);
    q.cp[k] = a.scr[(int64_t)i * a.nb_pad + bar];
    q.dp[k] = a.scr[plane + (int64_t)i * a.nb_pad + bar];
    q.T[k] = a.T[(int64_t)i * a.nb_pad + bar];
  }
}

// One Newton iteration: assemble F(T) and J(T) row by row inside the Thomas
// forward sweep, back-substitute, T <- T - dx.  Returns ||dx||^2.
__device__ __forceinline__ double Cg1::newton_iteration(const EnsArgs& a, const Bar& b, int64_t bar) {
  const int n = a.n_nodes;
  const int64_t plane = (int64_t)n * a.nb_pad;
  // ---- forward sweep
  double Tm = 0.0, dm = 0.0;  // node i - 1 (i = 0: multiplied by cml = ckl = 0)
  double T0 = a.T[bar];
  double d0 = T0 - a.Tp[bar];  // T - T_prev formed before the mass product
  double cml = 0.0, ckl = 0.0;  // cell below node i
  double cpp = 0.0, dpp = 0.0;  // modified upper diagonal / right-hand side of row i - 1
  FwdChunk cur, nxt;
  load_fwd(a, bar, 0, cur);
  nxt = cur;
  for (int base = 0; base < n; base += kChunk) {
    if (base + kChunk < n) load_fwd(a, bar, base + kChunk, nxt);
#pragma unroll
    for (int k = 0; k < kChunk; ++k) {
      const int i = base + k;
      if (i < n) {
        const bool last = i == n - 1;
        const double cmh = last ? 0.0 : cur.cm[k];
        const double ckh = last ? 0.0 : cur.ck[k];
        const double T1 = cur.T[k];
        const double d1 = T1 - cur.Tp[k];
        double F = (cml * (dm + 2.0 * d0) + cmh * (2.0 * d0 + d1)) + (ckl * (T0 - Tm) + ckh * (T0 - T1)) -
                   b.dtf * (3.0 * (cml + cmh));
        double diag = 2.0 * (cml + cmh) + (ckl + ckh);
        if (i == 0 || last) {
          const double T2 = T0 * T0;
          F += b.dt * (b.a_rad * (T2 * T2 - b.T_amb4) + b.a_conv * (T0 - b.T_amb));
          diag += b.dt * (b.a_rad * (4.0 * (T2 * T0)) + b.a_conv);
        }
        const double lo = cml - ckl, up = cmh - ckh;
        const double inv = 1.0 / (diag - lo * cpp);
        cpp = up * inv;
        dpp = (F - lo * dpp) * inv;
        a.scr[(int64_t)i * a.nb_pad + bar] = cpp;
        a.scr[plane + (int64_t)i * a.nb_pad + bar] = dpp;
        Tm = T0; dm = d0; T0 = T1; d0 = d1; cml = cmh; ckl = ckh;
      }
    }
    cur = nxt;
  }
  // ---- back substitution (row n - 1 has cp = 0, so dx = dp there)
  double dx = 0.0, nrm2 = 0.0;
  BackChunk bc, bn;
  load_back(a, bar, n - 1, bc);
  bn = bc;
  for (int top = n - 1; top >= 0; top -= kChunk) {
    if (top - kChunk >= 0) load_back(a, bar, top - kChunk, bn);
#pragma unroll
    for (int k = 0; k < kChunk; ++k) {
      const int i = top - k;
      if (i >= 0) {
        dx = bc.dp[k] - bc.cp[k] * dx;
        a.T[(int64_t)i * a.nb_pad + bar] = bc.T[k] - dx;
        nrm2 += dx * dx;
      }
    }
    bc = bn;
  }
  return nrm2;
}

template <bool kExt, int kModel>
__global__ __launch_bounds__(kWave) void k_ensemble(EnsArgs a, ViscoConst c, ViscoFields f,
                                                    const EnsExt* __restrict__ x) {
  ensemble_bar<Cg1, kExt, kModel>(a, c, f, x);
}

}  // namespace

// the model mode is the handle's (ViscoConst::paper: 0 reference, 1 paper, 2 paper with the exact
// relaxation), the scheduled instantiation runs when x is given
void launch_ensemble(const EnsArgs& a, const ViscoConst& c, const ViscoFields& f, const EnsExt* x, hipStream_t s) {
  const dim3 grid(a.nb_pad / kWave), block(kWave);
  dispatch_ensemble(c.paper, x != nullptr, [&](auto ext, auto model) {
    hipLaunchKernelGGL((k_ensemble<decltype(ext)::value, decltype(model)::value>), grid, block, 0, s, a, c, f, x);
  });
}

}  // namespace tv

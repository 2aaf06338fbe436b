// Ensemble of independent 1D CG1 tempering bars, gfx950: the whole time loop of
// thousands of bars in one launch.
//
// Mapping: one lane per bar, a wave = 64 consecutive bars, one wave per
// workgroup (so a small ensemble spreads over the CUs).  No LDS, no barriers,
// no cross-lane operations: a bar's arithmetic never depends on its
// neighbours in the wave, so a bar computes the same bits alone or in any
// ensemble.  Layout: bar-fastest, [component][node][bar] (EnsArgs), every
// load / store of a wave one contiguous 512-byte segment.
//
// Per step and lane (oracle/tv_oracle.py on a CG1 interval mesh):
//   residual  F = M (T - T_prev) + dt alpha K T - dt f int v, consistent mass
//             h/6 [2 1; 1 2], stiffness 1/h [1 -1; -1 1], plus at the two end
//             nodes dt 0.001 (sigma eps (T^4 - Ta^4) + htc (T - Ta))
//             (HeatForm.residual; in 1D a facet is a point of measure 1);
//   Jacobian  tridiagonal M + dt alpha K, plus dt 0.001 (4 sigma eps T^3 + htc)
//             on the two end diagonals (HeatForm.jacobian): SPD and
//             diagonally dominant, solved by the Thomas algorithm, no pivoting;
//   Newton    newton_solve restated: T <- T - dx, iteration 1 records
//             ||dx_1||, afterwards converged iff ||dx|| / ||dx_1|| < rtol or
//             ||dx|| < atol (||dx_1|| = 0: the quotient is NaN or inf and atol
//             decides, as in the oracle), at most max_it iterations;
//   visco     t_part / s_part of tv_visco_point.h per node (D = 1, reference
//             mode, stored s_tilde / sigma_tilde), then T_prev <- T.
// A bar whose Newton solve ends unconverged gets T <- T_prev, keeps the visco
// state of the previous step (tv_step's contract) and is frozen: failed_step
// records the step and the lane does nothing from then on.  Lanes of a wave
// converge at different Newton counts; a converged lane idles until the
// slowest bar of its wave is done.
//
// Process schedules and probe histories (EnsExt, the kExt instantiation): a
// bar's htc / T_ambient / epsilon may change at per-bar step numbers, the
// values of step s being those of the stage that holds s (the new time level,
// as every other implicit Euler term); and after every `every`-th step the
// lane stores T, Tf and sigma at a few shared probe nodes into
// [record][field][probe][bar], one contiguous segment per store of a wave.  A
// failed bar stores nothing more.  Without either the plain instantiation runs.
//
// The Thomas recurrences are one dependent divide chain per bar, but no
// address depends on them: both sweeps walk the nodes in chunks of kChunk and
// issue the loads of the next chunk before the chain of the current one.
#include "tv_internal.h"
#include "tv_visco_point.h"

namespace tv {
namespace {

constexpr int kChunk = 4;  // nodes whose loads are in flight ahead of the recurrence

struct Bar {
  double a_rad, a_conv, T_amb, T_amb4, dt, dtf;
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
__device__ __forceinline__ double newton_iteration(const EnsArgs& a, const Bar& b, int64_t bar) {
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

// The bar's Robin coefficients from its (current stage's) htc, T_ambient, epsilon
__device__ __forceinline__ void set_boundary(Bar& b, double sigma_sb, double htc, double Ta, double eps) {
  const double Ta2 = Ta * Ta;
  b.a_rad = 0.001 * (sigma_sb * eps);
  b.a_conv = 0.001 * htc;
  b.T_amb = Ta;
  b.T_amb4 = Ta2 * Ta2;
}

// kExt = false: constant boundary values, final state only; x is not read and
// the instructions are those of the kernel before schedules existed.
// kExt = true: per-bar stage tables and / or probe records (EnsExt).  A lane
// keeps its own stage and that stage's last step; both follow from the
// absolute step alone, so a launch may start at any step.  Lanes of a wave
// may sit in different stages: that predicates the reload of three values,
// no address pattern changes.
template <bool kExt>
__global__ __launch_bounds__(kWave) void k_ensemble(EnsArgs a, ViscoConst c, ViscoFields f, const EnsExt* __restrict__ x) {
  const int64_t bar = blockIdx.x * (int64_t)kWave + threadIdx.x;
  if (bar >= a.n_bars) return;        // tail lanes: no memory access
  if (a.failed_step[bar] != 0) return;  // frozen by an earlier failure
  const int n = a.n_nodes;
  Bar b;
  {
    const double Ta = a.T_amb[bar];
    const double Ta2 = Ta * Ta;
    b.a_rad = 0.001 * (a.sigma_sb * a.eps[bar]);
    b.a_conv = 0.001 * a.htc[bar];
    b.T_amb = Ta;
    b.T_amb4 = Ta2 * Ta2;
    b.dt = a.dt;
    b.dtf = a.dt * a.f[bar];
  }
  // kExt: the bar's stage and that stage's last step.  The host has dropped the
  // empty stages of each bar and closed its list with INT32_MAX, so the ends
  // rise strictly and passing one means exactly the next row.
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
      for (int i = 0; i < n; ++i) a.T[(int64_t)i * a.nb_pad + bar] = a.Tp[(int64_t)i * a.nb_pad + bar];
      failed = a.step_base + s + 1;
      break;
    }
    if (a.thermal_only) {
      for (int i = 0; i < n; ++i) a.Tp[(int64_t)i * a.nb_pad + bar] = a.T[(int64_t)i * a.nb_pad + bar];
    } else {
      bool dirty = false;  // LEAN bookkeeping of s_part, unused here
      for (int i = 0; i < n; ++i) {
        const int64_t t = (int64_t)i * a.nb_pad + bar;
        const TState ts = t_part<false, false>(c, f, t);
        s_part<1, false, false>(c, f, t, ts, dirty);
        f.Tp[t] = ts.T;
      }
    }
    if constexpr (kExt) {
      // record step / every - 1 of [record][field][probe][bar]: T, Tf, sigma as this step left them
      // (the host refuses steps past max_records * every; the bound here only keeps the stores inside)
      const int step = a.step_base + s + 1;
      if (x->n_probes > 0 && step % x->every == 0 && step / x->every <= x->max_records) {
        const int64_t rec = (int64_t)(step / x->every - 1) * 3 * x->n_probes;
        for (int p = 0; p < x->n_probes; ++p) {
          const int64_t t = (int64_t)x->probes[p] * a.nb_pad + bar;
          x->hist[(rec + p) * a.nb_pad + bar] = a.T[t];
          x->hist[(rec + x->n_probes + p) * a.nb_pad + bar] = f.Tf[t];
          x->hist[(rec + 2 * x->n_probes + p) * a.nb_pad + bar] = f.sigma[t];
        }
      }
    }
  }
  a.its_last[bar] = its;
  a.newton_total[bar] += total;
  if (failed) a.failed_step[bar] = failed;
}

}  // namespace

void launch_ensemble(const EnsArgs& a, const ViscoConst& c, const ViscoFields& f, const EnsExt* x, hipStream_t s) {
  if (x) hipLaunchKernelGGL(k_ensemble<true>, dim3(a.nb_pad / kWave), dim3(kWave), 0, s, a, c, f, x);
  else hipLaunchKernelGGL(k_ensemble<false>, dim3(a.nb_pad / kWave), dim3(kWave), 0, s, a, c, f, nullptr);
}

}  // namespace tv

// The time loop of one ensemble bar, shared by the CG1 (tv_ensemble.hip) and
// DG1 (tv_ensemble_dg.hip) temperature kernels: everything of the ensemble's
// contract towards tv_step and the oracle that does not depend on the
// discretisation.  A kernel is ensemble_bar<Fam, kExt, kModel> and nothing else.
//
// Mapping: one lane per bar, a wave = 64 consecutive bars, one wave per
// workgroup (so a small ensemble spreads over the CUs).  No LDS, no barriers,
// no cross-lane operations: a bar's arithmetic never depends on its
// neighbours in the wave, so a bar computes the same bits alone or in any
// ensemble.  Layout: bar-fastest, [component][dof][bar] (EnsArgs), every
// load / store of a wave one contiguous 512-byte segment.
//
// The family Fam supplies, as static members:
//   n_T(a)                      T dofs per bar;
//   newton_iteration(a, b, bar) assemble F(T) and J(T), solve, T <- T - dx;
//                               returns ||dx||^2;
//   sigma_node(a, i)            the sigma node that T dof i feeds, or -1
//                               (wave-uniform);
//   source_dof(a, node)         the T dof a probe node reads.
//
// Per step and lane (oracle/tv_oracle.py):
//   Newton    newton_solve restated: iteration 1 records ||dx_1||, afterwards
//             converged iff ||dx|| / ||dx_1|| < rtol or ||dx|| < atol
//             (||dx_1|| = 0: the quotient is NaN or inf and atol decides, as
//             in the oracle), at most max_it iterations;
//   visco     t_part of tv_visco_point.h per T dof and s_part at the sigma
//             node that dof feeds, with its state (D = 1, stored s_tilde /
//             sigma_tilde), then T_prev <- T.  kModel selects the model mode
//             of both (kModel 2: s_part's exact relaxation on top of paper
//             mode) and nothing else: in paper mode s_part also reads and
//             rewrites s_partial / sigma_partial (ViscoFields::sp / sgp, state
//             of a paper handle only), and the TState that t_part returns
//             carries the dof's Tf of the previous step to the sigma node, so
//             no Tfo work array exists.
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
// [record][field][probe][bar], one contiguous segment per store of a wave: T
// and Tf at the node's source dof, sigma at the node.  A failed bar stores
// nothing more.  Without either the plain instantiation runs.
#pragma once
#include "tv_internal.h"
#include "tv_visco_point.h"

namespace tv {

struct Bar {
  double a_rad, a_conv, T_amb, T_amb4, dt, dtf;
};

// The bar's Robin coefficients from its (current stage's) htc, T_ambient, epsilon
__device__ __forceinline__ void set_boundary(Bar& b, double sigma_sb, double htc, double Ta, double eps) {
  const double Ta2 = Ta * Ta;
  b.a_rad = 0.001 * (sigma_sb * eps);
  b.a_conv = 0.001 * htc;
  b.T_amb = Ta;
  b.T_amb4 = Ta2 * Ta2;
}

// kExt = false: constant boundary values, final state only; x is not read.
// kExt = true: per-bar stage tables and / or probe records (EnsExt).  A lane
// keeps its own stage and that stage's last step; both follow from the
// absolute step alone, so a launch may start at any step.  Lanes of a wave
// may sit in different stages: that predicates the reload of three values,
// no address pattern changes.
// The structs come by value: by reference the scheduled CG kernel gains a
// private segment.
// kModel is ViscoConst::paper: 0 reference, 1 paper, 2 paper with the exact
// exponential relaxation in s_part (t_part is the paper one).
template <class Fam, bool kExt, int kModel>
__device__ __forceinline__ void ensemble_bar(EnsArgs a, ViscoConst c, ViscoFields f, const EnsExt* __restrict__ x) {
  static_assert(kModel >= 0 && kModel <= 2, "model id: ViscoConst::paper");
  constexpr bool kPaper = kModel != 0;
  const int64_t bar = blockIdx.x * (int64_t)kWave + threadIdx.x;
  if (bar >= a.n_bars) return;          // tail lanes: no memory access
  if (a.failed_step[bar] != 0) return;  // frozen by an earlier failure
  const int nT = Fam::n_T(a);
  Bar b;
  set_boundary(b, a.sigma_sb, a.htc[bar], a.T_amb[bar], a.eps[bar]);
  b.dt = a.dt;
  b.dtf = a.dt * a.f[bar];
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
      const double r = sqrt(Fam::newton_iteration(a, b, bar));
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
      for (int i = 0; i < nT; ++i) {
        const int64_t t = (int64_t)i * a.nb_pad + bar;
        const TState ts = t_part<false, kPaper>(c, f, t);
        const int node = Fam::sigma_node(a, i);
        if (node >= 0) s_part<1, false, false, kPaper, kModel == 2>(c, f, (int64_t)node * a.nb_pad + bar, ts, dirty);
        f.Tp[t] = ts.T;
      }
    }
    if constexpr (kExt) {
      // record step / every - 1 of [record][field][probe][bar], as this step left them (the host refuses
      // steps past max_records * every; the bound here only keeps the stores inside)
      const int step = a.step_base + s + 1;
      if (x->n_probes > 0 && step % x->every == 0 && step / x->every <= x->max_records) {
        const int64_t rec = (int64_t)(step / x->every - 1) * 3 * x->n_probes;
        for (int p = 0; p < x->n_probes; ++p) {
          const int node = x->probes[p];
          const int64_t t = (int64_t)Fam::source_dof(a, node) * a.nb_pad + bar;
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

// The run-time pair of a launch (the handle's model id ViscoConst::paper, whether an EnsExt is given) as
// ensemble_bar's compile-time pair: fn(integral_constant<bool, kExt>, integral_constant<int, kModel>).
template <class Fn>
inline void dispatch_ensemble(int model, bool ext, Fn&& fn) {
  auto with_model = [&](auto m) { ext ? fn(std::true_type{}, m) : fn(std::false_type{}, m); };
  if (model == 2) with_model(std::integral_constant<int, 2>{});
  else if (model) with_model(std::integral_constant<int, 1>{});
  else with_model(std::integral_constant<int, 0>{});
}

}  // namespace tv

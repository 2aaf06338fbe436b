// Fused per-point viscoelastic update (Narayanaswamy shift, partial fictive
// temperatures, strains, scaled time, Prony-series stress increments), gfx950.
//
// Replaces the 17 dolfinx fem::interpolate(Expression) passes of one time step
// (ThermoViscoProblem.py:393-595) over the FFCx expression kernels of
// ViscoelasticModel._init_expressions (ViscoelasticModel.py:86-242), together
// with the _update_values copies (ThermoViscoProblem.py:349-354) and the final
// T_prev <- T update (ThermoViscoProblem.py:378-379).
//
// For degree-1 Lagrange spaces every expression is a per-dof map, so one thread
// owns one dof and carries the whole pipeline in registers: a single HBM pass
// that reads T, T_prev, Tf_partial and writes the state (Tf_partial, Tf, phi,
// xi, sigma) — plus every intermediate Function of the reference when
// materialize = all.  s_tilde / sigma_tilde (Q3: fed only by themselves, so
// +0.0 from the zero initial state on) are read and rewritten only once a
// value other than +0.0 has appeared (ViscoFields::tflag); until then they
// cost no HBM traffic.
//
// Semantics follow the reference, quirks included:
//   Q1 phi is Eq. 5 (the Eq. 25 expression is overwritten, VEM:100 vs :156);
//   Q2 Tf_prev is overwritten before the thermal strain reads it (TVP:481 vs
//      :492), so the alpha_liquid term is (Tf - Tf) = 0;
//   Q3 s_tilde / sigma_tilde are fed by their own previous values (VEM:196,205);
//   Q4 xi = dt/2 (phi_next - phi) with "-" (VEM:171);
//   Q5 xi == 0 gives 0/0 = NaN in ds / dsigma (VEM:178,187).
// The arithmetic is written in the reference's operator order and this file is
// compiled with -ffp-contract=off, so it performs the same IEEE operations as
// the CPU oracle (exp() may differ by an ulp between libm and ocml).
//
// Layout: component-major (SoA) fields, comp * stride + dof, so every load and
// store of a wavefront is one contiguous 512-byte segment.
#include "tv_internal.h"
#include "tv_visco_point.h"

namespace tv {
namespace {

template <int D, bool ALL, bool LEAN, bool PAPER = false, bool EXACT = false>
__device__ __forceinline__ void fused_loop(const ViscoConst& c, const ViscoFields& f) {
  bool dirty = false;
  for (int64_t t = blockIdx.x * (int64_t)kBlock + threadIdx.x; t < f.n; t += (int64_t)gridDim.x * kBlock) {
    const int64_t dT = f.off_T + t;
    const TState ts = t_part<ALL, PAPER>(c, f, dT);
    s_part<D, ALL, LEAN, PAPER, EXACT>(c, f, f.off_S + t, ts, dirty);
    if (f.copy_Tprev) f.Tp[dT] = ts.T;  // TVP:378-379, T_prev is not read after this point
  }
  if (dirty) *f.tflag = 1;
}

template <int D, bool ALL>
__global__ __launch_bounds__(kBlock) void k_visco_fused(ViscoConst c, ViscoFields f) {
  if (!newton_gate_open(f.gate)) return;
  if (c.paper) {
    fused_loop<D, ALL, false, true>(c, f);
    return;
  }
  // read once: a flag raised later in this launch changes nothing (see s_part)
  if (*f.tflag == 0) fused_loop<D, ALL, true>(c, f);
  else fused_loop<D, ALL, false>(c, f);
}

// paper mode with the exact relaxation (ViscoConst::paper == 2, tv_set_relaxation):
// a kernel of its own, chosen on the host, so the kernel above is the same code
// with or without it.  t_part does not see the relaxation.
template <int D, bool ALL>
__global__ __launch_bounds__(kBlock) void k_visco_fused_exact(ViscoConst c, ViscoFields f) {
  if (!newton_gate_open(f.gate)) return;
  fused_loop<D, ALL, false, true, true>(c, f);
}

// mixed families, T pass; in paper mode it also keeps the previous step's Tf
// per T dof (f.Tfo, a work array) for the sigma pass's thermal strain
template <bool ALL>
__global__ __launch_bounds__(kBlock) void k_visco_T(ViscoConst c, ViscoFields f) {
  if (!newton_gate_open(f.gate)) return;
  for (int64_t t = blockIdx.x * (int64_t)kBlock + threadIdx.x; t < f.n; t += (int64_t)gridDim.x * kBlock) {
    if (c.paper) {
      const TState ts = t_part<ALL, true>(c, f, f.off_T + t);
      f.Tfo[f.off_T + t] = ts.Tfo;
    } else {
      (void)t_part<ALL, false>(c, f, f.off_T + t);
    }
  }
}

// mixed families: sigma dof s reads the T-family values of the dof that the
// last cell written by fem::interpolate assigns to it (f.map).
template <int D, bool ALL, bool LEAN, bool PAPER = false, bool EXACT = false>
__device__ __forceinline__ void s_loop(const ViscoConst& c, const ViscoFields& f) {
  bool dirty = false;
  for (int64_t s = blockIdx.x * (int64_t)kBlock + threadIdx.x; s < f.n; s += (int64_t)gridDim.x * kBlock) {
    const int64_t t = f.map[s];
    TState ts;
    ts.T = f.T[t];
    ts.Tp = f.Tp[t];
    ts.Tf = f.Tf[t];
    ts.Tfo = PAPER ? f.Tfo[t] : ts.Tf;
    ts.xi = f.xi[t];
    s_part<D, ALL, LEAN, PAPER, EXACT>(c, f, f.off_S + s, ts, dirty);
  }
  if (dirty) *f.tflag = 1;
}

template <int D, bool ALL>
__global__ __launch_bounds__(kBlock) void k_visco_S(ViscoConst c, ViscoFields f) {
  if (!newton_gate_open(f.gate)) return;
  if (c.paper) s_loop<D, ALL, false, true>(c, f);
  else if (*f.tflag == 0) s_loop<D, ALL, true>(c, f);
  else s_loop<D, ALL, false>(c, f);
}

// the sigma pass with the exact relaxation (see k_visco_fused_exact)
template <int D, bool ALL>
__global__ __launch_bounds__(kBlock) void k_visco_S_exact(ViscoConst c, ViscoFields f) {
  if (!newton_gate_open(f.gate)) return;
  s_loop<D, ALL, false, true, true>(c, f);
}

__global__ __launch_bounds__(kBlock) void k_copy_gated(double* __restrict__ d, const double* __restrict__ s, int64_t n,
                                                       NewtonGate g) {
  if (!newton_gate_open(g)) return;
  for (int64_t t = blockIdx.x * (int64_t)kBlock + threadIdx.x; t < n; t += (int64_t)gridDim.x * kBlock) d[t] = s[t];
}

int blocks_for(int64_t n) {
  int64_t b = (n + kBlock - 1) / kBlock;
  if (b > 8192) b = 8192;
  return b < 1 ? 1 : (int)b;
}

}  // namespace

void launch_visco(int dim, int all, const ViscoConst& c, const ViscoFields& f, hipStream_t s) {
  const int b = blocks_for(f.n);
#define TV_V(D, A)                                                                                   \
  do {                                                                                               \
    if (c.paper == 2) hipLaunchKernelGGL((k_visco_fused_exact<D, A>), dim3(b), dim3(kBlock), 0, s, c, f); \
    else hipLaunchKernelGGL((k_visco_fused<D, A>), dim3(b), dim3(kBlock), 0, s, c, f);               \
  } while (0)
  if (dim == 1) { if (all) TV_V(1, true); else TV_V(1, false); }
  else if (dim == 2) { if (all) TV_V(2, true); else TV_V(2, false); }
  else { if (all) TV_V(3, true); else TV_V(3, false); }
#undef TV_V
}

void launch_copy_gated(double* dst, const double* src, int64_t n, const NewtonGate& g, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_copy_gated, dim3(blocks_for(n)), dim3(kBlock), 0, s, dst, src, n, g);
}

void launch_visco_Tpass(int dim, int all, const ViscoConst& c, const ViscoFields& f, hipStream_t s) {
  (void)dim;
  const int b = blocks_for(f.n);
  if (all) hipLaunchKernelGGL((k_visco_T<true>), dim3(b), dim3(kBlock), 0, s, c, f);
  else hipLaunchKernelGGL((k_visco_T<false>), dim3(b), dim3(kBlock), 0, s, c, f);
}

void launch_visco_Spass(int dim, int all, const ViscoConst& c, const ViscoFields& f, hipStream_t s) {
  const int b = blocks_for(f.n);
#define TV_V(D, A)                                                                               \
  do {                                                                                           \
    if (c.paper == 2) hipLaunchKernelGGL((k_visco_S_exact<D, A>), dim3(b), dim3(kBlock), 0, s, c, f); \
    else hipLaunchKernelGGL((k_visco_S<D, A>), dim3(b), dim3(kBlock), 0, s, c, f);               \
  } while (0)
  if (dim == 1) { if (all) TV_V(1, true); else TV_V(1, false); }
  else if (dim == 2) { if (all) TV_V(2, true); else TV_V(2, false); }
  else { if (all) TV_V(3, true); else TV_V(3, false); }
#undef TV_V
}

}  // namespace tv

// Geometric multigrid on the box hierarchy: setup, per-Newton preparation and
// the multigrid-preconditioned KSPCG (the reference's PCGAMG,
// ThermoViscoProblem.py:343-346, replaced for rectilinear 3D meshes).
//
// Here, shared by every box cycle: the hierarchy plan and transfer tables, the
// level view (mg_view: level 0 is a level), mg_prepare for every configuration,
// the restriction step, the coarse levels' mg_level, level 0's closing step and
// smoother; and the cycle and solve of one partition and of a DG1 slab.
// tv_mgdist.cpp: the slab-partitioned CG1 box's set-up, cycle and solves.
#include <cstdlib>

#include "tv_ctx.h"

namespace tv {
constexpr int64_t kMgFoldFacesNodes = 4000000;  // level 0: facet terms folded into the restriction below this

// ---- geometric-multigrid preconditioned CG (options.preconditioner = GMG) ----
// Gershgorin bound of D^-1 J on a rectilinear level: max over nodes of the
// exact absolute row sum of the 27-point cell operator M + dt alpha K over its
// diagonal (the tensor-product entries from the per-axis 1D rows), over the
// distinct (row_x, row_y, row_z) combinations only.  The Robin facet rows are
// facet masses (row sum / diagonal <= 2.25 for Q1 facets): floor 2.25, then 5 %.
double mg_gershgorin(const std::vector<double> (&X)[3], double dt_alpha) {
  using Row = std::array<double, 6>;  // M lo / di / up, K lo / di / up
  std::vector<Row> rows[3];
  for (int s = 0; s < 3; ++s) {
    std::vector<double> cf;
    axis_coefs(X[s], 0, (int)X[s].size(), cf);
    for (size_t i = 0; i < X[s].size(); ++i) {
      const double* c = &cf[i * C_NCOEF];
      rows[s].push_back({c[C_MLO], c[C_MDI], c[C_MUP], c[C_KLO], c[C_KDI], c[C_KUP]});
    }
    std::sort(rows[s].begin(), rows[s].end());
    rows[s].erase(std::unique(rows[s].begin(), rows[s].end()), rows[s].end());
  }
  double b = 0.0;
  for (const Row& r0 : rows[0])
    for (const Row& r1 : rows[1])
      for (const Row& r2 : rows[2]) {
        double sum = 0.0, diag = 0.0;
        for (int a = 0; a < 3; ++a)
          for (int bb = 0; bb < 3; ++bb)
            for (int cc = 0; cc < 3; ++cc) {
              const double v = r0[a] * r1[bb] * r2[cc] +
                               dt_alpha * (r0[3 + a] * r1[bb] * r2[cc] + r0[a] * r1[3 + bb] * r2[cc] +
                                           r0[a] * r1[bb] * r2[3 + cc]);
              sum += std::fabs(v);
              if (a == 1 && bb == 1 && cc == 1) diag = v;
            }
        b = std::max(b, sum / diag);
      }
  return std::max(b, 2.25) * 1.05;
}

double mg_omega(double b) { return 2.0 / (1.1 * b); }

// the CG1 level of the box given by X (single partition), its vectors and weight
int mg_add_cg_level(Ctx* c, const std::vector<double> (&X)[3], double da) {
  c->mg.emplace_back();
  MgLevel& L = c->mg.back();
  for (int s = 0; s < 3; ++s) L.X[s] = X[s];
  if (int e = build_cg_grid(c, 3, L.X, 0, (int)L.X[2].size(), 0, 0, true, true, L.g, L.coef, &L.bnodes, L.ffbuf))
    return e;
  if (int e = mg_level_vectors(c, L)) return e;
  L.omega = mg_omega(mg_gershgorin(L.X, da));
  return TV_OK;
}

// ---- level 0's smoother B (Smoother0): what each kind launches, here only ----
void level0_setup(Ctx* c, const double* T, bool dinv_fresh) {
  switch (c->smoother0) {
    case Smoother0::DG_BLOCK: return;  // the facet means of dg(T) are launched by mg_prepare, with level 1's T
    case Smoother0::AUX_BLOCK: aux_refresh(c, T); return;  // the blocks of the cells with an exterior facet follow T
    case Smoother0::POINT: break;
  }
  if (!c->um && c->fam_T == TV_CG) {
    // the box march path: the T-independent interior of dinv is written once; then the boundary nodes only
    if (!dinv_fresh) launch_cg_diag(c->cg, T, c->dinv, 1, c->stream, c->dinv_interior);
    c->dinv_interior = true;
  } else {
    op_diag(c, T, c->dinv, 1);
  }
}

void level0_smooth(Ctx* c, const PcgState* st, const double* b, double omega, double* x, int64_t off, int64_t n) {
  switch (c->smoother0) {
    case Smoother0::POINT:
      launch_mg_jacobi(n, st, b + off, nullptr, nullptr, c->dinv + off, omega, x + off, 0, c->stream);
      return;
    case Smoother0::DG_BLOCK: launch_dg_bsmooth(c->dg, st, b, nullptr, c->dggface, omega, x, 0, c->stream); return;
    case Smoother0::AUX_BLOCK: aux_smooth(c, st, b, omega, x); return;
  }
}

void level0_update(Ctx* c, int it, bool init, int64_t off, int64_t n, const double* lag, unsigned* counter) {
  double* dx = c->f[TV_F_DX].ptr;
  switch (c->smoother0) {
    case Smoother0::POINT: {
      // w lacks the facet terms of the faces along the march on a CG box only (DG, unstructured: complete)
      const FaceAdd fa = (!init && !c->um && c->fam_T == TV_CG) ? cg_face_add(c->cg, off) : FaceAdd{};
      launch_mg_update(n, c->st, c->pA + off, c->pB + off, c->w + off, init ? nullptr : &fa, c->dinv + off,
                       c->mg_omega0, c->r + off, dx + off, c->mgx + off, it, init, c->stream, lag, counter);
      return;
    }
    case Smoother0::DG_BLOCK:  // the owned cells (no lagged logic on DG)
      launch_dg_bupdate(c->dg, c->st, c->pA, c->pB, c->w, c->dggface, c->mg_omega0, c->r, dx, c->mgx, it, init,
                        c->stream);
      return;
    case Smoother0::AUX_BLOCK:
      launch_umdg_aux_update(c->udg, c->aux, c->st, c->pA, c->pB, c->w, c->mg_omega0, c->r, dx, c->mgx, it, init,
                             c->stream);
      return;
  }
}

// lambda_max(B^-1 J) of level 0 by power iteration, B its smoother at T (SIPG
// rows and general meshes have no closed-form Gershgorin bound here)
static int level0_lambda(Ctx* c, const double* T, double* lam) {
  // a partition of a distributed unstructured mesh (collective): its owned rows,
  // the start vector's entries at their partition-major global indices, the
  // ghosts refreshed before every product, the norms all-reduced
  const bool part = c->n_parts > 1;
  const int64_t n = part ? c->ownT_n : c->nT;
  std::vector<double> h((size_t)n);
  uint64_t st = 0x9E3779B97F4A7C15ull;
  double nrm = 0.0;
  const int64_t skip = part ? c->globT_off : 0;
  for (int64_t t = 0; t < skip + n; ++t) {  // fixed-seed xorshift start vector in (0.5, 1.5)
    st ^= st << 13; st ^= st >> 7; st ^= st << 17;
    if (t < skip) continue;
    h[(size_t)(t - skip)] = 0.5 + (double)(st >> 11) * (1.0 / 9007199254740992.0);
    nrm += h[(size_t)(t - skip)] * h[(size_t)(t - skip)];
  }
  auto gsum = [&](double& v) -> int {  // sum over the ranks (partitioned)
    if (!part) return TV_OK;
    HIPC(hipMemcpyAsync(c->sums + 4, &v, sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (int e = allreduce(c, c->sums + 4, 1)) return e;
    HIPC(hipMemcpyAsync(&v, c->sums + 4, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    return TV_OK;
  };
  if (int e = gsum(nrm)) return e;
  for (double& v : h) v /= std::sqrt(nrm);
  HIPC(hipMemcpyAsync(c->mgx, h.data(), sizeof(double) * (size_t)n, hipMemcpyHostToDevice, c->stream));
  const bool block = c->smoother0 != Smoother0::POINT;
  if (c->smoother0 == Smoother0::DG_BLOCK) launch_dg_gface(c->dg, T, c->dggface, c->stream);  // as mg_prepare does
  std::vector<double> prt(1024);
  double l = 0.0;
  level0_setup(c, T);
  for (int it = 0; it < 30; ++it) {
    if (part)
      if (int e = halo(c, c->mgx)) return e;
    op_japply(c, T, c->mgx, c->w, nullptr, nullptr);
    if (block) level0_smooth(c, nullptr, c->w, 1.0, c->w, 0, n);  // B^-1 in place, per cell; POINT: dinv below
    const int nb = launch_mg_pow(n, block ? nullptr : c->dinv, c->w, c->partials, c->stream);
    HIPC(hipMemcpyAsync(prt.data(), c->partials, sizeof(double) * (size_t)nb, hipMemcpyDeviceToHost, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    double s2 = 0.0;
    for (int b = 0; b < nb; ++b) s2 += prt[(size_t)b];
    if (int e = gsum(s2)) return e;
    l = std::sqrt(s2);  // ||D^-1 J x|| with ||x|| = 1
    if (!(l > 0.0) || !std::isfinite(l)) return c->fail(TV_ERR_HIP, "GMG: DG eigenvalue estimate failed");
    launch_mg_scale(n, c->w, 1.0 / l, c->mgx, c->stream);
  }
  *lam = l;
  return TV_OK;
}

// Level 0's smoother weight where no bound is known in advance (the DG1 cell
// blocks, the algebraic hierarchies): estimated lazily, at the first multigrid
// solve (or V-cycle application), from the temperature it will precondition
// -- the Robin term 4 a_rad T^3 vanishes at the T = 0 a freshly created context
// holds.  omega0 = 2 / (1.21 lambda_max) before the multiplicative box cycle,
// the coarse levels' 2 / (1.1 lambda_max) for the additive level 0 of AMG
int level0_weight(Ctx* c, const double* T) {
  if (!(c->smoother0 == Smoother0::DG_BLOCK || c->amg_on) || c->mg_omega0 > 0.0) return TV_OK;
  double lam = 0.0;
  if (int e = level0_lambda(c, T, &lam)) return e;
  c->mg_omega0 = c->amg_on ? 2.0 / (1.1 * lam) : 2.0 / (1.1 * 1.1 * lam);
  return TV_OK;
}

// Coarsening rule of the box hierarchy (identical for a whole box and for its
// partitions, which plan it over the global grid): every other node kept
// along each axis with at least two cells, plus the last node when the cell
// count is odd (coarse nodes are a subset of the fine ones); stop where the
// operator is mass-dominated (dt alpha / h^2 <= 0.5 with h the smallest mean
// cell length: a Jacobi step is then a good solve) or nothing coarsens.
static bool mg_next_level(const std::vector<double> (&Xp)[3], double da, bool automatic,
                          std::vector<double> (&Xc)[3], std::vector<char> (&is_c)[3], int coarse[3]) {
  double h = 1e300;
  bool any = false;
  for (int s = 0; s < 3; ++s) {
    const int cells = (int)Xp[s].size() - 1;
    coarse[s] = cells >= 2;
    any = any || coarse[s];
    if (cells >= 1) h = std::min(h, (Xp[s].back() - Xp[s].front()) / cells);
  }
  if (!any || (automatic && da / (h * h) <= 0.5)) return false;
  for (int s = 0; s < 3; ++s) {
    const int nf = (int)Xp[s].size();
    Xc[s].clear();
    is_c[s].assign(nf, 1);
    if (!coarse[s]) {
      Xc[s] = Xp[s];
      continue;
    }
    for (int i = 0; i < nf; ++i) is_c[s][i] = (i % 2 == 0 || i == nf - 1) ? 1 : 0;
    for (int i = 0; i < nf; ++i)
      if (is_c[s][i]) Xc[s].push_back(Xp[s][i]);
  }
  return true;
}

std::vector<MgPlanLevel> mg_plan(const Ctx* c, const std::vector<double> (&Xf)[3], double da, int have) {
  const int max_levels = c->O.mg_levels > 0 ? c->O.mg_levels : 8;
  const bool automatic = c->O.mg_levels <= 0;
  std::vector<MgPlanLevel> plan(1);
  for (int s = 0; s < 3; ++s) plan[0].X[s] = Xf[s];
  for (int lev = have; lev < max_levels; ++lev) {
    MgPlanLevel nl;
    if (!mg_next_level(plan.back().X, da, automatic, nl.X, nl.is_c, nl.coarse)) break;
    plan.push_back(std::move(nl));
  }
  return plan;
}

// Transfer tables of one axis over the whole (global) axis: prolongation = two
// (coarse index, weight) pairs per fine node (exact linear interpolation),
// restriction R = P^T = three (fine index, weight) pairs per coarse node
void mg_axis_tables(const std::vector<double>& Xf, const std::vector<char>& is_c, std::vector<int>& pi,
                    std::vector<double>& pw, std::vector<int>& ri, std::vector<double>& rw) {
  const int nf = (int)Xf.size();
  std::vector<int> cpos(nf, -1), fpos;
  for (int i = 0; i < nf; ++i)
    if (is_c[i]) {
      cpos[i] = (int)fpos.size();
      fpos.push_back(i);
    }
  const int nc = (int)fpos.size();
  pi.assign(2 * (size_t)nf, 0);
  pw.assign(2 * (size_t)nf, 0.0);
  ri.assign(3 * (size_t)nc, 0);
  rw.assign(3 * (size_t)nc, 0.0);
  for (int i = 0; i < nf; ++i) {
    if (is_c[i]) {
      pi[2 * i] = pi[2 * i + 1] = cpos[i];
      pw[2 * i] = 1.0;
    } else {  // linear interpolation between the coarse neighbours i - 1 and i + 1
      const double wl = (Xf[i + 1] - Xf[i]) / (Xf[i + 1] - Xf[i - 1]);
      pi[2 * i] = cpos[i - 1];
      pi[2 * i + 1] = cpos[i + 1];
      pw[2 * i] = wl;
      pw[2 * i + 1] = 1.0 - wl;
    }
  }
  for (int I = 0; I < nc; ++I) {  // R = P^T: the fine nodes that interpolate from I
    const int fc = fpos[I];
    for (int q = 0; q < 3; ++q) ri[3 * I + q] = fc;
    rw[3 * I + 1] = 1.0;
    if (fc - 1 >= 0 && !is_c[fc - 1]) {
      ri[3 * I] = fc - 1;
      rw[3 * I] = pw[2 * (fc - 1) + 1];  // fine fc - 1: its right coarse neighbour is I
    }
    if (fc + 1 < nf && !is_c[fc + 1]) {
      ri[3 * I + 2] = fc + 1;
      rw[3 * I + 2] = pw[2 * (fc + 1)];  // fine fc + 1: its left coarse neighbour is I
    }
  }
}

int mg_upload_axis(Ctx* c, MgLevel& L, int s, const std::vector<int>& pi, const std::vector<double>& pw,
                   const std::vector<int>& ri, const std::vector<double>& rw, int nf, int nc, int coarse) {
  MgXfer& x = L.xf;
  if (int e = mg_upload(c, L, pi, &x.pi[s])) return e;
  if (int e = mg_upload(c, L, pw, &x.pw[s])) return e;
  if (int e = mg_upload(c, L, ri, &x.ri[s])) return e;
  if (int e = mg_upload(c, L, rw, &x.rw[s])) return e;
  x.fn[s] = nf;
  x.cn[s] = nc;
  x.coarse[s] = coarse;
  return TV_OK;
}

// Tables of the fused residual restriction (RRArgs) along one axis: for coarse
// node I (fine node fc = ri[3I + 1]) the window fc - 2 .. fc + 2 and the weights
// of (R M), (R K) and R over it, from the fine 1D rows and the restriction
// weights.  False when a product reaches outside the window (not a nested pair).
static bool rr_axis(const std::vector<double>& Xf, const std::vector<int>& ri, const std::vector<double>& rw,
                    std::vector<int>& f0, std::vector<double>& w) {
  const int nf = (int)Xf.size(), nc = (int)ri.size() / 3;
  std::vector<double> cf;
  axis_coefs(Xf, 0, nf, cf);
  f0.assign(nc, 0);
  w.assign(15 * (size_t)nc, 0.0);
  for (int I = 0; I < nc; ++I) {
    f0[I] = ri[3 * I + 1] - 2;
    for (int q = 0; q < 3; ++q) {
      const int f = ri[3 * I + q];
      const double wt = rw[3 * I + q];
      if (wt == 0.0) continue;
      const double* cc = &cf[(size_t)f * C_NCOEF];
      auto add = [&](int col, int fi, double v) -> bool {
        if (v == 0.0) return true;
        const int m = fi - f0[I];
        if (fi < 0 || fi >= nf || m < 0 || m > 4) return false;
        w[15 * (size_t)I + 5 * col + m] += wt * v;
        return true;
      };
      if (!(add(0, f - 1, cc[C_MLO]) && add(0, f, cc[C_MDI]) && add(0, f + 1, cc[C_MUP]) &&
            add(1, f - 1, cc[C_KLO]) && add(1, f, cc[C_KDI]) && add(1, f + 1, cc[C_KUP]) && add(2, f, 1.0)))
        return false;
    }
  }
  return true;
}

// The fused residual restriction from fine coordinates Xp into coarse level L
// (single partition): x needs even fine cell counts (lanes own fine pairs
// 2I, 2I + 1), the march axis consecutive windows two fine planes apart (every
// coarsened axis: the odd tail's window too); the row axis is free.
static int rr_setup(Ctx* c, MgLevel& L, const std::vector<double> (&Xp)[3], const std::vector<int> (&ri)[3],
                    const std::vector<double> (&rw)[3]) {
  RRArgs& a = L.rr;
  a = RRArgs{};
  const MgXfer& x = L.xf;
  if (!x.coarse[0] || x.fn[0] < 5 || !(x.fn[0] & 1)) return TV_OK;
  std::vector<int> f0[3];
  std::vector<double> w[3];
  for (int s = 0; s < 3; ++s)
    if (!rr_axis(Xp[s], ri[s], rw[s], f0[s], w[s])) return TV_OK;
  auto regular = [&](int s) {
    if (!x.coarse[s] || x.cn[s] < 2) return false;
    for (int I = 0; I + 1 < x.cn[s]; ++I)
      if (f0[s][I + 1] - f0[s][I] != 2) return false;
    return true;
  };
  int qa = (x.cn[1] <= x.cn[2]) ? 1 : 2;
  if (!regular(qa)) qa = 3 - qa;
  if (!regular(qa)) return TV_OK;
  a.raxis = 3 - qa;
  for (int I = 0; I + 1 < x.cn[a.raxis]; ++I)  // the row axis: windows 1 or 2 fine rows apart (slab bound)
    if (f0[a.raxis][I + 1] - f0[a.raxis][I] > 2) return TV_OK;
  for (int s = 0; s < 3; ++s) {
    a.fn[s] = x.fn[s];
    a.cn[s] = x.cn[s];
    if (int e = mg_upload(c, L, f0[s], &a.ax[s].f0)) return e;
    if (int e = mg_upload(c, L, w[s], &a.ax[s].w)) return e;
  }
  a.da = L.g.dt_alpha;
  a.nseg = (x.cn[0] + 61) / 62;
  // chunks of the march axis: about `target` workgroups of 8 waves (2 fit a CU:
  // 67 KB of LDS each), >= 3 coarse planes per chunk (TVFEM_RR_WG overrides)
  // (256 measured best at C4: V-cycle 226 us against 240 / 231 us at 128 / 512)
  const char* te = std::getenv("TVFEM_RR_WG");
  const int target = te ? std::max(1, std::atoi(te)) : 256;
  const int64_t rowblocks = (x.cn[a.raxis] + 7) / 8;
  a.qchunk = std::min(x.cn[qa], kRRQMaxChunk);
  while ((int64_t)a.nseg * rowblocks * ((x.cn[qa] + a.qchunk - 1) / a.qchunk) < target && a.qchunk > 3)
    a.qchunk = (a.qchunk + 1) / 2;
  // the launcher refuses any other chunk (the kernel's weight stage holds kRRQMaxChunk planes)
  if (a.qchunk < 1 || a.qchunk > kRRQMaxChunk)
    return c->fail(TV_ERR_STATE, "GMG: fused residual restriction: march chunk " + std::to_string(a.qchunk) +
                                     " outside [1, " + std::to_string(kRRQMaxChunk) + "]");
  a.on = 1;
  return TV_OK;
}

// Levels whose restriction runs fused (bit l: from level l into level l + 1):
// level 0 on fine grids of >= kRRMinNodes nodes.  Measured (C4, 8.2M nodes,
// interleaved): V-cycle 249 -> 226 us, step 10.22 -> 9.85 ms; at C3 (1M nodes)
// 3.15 -> 3.21 ms and on the coarse levels slower (their J x launches are
// latency-bound, the facet launch adds one), so not there.  TVFEM_MG_RR (a bit
// mask, read at setup) overrides, for tests and A/B measurement.
constexpr int64_t kRRMinNodes = 3000000;
static unsigned rr_levels(int64_t fine_nodes) {
  const char* e = std::getenv("TVFEM_MG_RR");
  if (e) return (unsigned)std::strtoul(e, nullptr, 0);
  return fine_nodes >= kRRMinNodes ? 1u : 0u;
}

int mg_zeroed(Ctx* c, int64_t n, double** out) {
  const size_t bytes = sizeof(double) * (size_t)std::max<int64_t>(1, n);
  HIPC(tv_dev_alloc(out, bytes, kMemDoubles));
  HIPC(hipMemsetAsync(*out, 0, bytes, c->stream));
  return TV_OK;
}

// T, b, x, w, dinv of a level (local size L.n), zeroed
int mg_level_vectors(Ctx* c, MgLevel& L) {
  const CgGrid& f = c->cg;  // thermal constants (set by setup_mesh for both families)
  L.g.dt = f.dt; L.g.dt_alpha = f.dt_alpha; L.g.dt_f = f.dt_f;
  L.g.a_rad = f.a_rad; L.g.a_conv = f.a_conv; L.g.T_amb = f.T_amb; L.g.T_amb4 = f.T_amb4;
  L.n = (int64_t)L.g.n0 * L.g.n1 * L.g.n2;
  for (double** q : {&L.T, &L.b, &L.x, &L.w, &L.dinv}) {
    if (int e = mg_zeroed(c, L.n, q)) return e;
    L.bufs.push_back(*q);
  }
  return TV_OK;
}

int mg_setup(Ctx* c) {
  const bool dg = c->fam_T == TV_DG;
  if (c->dim != 3 || c->um || (!dg && !cg_cgs_supported(c->cg)) || (dg && (c->dg.deg1 || c->dg.deg2)))
    return c->fail(TV_ERR_ARG, "preconditioner GMG: 3D CG1 or DG1 temperature space on a rectilinear mesh only");
  if (c->cgs) return c->fail(TV_ERR_ARG, "preconditioner GMG runs in the KSPCG form (pcg_variant KSPCG or AUTO)");
  if (c->n_parts > 1 && !dg) return mg_setup_dist(c);  // slab-partitioned CG1 box (tv_mgdist.cpp)
  // a DG1 box, one partition or slab-partitioned: level 1 is the CG1 space of
  // the WHOLE box (the global coordinates), and it and every coarser level are
  // replicated on every slab (mg_A = 1): a slab restricts its owned cells into
  // the vertex planes they touch, one all-reduce of the level-1 vector sums the
  // shared planes, every slab runs the CG cycle below and prolongs into all its
  // local cells (ghost layers included: the level holds every vertex)
  if (c->n_parts > 1) c->mg_A = 1;
  std::vector<double> tmp, Xf[3];
  for (int s = 0; s < 3; ++s) Xf[s] = storage_coords(c, s, tmp);
  const double da = c->P.dt * c->P.alpha;
  if (int e = mg_zeroed(c, c->nT, &c->mgx)) return e;
  if (dg) {
    // level 1: the CG1 space of the same box (two-level DG -> CG, then the CG hierarchy)
    c->smoother0 = Smoother0::DG_BLOCK;
    HIPC(tv_dev_alloc(&c->dggface, sizeof(double) * (size_t)dg_gface_size(c->dg), kMemDoubles));
    c->mg_omega0 = 0.0;  // estimated at the first solve, at its T (level0_weight)
    if (int e = mg_add_cg_level(c, Xf, da)) return e;
  } else {
    c->mg_omega0 = mg_omega(mg_gershgorin(Xf, da));
  }
  const std::vector<MgPlanLevel> plan = mg_plan(c, Xf, da, dg ? 2 : 1);
  for (size_t l = 1; l < plan.size(); ++l) {
    const std::vector<double>(&Xp)[3] = plan[l - 1].X;
    if (int e = mg_add_cg_level(c, plan[l].X, da)) return e;
    MgLevel& L = c->mg.back();
    // transfer maps (finer level Xp -> this level)
    MgXfer& x = L.xf;
    std::vector<int> ri[3];
    std::vector<double> rw[3];
    for (int s = 0; s < 3; ++s) {
      std::vector<int> pi;
      std::vector<double> pw;
      mg_axis_tables(Xp[s], plan[l].is_c[s], pi, pw, ri[s], rw[s]);
      if (int e = mg_upload_axis(c, L, s, pi, pw, ri[s], rw[s], (int)Xp[s].size(), (int)L.X[s].size(),
                                 plan[l].coarse[s]))
        return e;
    }
    x.f_kb = 0;
    x.f_ke = x.fn[2];
    x.c_kb = 0;
    x.c_ke = x.cn[2];
    x.aligned = 1;
    // the fused residual restriction into this level (CG levels of a CG box;
    // the DG1 -> CG1 transfer is the cell-vertex one)
    const size_t from = c->mg.size() - 1 - (dg ? 1 : 0);  // index of the finer level (0: the fine grid)
    if (!dg && ((rr_levels(c->nT) >> from) & 1u))
      if (int e = rr_setup(c, L, Xp, ri, rw)) return e;
  }
  c->mg_on = true;
  return TV_OK;
}

// Level 1 of a DG1 box at T: the vertex mean of the cell-local values (a slab:
// on its owned vertex planes, summed over the slabs -- each plane from one
// slab), and the facet means of level 0's cell blocks
static int mg_dg_level1_T(Ctx* c, const double* T, MgLevel& L) {
  const bool slab = c->n_parts > 1;
  if (slab) HIPC(hipMemsetAsync(L.T, 0, sizeof(double) * (size_t)L.n, c->stream));
  launch_mg_dg_T(c->dg, T, L.T, c->plane_begin - c->dg.k_begin, c->stream);  // 0 on one partition
  if (slab)
    if (int e = allreduce_vec(c, L.T, L.n)) return e;
  launch_dg_gface(c->dg, T, c->dggface, c->stream);
  return TV_OK;
}

// T onto every level from the one above, one level at a time, and the level's
// Jacobi diagonal.  How T reaches a level: a DG1 box's level 1 as above; a
// distributed level of a CG1 slab (tv_mgdist.cpp) injected on the owned planes,
// then the ghost planes exchanged; its first replicated level: each rank
// injects its own planes into a zeroed vector, summed over the ranks; every
// other level injected locally
static int mg_inject_levels(Ctx* c, const double* T) {
  const bool dg = c->smoother0 == Smoother0::DG_BLOCK;
  const double* Tf = T;
  for (size_t l = 0; l < c->mg.size(); ++l) {
    MgLevel& L = c->mg[l];
    if (l == 0 && dg) {
      if (int e = mg_dg_level1_T(c, T, L)) return e;
    } else if (L.dist) {
      launch_mg_inject_range(L.xf, Tf, L.T, L.inj0, L.inj1, c->stream);
      if (int e = halo_grid(c, L.g, L.T)) return e;
    } else if (c->n_parts > 1 && !dg && (int)l + 1 == c->mg_A) {
      HIPC(hipMemsetAsync(L.T, 0, sizeof(double) * (size_t)L.n, c->stream));
      launch_mg_inject_range(L.xf, Tf, L.T, L.inj0, L.inj1, c->stream);
      if (int e = allreduce_vec(c, L.T, L.n)) return e;
    } else {
      launch_mg_inject(L.xf, Tf, L.T, c->stream);
    }
    launch_cg_diag(L.g, L.T, L.dinv, 1, c->stream, L.dinv_interior);
    L.dinv_interior = true;
    Tf = L.T;
  }
  HIPC(hipGetLastError());
  return TV_OK;
}

// per Newton iteration: T down the hierarchy and the coarse Jacobi diagonals
int mg_prepare(Ctx* c, const double* T) {
  if (c->amg_on) return TV_OK;  // the algebraic hierarchy is T-independent (tv_amg.cpp)
  const bool dg = c->smoother0 == Smoother0::DG_BLOCK;
  // every level a whole box (one partition, and a DG1 slab's replicated levels),
  // after the first call (dinv interiors in place): the CG levels below the
  // base in two launches (launch_mg_prepare)
  const size_t base = dg ? 1 : 0;  // DG: level 1 is the vertex mean of the DG field
  const size_t ncg = c->mg.size() - std::min(c->mg.size(), base);
  bool ready = (c->n_parts == 1 || dg) && ncg > 0 && ncg <= (size_t)kMgPrepMax;
  for (size_t l = base; l < c->mg.size() && ready; ++l)
    ready = c->mg[l].dinv_interior && cg_uses_march(c->mg[l].g) && c->mg[l].g.bnodes != nullptr;
  if (!ready) return mg_inject_levels(c, T);
  if (base == 1) {
    MgLevel& L = c->mg[0];
    if (int e = mg_dg_level1_T(c, T, L)) return e;
    launch_cg_diag(L.g, L.T, L.dinv, 1, c->stream, true);
  }
  MgPrep p{};
  p.nlev = (int)ncg;
  p.Tbase = base == 1 ? c->mg[0].T : T;
  for (size_t i = 0; i < ncg; ++i) {
    MgLevel& L = c->mg[base + i];
    p.xf[i] = L.xf;
    p.T[i] = L.T;
    p.dinv[i] = L.dinv;
    p.g[i] = L.g;
    p.off_n[i + 1] = p.off_n[i] + (L.n + 63) / 64 * 64;
    p.off_b[i + 1] = p.off_b[i] + (L.g.n_bnodes + 63) / 64 * 64;
  }
  launch_mg_prepare(p, c->stream);
  return TV_OK;
}

// The prolongation from coarse level index ci (c->mg[ci]) into its finer level:
// where that level has a post-smoothing step (not the coarsest) and the
// 2 x 2 block prolongation runs, the step is applied on the fly (CoarsePost)
// and mg_level skipped its k_mg_jacobi launch.
void mg_prolong_from(Ctx* c, size_t ci, double* xf, const double* mask) {
  MgLevel& C = c->mg[ci];
  const bool smoothed = ci + 1 < c->mg.size() && mg_prolong_smooths(C.xf);
  if (smoothed) {
    const CoarsePost cp{C.b, C.w, C.dinv, C.omega, cg_face_add(C.g, 0)};
    launch_mg_prolong(C.xf, c->st, xf, C.x, mask, c->stream, &cp);
  } else {
    launch_mg_prolong(C.xf, c->st, xf, C.x, mask, c->stream);
  }
}

MgView mg_view(Ctx* c, size_t l, const double* T0) {
  const MgLevel* L = l ? &c->mg[l - 1] : nullptr;
  MgView r = L ? MgView{&L->g, L->T, L->b, L->x, L->w, L->dinv, L->omega}
               : MgView{&c->cg, T0, c->r, c->mgx, c->w, c->dinv, c->mg_omega0};
  const int64_t plane = (int64_t)r.g->n0 * r.g->n1;
  r.off = plane * r.g->k_begin;
  r.n_own = plane * (r.g->k_end - r.g->k_begin);
  r.woff = plane * r.g->w_begin;
  r.n_win = plane * (r.g->w_end - r.g->w_begin);
  return r;
}

// The residual of fine level f (a whole box: one partition, or a replicated
// level) restricted into the next coarser level C, with C's pre-smoothing step
// from 0 (x = omega D^-1 b): b_C = R (b - J x), three ways.  mask: the transfer
// mask (level 0 under Dirichlet: the free subspace; else null).  fold_faces: the
// restriction may add the face-workgroup facet terms itself (no k_cg_addfaces;
// a per-node facet term inside the 27-point gather measured slower) -- one
// launch fewer where the V-cycle is launch-bound; level 0 allows it below
// kMgFoldFacesNodes (at C4 a complete J x measured the same).
static int mg_restrict_into(Ctx* c, const MgView& f, MgLevel& C, const double* mask, bool fold_faces) {
  hipStream_t s = c->stream;
  const FaceAdd fa = cg_face_add(*f.g, 0);
  if (C.rr.on && mask == nullptr && fa.on) {
    // without J x: the facet terms of x on every face, then the fused residual
    // restriction (RRArgs)
    launch_cg_facet_faces(*f.g, f.T, f.x, c->st, s);
    if (!launch_mg_rrestrict(C.rr, c->st, f.b, f.x, cg_face_add_all(*f.g), C.b, C.dinv, C.omega, C.x, s))
      return c->fail(TV_ERR_STATE, "GMG: fused residual restriction refused (march chunk out of range)");
  } else if (fa.on && mg_restrict_folds_faces(C.xf) && fold_faces) {
    launch_cg_japply_partial(*f.g, f.T, f.x, f.w, c->st, s);
    launch_mg_restrict(C.xf, c->st, f.b, f.w, &fa, mask, C.b, C.dinv, C.omega, C.x, s);
  } else {  // the complete J x (k_cg_addfaces)
    launch_cg_japply(*f.g, f.T, f.x, f.w, nullptr, nullptr, s, c->st);
    launch_mg_restrict(C.xf, c->st, f.b, f.w, nullptr, mask, C.b, C.dinv, C.omega, C.x, s);
  }
  return TV_OK;
}

// V-cycle on coarse level l >= 1 (index l - 1 in c->mg): rhs b -> x; the
// pre-smoothing step from 0 (x = omega D^-1 b) was formed by the restriction
// that produced b.  The J x before the post-smoothing leaves the facet terms
// of the faces along the march to that pointwise consumer (FaceAdd).
int mg_level(Ctx* c, size_t l) {
  MgLevel& L = c->mg[l - 1];
  hipStream_t s = c->stream;
  if (l < c->mg.size()) {
    if (int e = mg_restrict_into(c, mg_view(c, l, nullptr), c->mg[l], nullptr, true)) return e;
    if (int e = mg_level(c, l + 1)) return e;
    mg_prolong_from(c, l, L.x, nullptr);
    launch_cg_japply_partial(L.g, L.T, L.x, L.w, c->st, s);
    // post-smoothing, unless the prolongation out of this level applies it (mg_prolong_from)
    if (!mg_prolong_smooths(L.xf)) {
      const FaceAdd fa = cg_face_add(L.g, 0);
      launch_mg_jacobi(L.n, c->st, L.b, L.w, &fa, L.dinv, L.omega, L.x, 1, s);
    }
  }
  return TV_OK;
}

void mg_close0_unfused(Ctx* c, const MgView& v, const RedTail* tail) {
  hipStream_t s = c->stream;
  launch_cg_japply_partial(*v.g, v.T, v.x, v.w, c->st, s);
  const FaceAdd fa = cg_face_add(*v.g, v.off);
  launch_mg_post(v.n_own, c->st, v.x + v.off, v.b + v.off, v.w + v.off, &fa, v.dinv + v.off, v.omega, c->z + v.off,
                 c->partials, tail, s);
}

void mg_close0(Ctx* c, const MgView& v, const RedTail* tail) {
  // J x, post-smoothing and (z.z, z.r) in the march epilogue (+ the side-face
  // pass with the reduction tail), on one partition and on a slab alike
  if (launch_cg_japply_post(*v.g, v.T, v.x, v.b, v.dinv, v.omega, c->z, c->st, c->partials, tail, c->stream) >= 0)
    return;
  mg_close0_unfused(c, v, tail);
}

// Dirichlet mode constrains a CG1 temperature only (a DG1 dof belongs to no
// facet: tv_set_dirichlet).  The masks of the cycle's transfers are dinv with
// its constrained rows zeroed (launch_bc_mask), which nothing writes on a DG1
// context: there dinv stays all zero, and a cycle masked with it would keep
// only its block smoothing (z = omega0 B^-1 r)
static bool dirichlet_masks(const Ctx* c) { return c->dir_on && c->fam_T == TV_CG; }

// the box cycle of one partition (and of a DG1 slab): x0 = omega0 B^-1 r is in
// c->mgx (level0_update); coarse correction, post-smoothing into z with the
// (z.z, z.r) reduction tail
static int mg_cycle_box(Ctx* c, const double* T, const RedTail* tail) {
  hipStream_t s = c->stream;
  const double* mask = dirichlet_masks(c) ? c->dinv : nullptr;  // Dirichlet: the free subspace
  // DG1 level 0: complete DG J x (Robin facets inline), vertex sums / injection to CG1
  if (c->smoother0 == Smoother0::DG_BLOCK) {
    const DgGrid& d = c->dg;
    MgLevel& C = c->mg[0];
    const bool slab = c->n_parts > 1;  // the replicated level 1 (mg_setup), see there
    const int kg0 = c->plane_begin - d.k_begin;  // 0 on one partition
    if (slab)
      if (int e = halo(c, c->mgx)) return e;  // x0 of the ghost layers (J x0, the prolongation into them)
    launch_dg_japply(d, T, c->mgx, c->w, nullptr, nullptr, s, c->st);
    if (slab) {  // the slabs' partial restrictions summed, then level 1's pre-smoothing from 0
      HIPC(hipMemsetAsync(C.b, 0, sizeof(double) * (size_t)C.n, s));
      launch_mg_dg_restrict(d, c->st, c->r, c->w, mask, C.b, nullptr, 0.0, nullptr, kg0, s);
      if (int e = allreduce_vec(c, C.b, C.n)) return e;
      launch_mg_jacobi(C.n, c->st, C.b, nullptr, nullptr, C.dinv, C.omega, C.x, 0, s);
    } else {
      launch_mg_dg_restrict(d, c->st, c->r, c->w, mask, C.b, C.dinv, C.omega, C.x, kg0, s);
    }
    if (int e = mg_level(c, 1)) return e;
    launch_mg_dg_prolong(d, c->st, c->mgx, C.x, mask, kg0, s);
    launch_dg_japply(d, T, c->mgx, c->w, nullptr, nullptr, s, c->st);
    launch_dg_bpost(d, c->st, c->mgx, c->r, c->w, c->dggface, c->mg_omega0, c->z, c->partials, tail, s);
    return TV_OK;
  }
  const MgView v = mg_view(c, 0, T);
  if (!c->mg.empty()) {
    if (int e = mg_restrict_into(c, v, c->mg[0], mask, c->nT < kMgFoldFacesNodes)) return e;
    if (int e = mg_level(c, 1)) return e;
    mg_prolong_from(c, 0, c->mgx, mask);
  }
  mg_close0(c, v, tail);
  return TV_OK;
}

int mg_cycle(Ctx* c, const double* T, const RedTail* tail) {
  if (c->amg_on) return amg_apply0(c, tail);  // the algebraic cycle, agglomerated on partitions (tv_amg.cpp)
  if (c->n_parts > 1 && c->smoother0 != Smoother0::DG_BLOCK) return mg_cycle_dist(c, T, tail);
  return mg_cycle_box(c, T, tail);
}

int mg_dist_begin(Ctx* c, const double* T) {
  // the algebraic hierarchy is T-independent: level 0's weight at the first solve instead
  if (int e = c->amg_on ? level0_weight(c, T) : mg_prepare(c, T)) return e;
  if (dirichlet_masks(c))  // the prolongation masks level 0's ghost planes with dinv too
    if (int e = halo(c, c->dinv)) return e;
  if (c->mg_mask0)  // level 0's restriction mask: owned nodes, Dirichlet rows out
    launch_mg_ownmask(c->nT, c->ownT_off, c->ownT_off + c->ownT_n, dirichlet_masks(c) ? c->dinv : nullptr,
                      c->mg_mask0, c->stream);
  return TV_OK;
}

static int mg_iteration(Ctx* c, const double* T, int it) {
  RedTail t1{c->counters, c->partials, c->sums, c->st, 2, iter_stamp(c, it)};
  int np = 0;
  if (!op_japply_fused(c, T, &np, &t1, it))  // p <- z + b p ; w <- J p ; p.w ; alpha
    if (int e = reduce_logic(c, np, 1, 2, 1)) return e;
  level0_update(c, it, false, 0, c->nT);
  RedTail t2{c->counters + kTailCounters, c->partials, c->sums, c->st, 3, nullptr};
  return mg_cycle(c, T, &t2);  // z <- V(r); z.z, z.r; beta, convergence
}

// The three multigrid solves queue alike.  An MG iteration is ~25 launches: the
// count this Newton index took in the last step (hint) is queued right behind
// the init, with no host wait in between (the GPU would idle while the host
// enqueues ~100 launches), then one iteration at a time behind a poll.  The
// Newton solves of a step take near-constant counts, so the hint usually ends
// the solve at the first poll.  On several ranks every rank takes the same
// decisions: the polled state is formed from all-reduced sums, identical on
// every rank.
KrylovPolicy mg_krylov_policy(Ctx* c) {
  KrylovPolicy p{};
  p.ahead = false;
  p.hints = c->mg_hint;
  p.hint_min = 0;
  p.first_default = 1;
  p.hint_floor = 1;
  p.next = 1;
  p.guard = c->O.ksp_max_it + 2;
  p.ts_reserve = c->O.ksp_max_it + 8;
  return p;
}

int pcg_solve_mg(Ctx* c, const double* T, int* its, int* reason, bool post) {
  const int64_t n = c->nT;
  solve_begin(c, c->solve_gate);
  if (int e = mg_prepare(c, T)) return e;
  if (int e = level0_weight(c, T)) return e;
  level0_update(c, 0, true, 0, n);  // dx <- 0, x0 <- omega0 B^-1 r
  RedTail t0{c->counters + kTailCounters, c->partials, c->sums, c->st, 1, nullptr};
  if (int e = mg_cycle(c, T, &t0)) return e;  // z <- V(r); dp, beta (KSPCG init)
  auto iterate = [&](int it, int, int) { return mg_iteration(c, T, it); };
  auto published = [&]() -> int {
    if (!post) return TV_OK;
    // the Newton iteration's next work, queued before the host's poll (it runs once)
    launch_post_group(n, c->st, c->pA, c->pB, c->f[TV_F_DX].ptr, c->f[TV_F_T].ptr, c->partials, c->sums, c->stream);
    return queue_newton_norm(c, c->sums);
  };
  if (int e = krylov_drive(c, mg_krylov_policy(c), iterate, published, its, reason)) return e;
  // level 0 updates dx in pairs of iterations from iteration 1 on (level0_update's
  // kernels, DXU): solves of 0 / 1 iterations and the last step of an odd-length one
  if (!post) launch_mg_dx_finish(n, c->st, c->pA, c->pB, c->f[TV_F_DX].ptr, *its, c->stream);
  return TV_OK;
}

}  // namespace tv

using namespace tv;

extern "C" {

// On a partition (collective: every rank calls it): the operator the partitioned
// Krylov solve applies, on this rank's owned dofs -- Jacobi, or the partitioned
// V-cycle (GLOBAL: the distributed cycle of the whole box; LOCAL: this slab's own)
int tv_precond_apply(void* ctx, const double* r_dev, double* z_dev) {
  Ctx* c = static_cast<Ctx*>(ctx);
  if (!c || !r_dev || !z_dev) return TV_ERR_ARG;
  hipSetDevice(c->device);
  HIPC(hipDeviceSynchronize());  // inputs written on other streams (header)
  const bool part = c->n_parts > 1;
  const double* T = c->f[TV_F_T].ptr;
  if (part) {
    if (int e = require_comm(c, "tv_precond_apply")) return e;
    if (c->um || c->fam_T != TV_CG) return c->fail(TV_ERR_ARG, "tv_precond_apply: partitioned CG1 box meshes");
    if (int e = halo(c, c->f[TV_F_T].ptr)) return e;  // the PC setup reads the ghost planes' T (side-face facets)
  }
  const int64_t off = c->ownT_off, n = c->ownT_n;  // one partition: every dof
  hipStream_t s = c->stream;
  level0_setup(c, T);  // the PC setup of the Newton iteration at this T
  // Dirichlet mode: the solve's preconditioner acts on the free subspace only
  // (dinv = 0 on the constrained rows, as k_bc_lift sets it before every solve;
  // the V-cycle masks its transfers with the same dinv)
  if (c->dir_on && c->fam_T == TV_CG) launch_bc_mask(c, c->dinv);
  if (int e = level0_weight(c, T)) return e;
  if (!c->mg_on) {
    launch_mg_jacobi(n, nullptr, r_dev, nullptr, nullptr, c->dinv + off, 1.0, z_dev, 0, s);  // z = dinv .* r
  } else {
    PcgState h{};  // running state: the V-cycle's kernels skip work once a solve is done
    HIPC(hipMemcpyAsync(c->st, &h, sizeof(PcgState), hipMemcpyHostToDevice, s));
    if (int e = part ? mg_dist_begin(c, T) : mg_prepare(c, T)) return e;
    HIPC(hipMemcpyAsync(c->r + off, r_dev, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, s));
    int64_t woff, nwin;  // deep-ghost slabs: r on the ghost planes, x0 on the write window
    fine_window(c, &woff, &nwin);
    if (c->ghost_depth > 1)
      if (int e = halo(c, c->r)) return e;
    level0_smooth(c, c->st, c->r, c->mg_omega0, c->mgx, woff, nwin);  // x0 = omega0 B^-1 r
    if (int e = mg_cycle(c, T, nullptr)) return e;
    HIPC(hipMemcpyAsync(z_dev, c->z + off, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, s));
  }
  HIPC(hipGetLastError());
  HIPC(hipStreamSynchronize(s));
  return TV_OK;
}

}  // extern "C"

// Ensembles of independent 1D bars (parameter studies of the reference's own
// main.py workload): host side of csrc/tv_ensemble.hip (CG1 temperature and
// stress) and csrc/tv_ensemble_dg.hip (DG1 temperature, CG1 stress: main.py's
// own fe_config).  C-ABI: include/tvfem.h, tv_ensemble_*.
//   tv_ensemble_create / _create_dg    ThermoViscoProblem.__init__ once per bar
//   tv_ensemble_create_paper           the same with model_mode PAPER or PAPER_EXACT, either pairing
//   tv_ensemble_set_initial_condition  _set_initial_condition (:187-233), each bar's T_0
//   tv_ensemble_step                   n_steps x solve_timestep (:367-381) minus the
//                                      file output, every bar, one launch per
//                                      kMaxNodeStepsPerLaunch of work
#include <set>

#include "tv_ctx.h"

namespace tv {

// Upper bound of n_steps x n_nodes per launch.  A lane spends about 3 us per
// node and step (measured: 2.9 us on the 49-node main.py bar, three Newton
// iterations of two dependent sweeps plus the viscoelastic update, mostly
// memory latency, the same from 64 to 16384 bars), so one launch stays below
// half a second, far from any watchdog, while a 500-step main.py run of a
// bar of up to 262 nodes is still a single launch.
// A DG handle counts its T dofs (two per cell) in place of the nodes: measured
// 2.2 us per T dof and step on the 48-cell main.py bar from 64 to 1024 bars
// (one division per cell, six scratch values per cell), 2.8 at 4096 and 3.2 at
// 16384 bars, so a launch stays below 0.42 s.
constexpr int64_t kMaxNodeStepsPerLaunch = 1 << 17;

struct Ens {
  std::string err;
  int device = 0;
  hipStream_t stream = nullptr;
  tv_options O{};
  EnsArgs a{};
  ViscoConst vc{};
  ViscoFields vf{};
  std::vector<double> T0;     // per bar
  std::vector<double> par;    // [3][n_bars] htc, T_ambient, epsilon as created (a schedule's NULL tables)
  std::vector<void*> bufs;    // every device allocation that lives as long as the handle
  EnsExt x{};                 // schedule and history as the kernel reads them ...
  EnsExt* dx = nullptr;       // ... and their device copy (in bufs)
  void* sched_buf = nullptr;  // the stage tables in one allocation
  void* hist_buf = nullptr;   // the records, then the probe nodes
  bool ext() const { return x.n_stages > 0 || x.n_probes > 0; }
  double* field[TV_NUM_FIELDS] = {};
  int bs[TV_NUM_FIELDS] = {};
  int nd[TV_NUM_FIELDS] = {};  // dofs per bar of the field's family
  bool dg = false;             // DG1 temperature (tv_ensemble_create_dg): nT = 2 n_cells, nS = n_cells + 1
  int nT = 0, nS = 0;          // T-family / sigma-family dofs per bar (CG: both n_cells + 1)
  int steps_done = 0;
  int fail(int code, const std::string& m) {
    err = m;
    return code;
  }
};

static std::mutex g_ens_mu;
static std::set<const void*> g_ens_live;  // routes tv_last_error

const char* ensemble_last_error(const void* h) {
  std::lock_guard<std::mutex> lk(g_ens_mu);
  if (!g_ens_live.count(h)) return nullptr;
  return static_cast<const Ens*>(h)->err.c_str();
}

namespace {

int ens_alloc(Ens* c, size_t bytes, void** out, int kind = kMemDoubles) {
  HIPC(tv_dev_alloc(out, bytes, kind));
  c->bufs.push_back(*out);
  HIPC(hipMemsetAsync(*out, 0, bytes, c->stream));
  return TV_OK;
}

int ens_alloc_field(Ens* c, int id, int bs, int n_dofs) {
  void* p = nullptr;
  if (int e = ens_alloc(c, sizeof(double) * (size_t)bs * n_dofs * c->a.nb_pad, &p)) return e;
  c->field[id] = static_cast<double*>(p);
  c->bs[id] = bs;
  c->nd[id] = n_dofs;
  return TV_OK;
}

// host [bar][dof * bs + comp]  <->  device [comp][dof][bar], dof counted in the field's own family
int ens_transfer(Ens* c, int field, double* host, size_t n_values, bool to_device) {
  if (field < 0 || field >= TV_NUM_FIELDS || !c->field[field])
    return c->fail(TV_ERR_STATE, "tv_ensemble: field " + std::to_string(field) + " is not part of an ensemble's state");
  const int bs = c->bs[field], n = c->nd[field], nb = c->a.n_bars;
  const int64_t pad = c->a.nb_pad;
  if (!host || n_values != (size_t)nb * n * bs) return c->fail(TV_ERR_ARG, "tv_ensemble: field size mismatch");
  std::vector<double> dev((size_t)bs * n * pad);
  const size_t bytes = dev.size() * sizeof(double);
  HIPC(hipMemcpyAsync(dev.data(), c->field[field], bytes, hipMemcpyDeviceToHost, c->stream));
  HIPC(hipStreamSynchronize(c->stream));
  for (int b = 0; b < nb; ++b)
    for (int i = 0; i < n; ++i)
      for (int q = 0; q < bs; ++q) {
        double& d = dev[((size_t)q * n + i) * pad + b];
        double& h = host[((size_t)b * n + i) * bs + q];
        if (to_device) d = h;
        else h = d;
      }
  if (to_device) {
    HIPC(hipMemcpyAsync(c->field[field], dev.data(), bytes, hipMemcpyHostToDevice, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
  }
  return TV_OK;
}

// the kernel reads schedule and history through the device copy of Ens::x (allocated with the first
// of either, so an ensemble without them allocates what it always did)
int ens_push_ext(Ens* c) {
  if (!c->dx) {
    void* p = nullptr;
    if (int e = ens_alloc(c, sizeof(EnsExt), &p, kMemOther)) return e;
    c->dx = static_cast<EnsExt*>(p);
  }
  HIPC(hipMemcpyAsync(c->dx, &c->x, sizeof(EnsExt), hipMemcpyHostToDevice, c->stream));
  HIPC(hipStreamSynchronize(c->stream));
  return TV_OK;
}

// tv_ensemble_create (dg = false), tv_ensemble_create_dg (dg = true) and tv_ensemble_create_paper (paper:
// model_mode PAPER or PAPER_EXACT required, both refused by the other two): every refusal but the device's
// is decided before the first HIP call
int ens_create(const char* fn, bool dg, bool paper, const tv_ensemble_desc* d, const tv_fe_config* fe,
               const tv_params* P, const tv_options* opts, int device, void** ens_out) {
  if (!d || !fe || !P || !ens_out) {
    set_global_error(std::string(fn) + ": null argument");
    return TV_ERR_ARG;
  }
  *ens_out = nullptr;
  auto bad = [fn](const std::string& m) {
    set_global_error(std::string(fn) + ": " + m);
    return TV_ERR_ARG;
  };
  if (d->n_bars < 1) return bad("n_bars must be at least 1");
  if (d->n_cells < 1) return bad("n_cells must be at least 1");
  if (!d->coords) return bad("coords is null");
  const bool cg_stress = fe->sigma_family == TV_CG && fe->sigma_degree == 1;
  if (!dg && (fe->T_family != TV_CG || fe->T_degree != 1 || !cg_stress))
    return bad("only CG1 temperature with CG1 stress is implemented (DG temperature is out of scope)");
  if (dg && (fe->T_family != TV_DG || fe->T_degree != 1 || !cg_stress)) {
    if (fe->T_family == TV_CG && fe->T_degree == 1 && cg_stress)
      return bad("only DG1 temperature with CG1 stress is implemented here (CG1 temperature: tv_ensemble_create)");
    return bad("only DG1 temperature with CG1 stress is implemented");
  }
  auto c = std::make_unique<Ens>();
  c->dg = dg;
  if (opts) c->O = *opts;
  else tv_default_options(&c->O);
  if (paper) {
    if (!opts) return bad("options are required and must set model_mode PAPER (reference mode: tv_ensemble_create" +
                          std::string(dg ? "_dg)" : ")"));
    if (c->O.model_mode != TV_MODEL_PAPER && c->O.model_mode != TV_MODEL_PAPER_EXACT)
      return bad("model_mode must be PAPER (reference mode: tv_ensemble_create" + std::string(dg ? "_dg)" : ")"));
  } else if (c->O.model_mode != TV_MODEL_REFERENCE) {
    return bad("model_mode PAPER is not implemented for ensembles");
  }
  const bool exact = paper && c->O.model_mode == TV_MODEL_PAPER_EXACT;
  if (!(P->dt > 0.0)) return bad("dt must be positive");
  if (c->O.newton_max_it < 1 || c->O.newton_rtol < 0.0 || c->O.newton_atol < 0.0)
    return bad("newton_max_it < 1 or a negative Newton tolerance");
  const int nb = d->n_bars, n = d->n_cells + 1;
  for (int b = 0; b < (d->coords_shared ? 1 : nb); ++b) {
    const double* X = d->coords + (size_t)b * n;
    for (int i = 0; i + 1 < n; ++i)
      if (!(X[i + 1] > X[i])) return bad("coordinates of bar " + std::to_string(b) + " are not strictly increasing");
  }
  const int nT = dg ? 2 * (n - 1) : n, nS = n;  // dofs per bar of the T family / the sigma family
  const int64_t pad = ((int64_t)nb + kWave - 1) / kWave * kWave;
  if (pad * nT * 6 > INT64_C(1) << 40 || pad > INT32_MAX) return bad("ensemble too large");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    set_global_error("no HIP device available: libtvfem requires an MI355X (gfx950) GPU");
    return TV_ERR_HIP;
  }
  if (device < 0 || device >= ndev) return bad("device index out of range");
  c->device = device;
  if (hipSetDevice(device) != hipSuccess ||
      hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
    set_global_error("HIP stream creation failed");
    return TV_ERR_HIP;
  }
  EnsArgs& a = c->a;
  a.n_bars = nb;
  a.nb_pad = (int)pad;
  a.n_nodes = n;
  c->nT = nT;
  c->nS = nS;
  a.max_it = c->O.newton_max_it;
  a.rtol = c->O.newton_rtol;
  a.atol = c->O.newton_atol;
  a.dt = P->dt;
  a.sigma_sb = P->sigma;
  // per-bar parameters and cell coefficients, bar-fastest; padding lanes hold zeros (never read)
  auto per_bar = [&](const double* v, double dflt, int b) { return v ? v[b] : dflt; };
  std::vector<double> par((size_t)4 * pad, 0.0), cell((size_t)2 * (n - 1) * pad, 0.0);
  c->T0.resize(nb);
  for (int b = 0; b < nb; ++b) {
    par[b] = per_bar(d->htc, P->htc, b);
    par[pad + b] = per_bar(d->T_ambient, P->T_ambient, b);
    par[2 * pad + b] = per_bar(d->epsilon, P->epsilon, b);
    par[3 * pad + b] = per_bar(d->f, P->f, b);
    c->T0[b] = per_bar(d->T_0, P->T_0, b);
    const double alpha = per_bar(d->alpha, P->alpha, b);
    const double* X = d->coords + (d->coords_shared ? 0 : (size_t)b * n);
    for (int i = 0; i + 1 < n; ++i) {
      const double h = X[i + 1] - X[i];
      cell[(size_t)i * pad + b] = h / 6.0;
      cell[((size_t)(n - 1) + i) * pad + b] = P->dt * alpha / h;
    }
  }
  int rc = TV_OK;
  void *dpar = nullptr, *dcell = nullptr, *scr = nullptr, *its = nullptr, *fs = nullptr, *tot = nullptr;
  // id, block size, family (0: T, 1: sigma)
  static const int kState[][3] = {{TV_F_T, 1, 0}, {TV_F_T_PREV, 1, 0}, {TV_F_TF, 1, 0}, {TV_F_TF_PARTIAL, 6, 0},
                                  {TV_F_PHI, 1, 0}, {TV_F_XI, 1, 0}, {TV_F_SIGMA, 1, 1}, {TV_F_S_TILDE, 6, 1},
                                  {TV_F_SIGMA_TILDE, 6, 1}};
  for (const auto& s : kState)
    if (rc == TV_OK) rc = ens_alloc_field(c.get(), s[0], s[1], s[2] ? nS : nT);
  // paper mode: the partial stresses are state (Eq. 16 reads them back); zero as allocated, as in the oracle
  if (paper && rc == TV_OK) rc = ens_alloc_field(c.get(), TV_F_S_PARTIAL, 6, nS);
  if (paper && rc == TV_OK) rc = ens_alloc_field(c.get(), TV_F_SIGMA_PARTIAL, 6, nS);
  if (rc == TV_OK) rc = ens_alloc(c.get(), par.size() * sizeof(double), &dpar);
  if (rc == TV_OK) rc = ens_alloc(c.get(), cell.size() * sizeof(double), &dcell);
  // Thomas scratch [2][n_nodes][pad]; DG: C and d of the block elimination, [6][n_cells][pad]
  if (rc == TV_OK) rc = ens_alloc(c.get(), sizeof(double) * (dg ? (size_t)6 * (n - 1) : (size_t)2 * n) * pad, &scr);
  if (rc == TV_OK) rc = ens_alloc(c.get(), sizeof(int) * pad, &its, kMemOther);
  if (rc == TV_OK) rc = ens_alloc(c.get(), sizeof(int) * pad, &fs, kMemOther);
  if (rc == TV_OK) rc = ens_alloc(c.get(), sizeof(int64_t) * pad, &tot, kMemOther);
  auto upload = [&](void* dst, const std::vector<double>& src) {
    HIPC(hipMemcpyAsync(dst, src.data(), src.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPC(hipStreamSynchronize(c->stream));
    return (int)TV_OK;
  };
  if (rc == TV_OK) rc = upload(dpar, par);
  if (rc == TV_OK) rc = upload(dcell, cell);
  if (rc != TV_OK) {
    set_global_error(c->err);
    for (void* p : c->bufs) tv_dev_free(p);
    hipStreamDestroy(c->stream);
    return rc;
  }
  double* dp = static_cast<double*>(dpar);
  a.htc = dp;
  a.T_amb = dp + pad;
  a.eps = dp + 2 * pad;
  a.f = dp + 3 * pad;
  a.cm = static_cast<double*>(dcell);
  a.ck = a.cm + (size_t)(n - 1) * pad;
  a.T = c->field[TV_F_T];
  a.Tp = c->field[TV_F_T_PREV];
  a.scr = static_cast<double*>(scr);
  a.its_last = static_cast<int*>(its);
  a.failed_step = static_cast<int*>(fs);
  a.newton_total = static_cast<int64_t*>(tot);
  c->x.every = 1;
  c->par.resize((size_t)3 * nb);
  for (int q = 0; q < 3; ++q) std::copy_n(par.begin() + (size_t)q * pad, nb, c->par.begin() + (size_t)q * nb);
  fill_visco_const(c->vc, *P, 1, exact ? 2 : (paper ? 1 : 0));  // the kernels' model id
  ViscoFields& v = c->vf;
  std::memset(&v, 0, sizeof(v));
  v.sT = (int64_t)nT * pad;
  v.sS = (int64_t)nS * pad;
  v.T = c->field[TV_F_T]; v.Tp = c->field[TV_F_T_PREV];
  v.phi = c->field[TV_F_PHI]; v.xi = c->field[TV_F_XI];
  v.Tf = c->field[TV_F_TF]; v.Tfp = c->field[TV_F_TF_PARTIAL];
  v.st = c->field[TV_F_S_TILDE]; v.sgt = c->field[TV_F_SIGMA_TILDE];
  v.sigma = c->field[TV_F_SIGMA];
  v.sp = c->field[TV_F_S_PARTIAL]; v.sgp = c->field[TV_F_SIGMA_PARTIAL];  // null on a reference handle
  {
    std::lock_guard<std::mutex> lk(g_ens_mu);
    g_ens_live.insert(c.get());
  }
  *ens_out = c.release();
  return TV_OK;
}

}  // namespace
}  // namespace tv

using namespace tv;

extern "C" {

int tv_ensemble_create(const tv_ensemble_desc* d, const tv_fe_config* fe, const tv_params* P, const tv_options* opts,
                       int device, void** ens_out) {
  return ens_create("tv_ensemble_create", false, false, d, fe, P, opts, device, ens_out);
}


int tv_ensemble_create_dg(const tv_ensemble_desc* d, const tv_fe_config* fe, const tv_params* P,
                          const tv_options* opts, int device, void** ens_out) {
  return ens_create("tv_ensemble_create_dg", true, false, d, fe, P, opts, device, ens_out);
}


int tv_ensemble_create_paper(const tv_ensemble_desc* d, const tv_fe_config* fe, const tv_params* P,
                             const tv_options* opts, int device, void** ens_out) {
  // the family decides the kernel; a pairing neither accepts gets the refusal of that family's constructor
  const bool dg = fe && fe->T_family == TV_DG;
  return ens_create("tv_ensemble_create_paper", dg, true, d, fe, P, opts, device, ens_out);
}


int tv_ensemble_destroy(void* ens) {
  Ens* c = static_cast<Ens*>(ens);
  if (!c) return TV_ERR_ARG;
  {
    std::lock_guard<std::mutex> lk(g_ens_mu);
    if (!g_ens_live.erase(c)) return TV_ERR_ARG;
  }
  hipSetDevice(c->device);
  hipStreamSynchronize(c->stream);
  for (void* p : c->bufs) tv_dev_free(p);
  tv_dev_free(c->sched_buf);
  tv_dev_free(c->hist_buf);
  hipStreamDestroy(c->stream);
  delete c;
  return TV_OK;
}


int tv_ensemble_set_initial_condition(void* ens) {
  Ens* c = static_cast<Ens*>(ens);
  if (!c) return TV_ERR_ARG;
  hipSetDevice(c->device);
  // __set_IC_T, __set_IC_Tf, __set_IC_Tf_partial (ThermoViscoProblem.py:193-233) with each bar's T_0
  const int n = c->nT;  // all four are T-family fields
  const int64_t pad = c->a.nb_pad;
  std::vector<double> v((size_t)6 * n * pad, 0.0);
  for (int q = 0; q < 6 * n; ++q)
    for (int b = 0; b < c->a.n_bars; ++b) v[(size_t)q * pad + b] = c->T0[b];
  const size_t plane = sizeof(double) * n * pad;
  HIPC(hipMemcpyAsync(c->field[TV_F_T], v.data(), plane, hipMemcpyHostToDevice, c->stream));
  HIPC(hipMemcpyAsync(c->field[TV_F_T_PREV], v.data(), plane, hipMemcpyHostToDevice, c->stream));
  HIPC(hipMemcpyAsync(c->field[TV_F_TF], v.data(), plane, hipMemcpyHostToDevice, c->stream));
  HIPC(hipMemcpyAsync(c->field[TV_F_TF_PARTIAL], v.data(), 6 * plane, hipMemcpyHostToDevice, c->stream));
  // a paper handle's stress memory starts at zero (the oracle's s_partial / sigma_partial)
  for (int id : {TV_F_S_PARTIAL, TV_F_SIGMA_PARTIAL})
    if (c->field[id]) HIPC(hipMemsetAsync(c->field[id], 0, sizeof(double) * 6 * c->nS * pad, c->stream));
  HIPC(hipStreamSynchronize(c->stream));
  return TV_OK;
}


int tv_ensemble_step(void* ens, int n_steps, int thermal_only) {
  Ens* c = static_cast<Ens*>(ens);
  if (!c) return TV_ERR_ARG;
  if (n_steps < 0 || (int64_t)c->steps_done + n_steps > INT32_MAX - 1)
    return c->fail(TV_ERR_ARG, "tv_ensemble_step: n_steps out of range");
  if (c->x.n_probes > 0 && (int64_t)c->steps_done + n_steps > (int64_t)c->x.max_records * c->x.every)
    return c->fail(TV_ERR_STATE, "tv_ensemble_step: step " + std::to_string((int64_t)c->steps_done + n_steps) +
                                     " lies past the open history (max_records " + std::to_string(c->x.max_records) +
                                     " x every " + std::to_string(c->x.every) + "); no bar has advanced");
  hipSetDevice(c->device);
  const int before = c->steps_done;
  const int per_launch = (int)std::max<int64_t>(1, kMaxNodeStepsPerLaunch / c->nT);
  for (int left = n_steps; left > 0;) {
    EnsArgs a = c->a;
    a.n_steps = std::min(left, per_launch);
    a.step_base = c->steps_done;
    a.thermal_only = thermal_only ? 1 : 0;
    (c->dg ? launch_ensemble_dg : launch_ensemble)(a, c->vc, c->vf, c->ext() ? c->dx : nullptr, c->stream);
    HIPC(hipGetLastError());
    c->steps_done += a.n_steps;
    left -= a.n_steps;
  }
  // the failure records decide the status: wait for the launches
  std::vector<int> failed(c->a.n_bars);
  HIPC(hipMemcpyAsync(failed.data(), c->a.failed_step, sizeof(int) * failed.size(), hipMemcpyDeviceToHost, c->stream));
  HIPC(hipStreamSynchronize(c->stream));
  if (!c->O.error_on_nonconvergence) return TV_OK;
  for (int b = 0; b < c->a.n_bars; ++b)
    if (failed[b] > before)
      return c->fail(TV_ERR_NOT_CONVERGED,
                     "Newton solver did not converge because maximum number of iterations reached: bar " +
                         std::to_string(b) + " at step " + std::to_string(failed[b]) + " (first failed bar; frozen)");
  return TV_OK;
}


int tv_ensemble_get_field(void* ens, int field, double* host, size_t n_values) {
  Ens* c = static_cast<Ens*>(ens);
  if (!c) return TV_ERR_ARG;
  hipSetDevice(c->device);
  return ens_transfer(c, field, host, n_values, false);
}


int tv_ensemble_set_field(void* ens, int field, const double* host, size_t n_values) {
  Ens* c = static_cast<Ens*>(ens);
  if (!c) return TV_ERR_ARG;
  hipSetDevice(c->device);
  return ens_transfer(c, field, const_cast<double*>(host), n_values, true);
}


int tv_ensemble_stats(void* ens, int* newton_its_last, int* failed_step, int64_t* newton_total) {
  Ens* c = static_cast<Ens*>(ens);
  if (!c) return TV_ERR_ARG;
  hipSetDevice(c->device);
  const size_t nb = c->a.n_bars;
  if (newton_its_last)
    HIPC(hipMemcpyAsync(newton_its_last, c->a.its_last, sizeof(int) * nb, hipMemcpyDeviceToHost, c->stream));
  if (failed_step)
    HIPC(hipMemcpyAsync(failed_step, c->a.failed_step, sizeof(int) * nb, hipMemcpyDeviceToHost, c->stream));
  if (newton_total)
    HIPC(hipMemcpyAsync(newton_total, c->a.newton_total, sizeof(int64_t) * nb, hipMemcpyDeviceToHost, c->stream));
  HIPC(hipStreamSynchronize(c->stream));
  return TV_OK;
}


int tv_ensemble_set_schedule(void* ens, const tv_ensemble_schedule* s) {
  Ens* c = static_cast<Ens*>(ens);
  if (!c) return TV_ERR_ARG;
  hipSetDevice(c->device);
  if (!s) {  // back to the creation values
    tv_dev_free(c->sched_buf);  // no launch is in flight: tv_ensemble_step returns after its launches
    c->sched_buf = nullptr;
    c->x.n_stages = 0;
    c->x.stage_end = nullptr;
    c->x.htc = c->x.T_amb = c->x.eps = nullptr;
    return ens_push_ext(c);
  }
  auto bad = [&](const std::string& m) { return c->fail(TV_ERR_ARG, "tv_ensemble_set_schedule: " + m); };
  const int nst = s->n_stages, nb = c->a.n_bars;
  const int64_t pad = c->a.nb_pad;
  if (nst < 1) return bad("n_stages must be at least 1");
  if ((nst == 1) != (s->stage_end == nullptr))
    return bad("stage_end is NULL if and only if n_stages == 1");
  if (nst * pad > INT32_MAX) return bad("schedule too large");
  for (int b = 0; b < nb; ++b)
    for (int j = 0, prev = 0; j + 1 < nst; ++j) {
      const int e = s->stage_end[(size_t)j * nb + b];
      if (e < 0) return bad("stage_end of bar " + std::to_string(b) + ", stage " + std::to_string(j) + " is negative");
      if (e < prev)
        return bad("stage_end of bar " + std::to_string(b) + " decreases at stage " + std::to_string(j));
      prev = e;
    }
  const double* tab[3] = {s->htc, s->T_ambient, s->epsilon};
  static const char* const kName[3] = {"htc", "T_ambient", "epsilon"};
  for (int q = 0; q < 3; ++q)
    for (size_t i = 0; tab[q] && i < (size_t)nst * nb; ++i)
      if (!std::isfinite(tab[q][i]))
        return bad(std::string(kName[q]) + " of bar " + std::to_string(i % nb) + ", stage " + std::to_string(i / nb) +
                   " is not finite");
  // device rows (EnsExt): per bar its non-empty stages in order, the last stage closing the list
  // with INT32_MAX and repeated down to row nst - 1; padding lanes (never read) hold the same end
  const size_t rows = (size_t)nst * pad;
  std::vector<double> val(3 * rows, 0.0);
  std::vector<int> end(rows, INT32_MAX);
  for (int b = 0; b < nb; ++b) {
    int row = 0, prev = 0;
    auto put = [&](int j, int e) {
      for (int q = 0; q < 3; ++q)
        val[q * rows + (size_t)row * pad + b] = tab[q] ? tab[q][(size_t)j * nb + b] : c->par[(size_t)q * nb + b];
      end[(size_t)row * pad + b] = e;
    };
    int last = nst - 1;  // the stage that never ends: the last one, or one whose end no step can pass
    for (int j = 0; j + 1 < nst; ++j) {
      const int e = s->stage_end[(size_t)j * nb + b];
      if (e == prev) continue;  // empty
      if (e == INT32_MAX) {
        last = j;
        break;
      }
      put(j, e);
      prev = e;
      ++row;
    }
    for (; row < nst; ++row) put(last, INT32_MAX);
  }
  void* buf = nullptr;
  HIPC(tv_dev_alloc(&buf, val.size() * sizeof(double) + end.size() * sizeof(int), kMemOther));
  double* dval = static_cast<double*>(buf);
  int* dend = reinterpret_cast<int*>(dval + val.size());
  hipError_t e1 = hipMemcpyAsync(dval, val.data(), val.size() * sizeof(double), hipMemcpyHostToDevice, c->stream);
  hipError_t e2 = hipMemcpyAsync(dend, end.data(), end.size() * sizeof(int), hipMemcpyHostToDevice, c->stream);
  hipError_t e3 = hipStreamSynchronize(c->stream);
  if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) {
    tv_dev_free(buf);
    return c->fail(TV_ERR_HIP, "tv_ensemble_set_schedule: upload failed");
  }
  tv_dev_free(c->sched_buf);
  c->sched_buf = buf;
  c->x.n_stages = nst;
  c->x.stage_end = dend;
  c->x.htc = dval;
  c->x.T_amb = dval + rows;
  c->x.eps = dval + 2 * rows;
  return ens_push_ext(c);
}


int tv_ensemble_history_open(void* ens, int n_probes, const int* dofs, int every, int max_records) {
  Ens* c = static_cast<Ens*>(ens);
  if (!c) return TV_ERR_ARG;
  hipSetDevice(c->device);
  auto bad = [&](const std::string& m) { return c->fail(TV_ERR_ARG, "tv_ensemble_history_open: " + m); };
  if (n_probes < 0) return bad("n_probes is negative");
  if (n_probes == 0) {  // close: the records go, the step cap with them
    tv_dev_free(c->hist_buf);
    c->hist_buf = nullptr;
    c->x.n_probes = 0;
    c->x.every = 1;
    c->x.max_records = 0;
    c->x.probes = nullptr;
    c->x.hist = nullptr;
    return ens_push_ext(c);
  }
  if (!dofs) return bad("dofs is null");
  if (every < 1) return bad("every must be at least 1");
  if (max_records < 1) return bad("max_records must be at least 1");
  for (int p = 0; p < n_probes; ++p)
    if (dofs[p] < 0 || dofs[p] >= c->a.n_nodes)
      return bad("probe " + std::to_string(p) + " (dof " + std::to_string(dofs[p]) + ") lies outside [0, n_cells = " +
                 std::to_string(c->a.n_nodes - 1) + "]");
  const int64_t pad = c->a.nb_pad;
  if ((int64_t)max_records * every > INT32_MAX - 1) return bad("max_records x every exceeds the step range");
  if ((double)max_records * 3.0 * n_probes * (double)pad > (double)(INT64_C(1) << 37)) return bad("history too large");
  const size_t n_val = (size_t)max_records * 3 * n_probes * pad;
  void* buf = nullptr;
  HIPC(tv_dev_alloc(&buf, n_val * sizeof(double) + (size_t)n_probes * sizeof(int), kMemOther));
  double* dh = static_cast<double*>(buf);
  int* dprobes = reinterpret_cast<int*>(dh + n_val);
  // all bits set is a NaN: what a record reads until its step has written it
  hipError_t e1 = hipMemsetAsync(dh, 0xFF, n_val * sizeof(double), c->stream);
  hipError_t e2 = hipMemcpyAsync(dprobes, dofs, (size_t)n_probes * sizeof(int), hipMemcpyHostToDevice, c->stream);
  hipError_t e3 = hipStreamSynchronize(c->stream);
  if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) {
    tv_dev_free(buf);
    return c->fail(TV_ERR_HIP, "tv_ensemble_history_open: device setup failed");
  }
  tv_dev_free(c->hist_buf);
  c->hist_buf = buf;
  c->x.n_probes = n_probes;
  c->x.every = every;
  c->x.max_records = max_records;
  c->x.probes = dprobes;
  c->x.hist = dh;
  return ens_push_ext(c);
}


int tv_ensemble_history_read(void* ens, double* host, size_t n_values, int* n_records) {
  Ens* c = static_cast<Ens*>(ens);
  if (!c) return TV_ERR_ARG;
  hipSetDevice(c->device);
  if (c->x.n_probes == 0) return c->fail(TV_ERR_STATE, "tv_ensemble_history_read: no history is open");
  const int nrec = std::min(c->steps_done / c->x.every, c->x.max_records);
  if (n_records) *n_records = nrec;
  if (!host) {
    if (n_records) return TV_OK;  // a query of the record count
    return c->fail(TV_ERR_ARG, "tv_ensemble_history_read: host and n_records are both null");
  }
  const int np = c->x.n_probes, nb = c->a.n_bars;
  const int64_t pad = c->a.nb_pad;
  if (n_values < (size_t)nrec * 3 * nb * np)
    return c->fail(TV_ERR_ARG, "tv_ensemble_history_read: host holds fewer than n_records x 3 x n_bars x n_probes values");
  if (nrec == 0) return TV_OK;
  // device [record][field][probe][bar_pad]  ->  host [record][field][bar][probe]
  std::vector<double> dev((size_t)nrec * 3 * np * pad);
  HIPC(hipMemcpyAsync(dev.data(), c->x.hist, dev.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPC(hipStreamSynchronize(c->stream));
  for (size_t rf = 0; rf < (size_t)nrec * 3; ++rf)
    for (int b = 0; b < nb; ++b)
      for (int p = 0; p < np; ++p) host[(rf * nb + b) * np + p] = dev[(rf * np + p) * pad + b];
  return TV_OK;
}

}  // extern "C"

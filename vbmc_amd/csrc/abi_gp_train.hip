// C-ABI entry points for the two device-resident halves of gplite_train: vbmc_gp_slice_sample, vbmc_gp_train_optimize (and
// vbmc_slice_rng_dump) (include/vbmc_hip.h).  Both turn candidate hyper-parameter vectors into GP objective values on the device
// (gpobj_kernels.h) and are driven from the host in chunks of ROUNDS; what they share on the host is in the namespace below, over
// the factorisation core of gp_factor.h.
#include <algorithm>
#include <cmath>
#include <limits>

#include "gp_factor.h"
#include "parity_rng.h"
#include "round_driver.h"
#include "slice_kernels.h"
#include "trainopt_kernels.h"

namespace {

double host_eps(double x) {   // MATLAB's eps(x): NaN for an infinite x
  const double ax = std::fabs(x);
  return std::nextafter(ax, std::numeric_limits<double>::infinity()) - ax;
}

// hyper-prior classes and normalising terms (gplite_hypprior.m:34-36,49-58)
struct HyperPrior {
  std::vector<double> pmu, psig, pdf, pc;
  std::vector<int> ptype;
  HyperPrior(const double* prior_mu, const double* prior_sigma, const double* prior_df, int Nhyp)
      : pmu(Nhyp, 0.0), psig(Nhyp, 1.0), pdf(Nhyp, 7.0), pc(Nhyp, 0.0), ptype(Nhyp, 0) {
    if (prior_mu)
      for (int i = 0; i < Nhyp; ++i) {
        const double mu = prior_mu[i], sg = std::fabs(prior_sigma[i]), df = prior_df ? prior_df[i] : 7.0;
        if (!std::isfinite(mu) || !std::isfinite(sg)) continue;
        pmu[i] = mu; psig[i] = sg; pdf[i] = df;
        if (df == 0.0 || !std::isfinite(df)) { ptype[i] = 1; pc[i] = std::log(2.0 * 3.14159265358979323846 * sg * sg); }
        else if (df > 0.0) { ptype[i] = 2; pc[i] = std::lgamma(0.5 * (df + 1.0)) - std::lgamma(0.5 * df) - 0.5 * std::log(3.14159265358979323846 * df) - std::log(sg); }
      }
  }
};

// The factorisation workspace of B candidates at (N, D), and the value path of gplite_nlZ over it.
struct GpObjWork {
  GpWork w;
  // what the value path reads besides the workspace: set by the caller once its kernel arguments are laid out
  vbmc_ctx* ctx = nullptr;
  int N = 0, D = 0, Nhyp = 0, moff = 0, meanfun = 0;
  const double *X = nullptr, *y = nullptr, *hyp = nullptr, *sn2 = nullptr;
  double* scal = nullptr;
  unsigned char *act = nullptr, *on = nullptr;

  vbmc_status alloc(vbmc_ctx* c, int N_, int D_, int B) {
    ctx = c; N = N_; D = D_;
    return w.alloc(ctx, N, D, B);
  }
  // value path of n candidates whose inputs a propose launch has written; checked: with the nine x10 noise-inflation retries
  vbmc_status value_path(hipStream_t st, int n, int checked) {
    gp_launch_scale(st, N, D, n, Nhyp, moff, meanfun, X, hyp, w.dXc.as<double>(), w.daa.as<double>(), y, w.dr.as<double>());
    for (int t = 0; t < (checked ? 10 : 1); ++t) {
      if (t > 0) hipLaunchKernelGGL(k_gpobj_retry, dim3((n + 63) / 64), dim3(64), 0, st, n, w.dpf.as<int>(), scal, act);
      HIP_TRY(ctx, gp_launch_try(st, N, D, n, Nhyp, hyp, sn2, scal, act, w));
    }
    gp_launch_alpha(st, N, n, w.dA.as<double>(), w.dfinv.as<double>(), on, w.dz.as<double>(), w.dal.as<double>(), scal);
    return VBMC_OK;
  }
};

}  // namespace

// ------------------------------------------------------------------------------------------
// vbmc_gp_slice_sample: slicesamplebnd on the GP hyper-parameter posterior, the chain resident on the device (slice_kernels.h).
// The host enqueues ROUNDS (propose, the value path of gplite_nlZ for the W candidates, decide) in chunks on the context's stream and
// reads the chain's state word once per chunk, one chunk behind the one being enqueued: no round trip per evaluation.  A candidate
// whose first factorisation fails stalls the chain (rounds already enqueued become no-ops); the host then enqueues ONE checked round
// with the nine x10 noise-inflation retries of gplite_core.m:77-80,91-94 between the tries, all on the device, and goes on.
#define SLICE_DEFAULT_W 1   // the five-run table that a wider default has to rest on has not been measured (profiles/gp_slice_sample.md)
#define SLICE_CHUNK 32

extern "C" vbmc_status vbmc_slice_rng_dump(uint64_t seed, int sweeps, int Nhyp, int Kmax, int32_t* perms, double* uniforms) {
  if (sweeps <= 0 || Nhyp <= 0 || Kmax < 0) return VBMC_ERR_INVALID;
  for (int sw = 0; sw < sweeps; ++sw) {
    if (perms) {   // Fisher-Yates driven by the generator's permutation stream
      int32_t* p = perms + (size_t)sw * Nhyp;
      for (int i = 0; i < Nhyp; ++i) p[i] = i;
      for (int i = Nhyp - 1; i > 0; --i) {
        const unsigned j = slice_perm_word(seed, (unsigned)sw, (unsigned)i) % (unsigned)(i + 1);
        std::swap(p[i], p[j]);
      }
    }
    if (uniforms)
      for (int i = 0; i < Nhyp; ++i)
        for (int k = 0; k < 2 + Kmax; ++k)
          uniforms[((size_t)sw * Nhyp + i) * (size_t)(2 + Kmax) + k] = slice_uniform(seed, (unsigned)sw, (unsigned)i, (unsigned)k);
  }
  return VBMC_OK;
}

extern "C" vbmc_status vbmc_gp_slice_sample(vbmc_ctx* ctx, const vbmc_slice_args* args) {
  if (!ctx) return VBMC_ERR_INVALID;
  if (!args || args->struct_size != sizeof(vbmc_slice_args)) return set_err(ctx, VBMC_ERR_INVALID, "vbmc_gp_slice_sample: struct_size mismatch");
  const vbmc_slice_args& g = *args;
  const int N = g.N, D = g.D, Nhyp = g.Nhyp, meanfun = g.meanfun;
  if (N <= 0 || D <= 0 || !g.X || !g.y || !g.LB || !g.UB || !g.hyp_start || !g.widths)
    return set_err(ctx, VBMC_ERR_INVALID, "vbmc_gp_slice_sample: bad arguments");
  GpModel gm;
  VB_TRY(gp_noise_range_check(ctx, g.noisefun));
  VB_TRY(gp_model_check(ctx, "gplite_nlZ", N, D, Nhyp, meanfun, g.noisefun, 0, gm));
  const int Ncov = gm.Ncov, Nnoise = gm.Nnoise, Nmean = gm.Nmean;
  if (Nhyp > SLICE_MAXHYP) return set_err(ctx, VBMC_ERR_UNSUPPORTED, "Nhyp = %d > %d not accelerated", Nhyp, SLICE_MAXHYP);
  if (g.Ns < 1 || g.Thin < 1 || g.Burnin < 0)
    return set_err(ctx, VBMC_ERR_INVALID, "slicesamplebnd:options Ns and the thinning factor need to be positive integers, the burn-in non-negative.");
  if (g.W < 0 || g.W > SLICE_MAXW) return set_err(ctx, VBMC_ERR_INVALID, "vbmc_gp_slice_sample: speculation width W = %d outside 0 .. %d", g.W, SLICE_MAXW);
  if (g.rng_mode != 0 && g.rng_mode != 1) return set_err(ctx, VBMC_ERR_INVALID, "vbmc_gp_slice_sample: rng_mode %d (0 device, 1 parity)", g.rng_mode);
  if (g.rng_mode == 1 && (!g.perms || !g.uniforms || g.Kmax < 1))
    return set_err(ctx, VBMC_ERR_INVALID, "vbmc_gp_slice_sample: parity mode needs perms, uniforms and Kmax >= 1");
  if (g.prior_mu && !g.prior_sigma) return set_err(ctx, VBMC_ERR_INVALID, "vbmc_gp_slice_sample: prior_mu without prior_sigma");
  const long long total_ll = (long long)g.Burnin + g.Ns + (long long)(g.Ns - 1) * (g.Thin - 1);   // effN + burn (:205,229)
  if (total_ll > (1ll << 30) / Nhyp) return set_err(ctx, VBMC_ERR_INVALID, "vbmc_gp_slice_sample: %lld sweeps are too many", total_ll);
  const int total = (int)total_ll;
  std::vector<double> wd(g.widths, g.widths + Nhyp), xx0(g.hyp_start, g.hyp_start + Nhyp), LBo(Nhyp), UBo(Nhyp);
  for (int i = 0; i < Nhyp; ++i) {
    const double lb = g.LB[i], ub = g.UB[i];
    if (lb != lb || ub != ub || !(ub >= lb))
      return set_err(ctx, VBMC_ERR_INVALID, "slicesamplebnd:bounds All upper bounds UB need to be equal or greater than lower bounds LB.");
    if (lb == ub) wd[i] = 1.0;                                            // (:185)
    if (!(wd[i] > 0.0) || !std::isfinite(wd[i]))
      return set_err(ctx, VBMC_ERR_INVALID, "slicesamplebnd:widths The vector WIDTHS need to be all positive real numbers.");
    if (!(xx0[i] >= lb && xx0[i] <= ub))
      return set_err(ctx, VBMC_ERR_INVALID, "slicesamplebnd:start The initial starting point X0 is outside the bounds.");
    if (g.basewidths && !(g.basewidths[i] >= 0.0))
      return set_err(ctx, VBMC_ERR_INVALID, "slicesamplebnd:widths The vector WIDTHS need to be all positive real numbers.");
    LBo[i] = lb - host_eps(lb);                                           // (:164-165)
    UBo[i] = ub + host_eps(ub);
  }
  if (g.rng_mode == 1)
    for (size_t e = 0; e < (size_t)total * Nhyp; ++e)
      if (g.perms[e] < 0 || g.perms[e] >= Nhyp) return set_err(ctx, VBMC_ERR_INVALID, "vbmc_gp_slice_sample: perms holds an index outside 0 .. Nhyp - 1");
  const HyperPrior pr(g.prior_mu, g.prior_sigma, g.prior_df, Nhyp);
  int W = g.W == 0 ? SLICE_DEFAULT_W : g.W;
  while (W > 1 && (size_t)W * N * N * 8 > ((size_t)2 << 30)) --W;        // the W factorisations' work matrices stay below 2 GiB (include/vbmc_hip.h says so)
  std::vector<int32_t> perm_own;
  const int32_t* perms = g.perms;
  if (g.rng_mode == 0) {
    perm_own.resize((size_t)total * Nhyp);
    vbmc_slice_rng_dump(g.seed, total, Nhyp, 0, perm_own.data(), nullptr);
    perms = perm_own.data();
  }

  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const size_t nU = g.rng_mode == 1 ? (size_t)total * Nhyp * (size_t)(2 + g.Kmax) : 0;
  const SliceBlocks L(N, D, Nhyp, g.s2 != nullptr, total, nU, g.Ns);   // one block of fp64 inputs / chain vectors, one of work space
  TmpBuf dIn, dInt, dState, dHyp, dSn2, dScal, dLp, dFlags, dOut, dSmp;
  GpObjWork wk;
  HIP_TRY(ctx, dIn.alloc(ctx, L.in.bytes()));
  HIP_TRY(ctx, dInt.alloc(ctx, L.ints.bytes()));
  HIP_TRY(ctx, dState.alloc(ctx, sizeof(SliceChainState)));
  HIP_TRY(ctx, dHyp.alloc(ctx, (size_t)W * Nhyp * 8));
  HIP_TRY(ctx, dSn2.alloc(ctx, (size_t)W * N * 8));
  HIP_TRY(ctx, dScal.alloc(ctx, (size_t)W * 4 * 8));
  HIP_TRY(ctx, dLp.alloc(ctx, (size_t)W * 8));
  HIP_TRY(ctx, dFlags.alloc(ctx, L.flags.bytes()));
  VB_TRY(wk.alloc(ctx, N, D, W));
  HIP_TRY(ctx, dOut.alloc(ctx, (size_t)W * 2 * 8));
  HIP_TRY(ctx, dSmp.alloc(ctx, L.smp.bytes()));
  VB_TRY(ensure_pin(ctx, 2 * sizeof(SliceChainState) + 64));              // two landing slots of the progress word

  std::vector<double> hin(L.in.count(), 0.0);                            // (basew without the caller's; xsum, xsq start at zero)
  L.head.pack(hin.data(), g.X, g.y, g.s2);
  L.LB.put(hin.data(), g.LB); L.UB.put(hin.data(), g.UB); L.LBo.put(hin.data(), LBo.data()); L.UBo.put(hin.data(), UBo.data());
  L.prior.pack(hin.data(), pr.pmu.data(), pr.psig.data(), pr.pdf.data(), pr.pc.data());
  L.basew.put(hin.data(), g.basewidths); L.xx.put(hin.data(), xx0.data()); L.widths.put(hin.data(), wd.data()); L.U.put(hin.data(), g.uniforms);
  std::vector<int> hint(L.ints.count<int>());
  L.perms.put(hint.data(), perms); L.ptype.put(hint.data(), pr.ptype.data());
  HIP_TRY(ctx, hipMemcpyAsync(dIn.p, hin.data(), L.in.bytes(), hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(dInt.p, hint.data(), L.ints.bytes(), hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemsetAsync(dState.p, 0, sizeof(SliceChainState), st));
  HIP_TRY(ctx, hipMemsetAsync(dFlags.p, 0, L.flags.bytes(), st));
  HIP_TRY(ctx, hipMemsetAsync(dHyp.p, 0, (size_t)W * Nhyp * 8, st));     // k_gp_scale / k_nlz_final are not gated: they read every row
  HIP_TRY(ctx, hipMemsetAsync(dScal.p, 0, (size_t)W * 4 * 8, st));

  SliceKernelArgs a{};
  a.N = N; a.D = D; a.Nhyp = Nhyp; a.Ncov = Ncov; a.Nnoise = Nnoise; a.W = W; a.Kmax = g.Kmax; a.Ns = g.Ns; a.thin = g.Thin; a.burn = g.Burnin;
  a.adaptive = g.Adaptive ? 1 : 0; a.total = total; a.parity = g.rng_mode; a.nf0 = g.noisefun[0]; a.nf1 = g.noisefun[1]; a.nf2 = g.noisefun[2];
  a.has_base = g.basewidths ? 1 : 0; a.has_prior = g.prior_mu ? 1 : 0; a.seed = g.seed;
  {
    double* dX = L.bind(a, dIn.p, dInt.p, dFlags.p, dSmp.p);
    a.st = dState.as<SliceChainState>();
    a.hyp = dHyp.as<double>(); a.sn2 = dSn2.as<double>(); a.scal = dScal.as<double>(); a.lp = dLp.as<double>();
    a.out = dOut.as<double>();
    wk.Nhyp = Nhyp; wk.moff = Ncov + Nnoise; wk.meanfun = meanfun; wk.X = dX; wk.y = a.y; wk.hyp = a.hyp; wk.sn2 = a.sn2; wk.scal = a.scal;
    wk.act = a.act; wk.on = a.on;
    long long enqueued = 0;
    auto round = [&](int checked) -> vbmc_status {
      ++enqueued;
      hipLaunchKernelGGL(k_slice_propose, dim3(W), dim3(256), 0, st, a, checked);
      VB_TRY(wk.value_path(st, W, checked));
      gp_launch_nlz_final(st, N, D, W, Nhyp, Nnoise, Nmean, meanfun, 0, 0, dX, a.y, a.hyp, wk.w.dA.as<double>(), wk.w.dal.as<double>(), a.scal, nullptr,
                          wk.w.pfd, dOut.as<double>());
      hipLaunchKernelGGL(k_slice_decide, dim3(1), dim3(64), 0, st, a, checked);
      HIP_TRY(ctx, hipGetLastError());
      return VBMC_OK;
    };
    VB_TRY(drive_rounds(ctx, "vbmc_gp_slice_sample", SLICE_CHUNK, round, dState.p, sizeof(SliceChainState), sizeof(SliceChainState), [](const char* p) {
      const SliceChainState& h = *(const SliceChainState*)p;
      return h.phase >= 2 ? Progress::finished : h.stall ? Progress::stalled : Progress::running;
    }));
    if (g.rounds) g.rounds[1] = enqueued;
  }
  SliceChainState fin;
  HIP_TRY(ctx, hipMemcpy(&fin, dState.p, sizeof(SliceChainState), hipMemcpyDeviceToHost));
  if (fin.phase == 3) {
    if (fin.err == SLICE_ERR_COLLAPSE) {
      std::vector<double> xx(Nhyp);
      HIP_TRY(ctx, hipMemcpy(xx.data(), a.xx, (size_t)Nhyp * 8, hipMemcpyDeviceToHost));
      std::string pos;
      char b[64];
      for (int i = 0; i < Nhyp && pos.size() < 300; ++i) { snprintf(b, sizeof b, " %g", xx[i]); pos += b; }
      return set_err(ctx, VBMC_ERR_INVALID, "slicesamplebnd:collapse Shrunk to current position and proposal still not acceptable. Current position:%s. "
                     "Log f: (new value) %g, (target value) %g.", pos.c_str(), fin.err_newval, fin.log_uprime);
    }
    if (fin.err == SLICE_ERR_X0)
      return set_err(ctx, VBMC_ERR_INVALID, "slicesamplebnd:start The initial starting point X0 needs to evaluate to a real number (not Inf or NaN).");
    return set_err(ctx, VBMC_ERR_INVALID, "vbmc_gp_slice_sample: uniform block exhausted: a coordinate of sweep %d needed more than Kmax = %d shrink proposals",
                   fin.sweep, g.Kmax);
  }
  if (fin.phase != 2) return set_err(ctx, VBMC_ERR_HIP, "vbmc_gp_slice_sample: the chain did not finish (phase %d)", fin.phase);
  if (g.samples) HIP_TRY(ctx, hipMemcpy(g.samples, a.samples, (size_t)g.Ns * Nhyp * 8, hipMemcpyDeviceToHost));
  if (g.logp) HIP_TRY(ctx, hipMemcpy(g.logp, a.logp, (size_t)g.Ns * 8, hipMemcpyDeviceToHost));
  if (g.widths_out) HIP_TRY(ctx, hipMemcpy(g.widths_out, a.widths, (size_t)Nhyp * 8, hipMemcpyDeviceToHost));
  if (g.funccount) *g.funccount = fin.funccount;
  if (g.performed) *g.performed = fin.performed;
  if (g.max_shrink) *g.max_shrink = fin.maxshrink;
  if (g.rounds) g.rounds[0] = fin.rounds;
  return VBMC_OK;
}

// ------------------------------------------------------------------------------------------
// vbmc_gp_train_optimize: the optimisation half of gplite_train (gplite_train.m:200-306, fminfill.m:101-114) resident on the device
// (trainopt_kernels.h).  The fill stage is a handful of checked value-only passes over chunks of the design; the optimiser is a
// chain of ROUNDS (propose, the value + gradient path of gplite_nlZ for Nopts x W candidates, decide) enqueued in chunks, the Nopts
// progress words read one chunk behind the one being enqueued, as in vbmc_gp_slice_sample.
#define TOPT_DEFAULT_W 1   // profiles/gp_train_optimize.md: what has been measured for W = 1 / 2 / 4
#define TOPT_CHUNK 16
#define TOPT_FILL_CHUNK 256
#define TOPT_MAXINIT 16384

extern "C" vbmc_status vbmc_gp_train_optimize(vbmc_ctx* ctx, const vbmc_gptrain_args* args) {
  if (!ctx) return VBMC_ERR_INVALID;
  if (!args || args->struct_size != sizeof(vbmc_gptrain_args)) return set_err(ctx, VBMC_ERR_INVALID, "vbmc_gp_train_optimize: struct_size mismatch");
  const vbmc_gptrain_args& g = *args;
  const int N = g.N, D = g.D, Nhyp = g.Nhyp, meanfun = g.meanfun, Nopts = g.Nopts;
  if (N <= 0 || D <= 0 || !g.X || !g.y || !g.LB || !g.UB || !g.design) return set_err(ctx, VBMC_ERR_INVALID, "vbmc_gp_train_optimize: bad arguments");
  GpModel gm;
  VB_TRY(gp_noise_range_check(ctx, g.noisefun));
  VB_TRY(gp_model_check(ctx, "gplite_nlZ", N, D, Nhyp, meanfun, g.noisefun, g.Ncov, gm));
  const int Ncov = gm.Ncov, Nnoise = gm.Nnoise, Nmean = gm.Nmean;
  if (Nhyp > TOPT_MAXHYP) return set_err(ctx, VBMC_ERR_UNSUPPORTED, "Nhyp = %d > %d not accelerated", Nhyp, TOPT_MAXHYP);
  if (Nopts < 1 || Nopts > TOPT_MAXOPTS) return set_err(ctx, VBMC_ERR_UNSUPPORTED, "Nopts = %d outside 1 .. %d", Nopts, TOPT_MAXOPTS);
  if (g.W < 0 || g.W > TOPT_MAXW) return set_err(ctx, VBMC_ERR_INVALID, "vbmc_gp_train_optimize: speculation width W = %d outside 0 .. %d", g.W, TOPT_MAXW);
  const bool fill = g.Ninit > 0;
  const int Nrows = fill ? g.Ninit : g.N0;
  if (g.Ninit < 0 || Nrows < Nopts)
    return set_err(ctx, VBMC_ERR_INVALID, "vbmc_gp_train_optimize: the design has %d rows, Nopts = %d starts need at least as many", Nrows, Nopts);
  // (k_topt_fill_sort ranks the fill values with Ninit^2 comparisons in one workgroup: 16 times the reference's default design, no more)
  if (Nrows > TOPT_MAXINIT) return set_err(ctx, VBMC_ERR_UNSUPPORTED, "Ninit = %d > %d not accelerated", Nrows, TOPT_MAXINIT);
  if ((size_t)Nopts * N * N * 8 > ((size_t)2 << 30))
    return set_err(ctx, VBMC_ERR_UNSUPPORTED, "Nopts = %d starts of N = %d: the lock-step work matrices would pass 2 GiB", Nopts, N);
  if (!(g.TolFun >= 0.0)) return set_err(ctx, VBMC_ERR_INVALID, "vbmc_gp_train_optimize: TolFun must be non-negative");
  if (g.prior_mu && !g.prior_sigma) return set_err(ctx, VBMC_ERR_INVALID, "vbmc_gp_train_optimize: prior_mu without prior_sigma");
  if (g.hist_cap < 0 || ((g.hist_x || g.hist_f || g.hist_k) && !(g.hist_x && g.hist_f && g.hist_k && g.hist_cap > 0)))
    return set_err(ctx, VBMC_ERR_INVALID, "vbmc_gp_train_optimize: the history needs hist_x, hist_f, hist_k and hist_cap > 0");
  for (int i = 0; i < Nhyp; ++i) {
    const double lb = g.LB[i], ub = g.UB[i];
    if (lb != lb || ub != ub || !(ub >= lb))
      return set_err(ctx, VBMC_ERR_INVALID, "vbmc_gp_train_optimize: all upper bounds UB need to be equal or greater than lower bounds LB.");
  }
  for (size_t e = 0; e < (size_t)Nrows * Nhyp; ++e)
    if (!std::isfinite(g.design[e])) return set_err(ctx, VBMC_ERR_INVALID, "vbmc_gp_train_optimize: the design holds a value that is not finite");
  const HyperPrior pr(g.prior_mu, g.prior_sigma, g.prior_df, Nhyp);
  int W = g.W == 0 ? TOPT_DEFAULT_W : g.W;
  while (W > 1 && (size_t)Nopts * W * N * N * 8 > ((size_t)2 << 30)) --W;     // each of the three work matrices per candidate stays below 2 GiB
  const int B = Nopts * W;
  const int CH = (int)std::max<size_t>(1, std::min<size_t>(std::min<size_t>(Nrows, TOPT_FILL_CHUNK), ((size_t)2 << 30) / ((size_t)N * N * 8)));
  const int BB = std::max(B, CH);
  const int hist_cap = g.hist_f ? g.hist_cap : 0;

  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const ToptBlocks L(N, D, Nhyp, g.s2 != nullptr, Nrows, Nopts, BB, hist_cap);
  const int nt1 = (N + NLZ_T - 1) / NLZ_T, ntile = nt1 * nt1, P = D + 1 + Nnoise;
  TmpBuf dIn, dInt, dState, dVec, dH, dHyp, dSn2, dDs, dScal, dLp, dFlags, dCode, dOut, dKi, dTT, dPart, dFill, dRes, dHist;
  GpObjWork wk;
  HIP_TRY(ctx, dIn.alloc(ctx, L.in.bytes()));
  HIP_TRY(ctx, dInt.alloc(ctx, L.ints.bytes()));
  HIP_TRY(ctx, dState.alloc(ctx, (size_t)Nopts * sizeof(ToptStart)));
  HIP_TRY(ctx, dVec.alloc(ctx, L.vec.bytes()));
  HIP_TRY(ctx, dH.alloc(ctx, (size_t)Nopts * Nhyp * Nhyp * 8));
  HIP_TRY(ctx, dHyp.alloc(ctx, (size_t)BB * Nhyp * 8));
  HIP_TRY(ctx, dSn2.alloc(ctx, (size_t)BB * N * 8));
  HIP_TRY(ctx, dDs.alloc(ctx, (size_t)BB * std::max(Nnoise, 1) * N * 8));
  HIP_TRY(ctx, dScal.alloc(ctx, (size_t)BB * 4 * 8));
  HIP_TRY(ctx, dLp.alloc(ctx, L.lp.bytes()));
  HIP_TRY(ctx, dFlags.alloc(ctx, L.flags.bytes()));
  HIP_TRY(ctx, dCode.alloc(ctx, (size_t)BB * sizeof(int)));
  VB_TRY(wk.alloc(ctx, N, D, BB));
  HIP_TRY(ctx, dOut.alloc(ctx, (size_t)BB * (2 + Nhyp) * 8));
  HIP_TRY(ctx, dKi.alloc(ctx, (size_t)B * N * N * 8));
  HIP_TRY(ctx, dTT.alloc(ctx, (size_t)B * N * N * 8));
  HIP_TRY(ctx, dPart.alloc(ctx, (size_t)B * ntile * P * 8));
  HIP_TRY(ctx, dFill.alloc(ctx, L.fill.bytes()));
  HIP_TRY(ctx, dRes.alloc(ctx, L.res.bytes()));
  HIP_TRY(ctx, dHist.alloc(ctx, L.hist.bytes()));
  VB_TRY(ensure_pin(ctx, 2 * (size_t)TOPT_MAXOPTS * sizeof(ToptStart) + 64));    // two landing slots of the progress words

  std::vector<double> hin(L.in.count(), 0.0);
  L.head.pack(hin.data(), g.X, g.y, g.s2);
  L.LB.put(hin.data(), g.LB); L.UB.put(hin.data(), g.UB);
  L.prior.pack(hin.data(), pr.pmu.data(), pr.psig.data(), pr.pdf.data(), pr.pc.data());
  L.design.put(hin.data(), g.design);
  HIP_TRY(ctx, hipMemcpyAsync(dIn.p, hin.data(), L.in.bytes(), hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(L.ptype.at(dInt.p), pr.ptype.data(), L.ptype.size(), hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemsetAsync(dState.p, 0, (size_t)Nopts * sizeof(ToptStart), st));
  HIP_TRY(ctx, hipMemsetAsync(dVec.p, 0, L.vec.bytes(), st));
  HIP_TRY(ctx, hipMemsetAsync(dFlags.p, 0, L.flags.bytes(), st));
  HIP_TRY(ctx, hipMemsetAsync(dHyp.p, 0, (size_t)BB * Nhyp * 8, st));       // k_gp_scale / k_nlz_grad / k_nlz_final are not gated: they read every row
  HIP_TRY(ctx, hipMemsetAsync(dScal.p, 0, (size_t)BB * 4 * 8, st));
  HIP_TRY(ctx, hipMemsetAsync(dDs.p, 0, (size_t)BB * std::max(Nnoise, 1) * N * 8, st));
  HIP_TRY(ctx, hipMemsetAsync(wk.w.dal.p, 0, ((size_t)BB * N + BB) * 8, st));
  HIP_TRY(ctx, hipMemsetAsync(dKi.p, 0, (size_t)B * N * N * 8, st));
  HIP_TRY(ctx, hipMemsetAsync(dHist.p, 0, L.hist.bytes(), st));
  HIP_TRY(ctx, hipMemsetAsync(L.order.at(dInt.p), 0, L.ints.bytes() - L.order.off, st));   // everything behind ptype

  ToptArgs a{};
  a.N = N; a.D = D; a.Nhyp = Nhyp; a.Ncov = Ncov; a.Nnoise = Nnoise; a.Nopts = Nopts; a.W = W; a.Ninit = Nrows;
  a.nf0 = g.noisefun[0]; a.nf1 = g.noisefun[1]; a.nf2 = g.noisefun[2]; a.has_prior = g.prior_mu ? 1 : 0;
  a.max_iter = g.MaxIter > 0 ? g.MaxIter : 1000; a.max_evals = g.MaxFunEvals > 0 ? g.MaxFunEvals : 3000; a.hist_cap = hist_cap;
  a.lownoise = fill ? 1 : 0; a.tol = g.TolFun;
  double* dX = L.bind(a, dIn.p, dInt.p, dVec.p, dLp.p, dFlags.p, dFill.p, dRes.p, dHist.p);
  a.st = dState.as<ToptStart>();
  a.H = dH.as<double>();
  a.hyp = dHyp.as<double>(); a.sn2 = dSn2.as<double>(); a.scal = dScal.as<double>();
  a.dsn2 = dDs.as<double>(); a.code = dCode.as<int>(); a.out = dOut.as<double>();
  wk.Nhyp = Nhyp; wk.moff = Ncov + Nnoise; wk.meanfun = meanfun; wk.X = dX; wk.y = a.y; wk.hyp = a.hyp; wk.sn2 = a.sn2; wk.scal = a.scal;
  wk.act = a.act; wk.on = a.on;
  // the tile form of the inverse's rank-k product is fixed by Nopts and N, not by W: every W computes the same bits
  const int syrk_form = (size_t)Nopts * ((N + 63) / 64) * ((N + 63) / 64 + 1) / 2 <= 128 ? 1 : 2;

  // 1. fill
  for (int c0 = 0; c0 < Nrows; c0 += CH) {
    const int n = std::min(CH, Nrows - c0);
    hipLaunchKernelGGL(k_topt_propose, dim3(n), dim3(256), 0, st, a, 1, c0, 1);
    VB_TRY(wk.value_path(st, n, 1));
    gp_launch_nlz_final(st, N, D, n, Nhyp, Nnoise, Nmean, meanfun, 0, 0, dX, a.y, a.hyp, wk.w.dA.as<double>(), wk.w.dal.as<double>(), a.scal, nullptr,
                        wk.w.pfd, dOut.as<double>());
    hipLaunchKernelGGL(k_topt_fill_collect, dim3((n + 255) / 256), dim3(256), 0, st, a, n, c0);
    HIP_TRY(ctx, hipGetLastError());
  }
  // 2. starts
  hipLaunchKernelGGL(k_topt_fill_sort, dim3(1), dim3(256), 0, st, a);
  HIP_TRY(ctx, hipMemsetAsync(dFlags.p, 0, L.flags.bytes(), st));
  HIP_TRY(ctx, hipGetLastError());
  // 3. optimiser
  // (a start that is done and a candidate that is never consumed launch nothing in propose / build / factorise / solve / inverse /
  // decide, but k_gp_scale, k_nlz_grad and k_nlz_final have no activity flag -- vbmc_gp_nlz shares them -- and still run on those
  // rows: N^2 D work per idle candidate and round, paid from the moment the first of several starts finishes until the last does)
  auto round = [&](int checked) -> vbmc_status {
    hipLaunchKernelGGL(k_topt_propose, dim3(B), dim3(256), 0, st, a, 0, 0, checked);
    VB_TRY(wk.value_path(st, B, checked));
    VB_TRY(gp_launch_grad(ctx, st, N, D, B, Nhyp, Nnoise, a.hyp, a.scal, a.on, a.dsn2, wk.w, dTT.as<double>(), dKi.as<double>(), dPart.as<double>(), false,
                          syrk_form, nullptr));
    gp_launch_nlz_final(st, N, D, B, Nhyp, Nnoise, Nmean, meanfun, ntile, 1, dX, a.y, a.hyp, wk.w.dA.as<double>(), wk.w.dal.as<double>(), a.scal,
                        dPart.as<double>(), wk.w.pfd, dOut.as<double>());
    hipLaunchKernelGGL(k_topt_decide, dim3(Nopts), dim3(64), 0, st, a, checked);
    HIP_TRY(ctx, hipGetLastError());
    return VBMC_OK;
  };
  VB_TRY(drive_rounds(ctx, "vbmc_gp_train_optimize", TOPT_CHUNK, round, dState.p, (size_t)Nopts * sizeof(ToptStart),
                      (size_t)TOPT_MAXOPTS * sizeof(ToptStart), [Nopts](const char* p) {
    const ToptStart* h = (const ToptStart*)p;
    bool all_done = true, stalled = false;
    for (int s = 0; s < Nopts; ++s) { all_done = all_done && h[s].done; stalled = stalled || h[s].stall; }
    return all_done ? Progress::finished : stalled ? Progress::stalled : Progress::running;
  }));
  // 4. closing
  hipLaunchKernelGGL(k_topt_close, dim3(1), dim3(64), 0, st, a);
  HIP_TRY(ctx, hipGetLastError());
  std::vector<ToptStart> fin(Nopts);
  HIP_TRY(ctx, hipMemcpy(fin.data(), dState.p, (size_t)Nopts * sizeof(ToptStart), hipMemcpyDeviceToHost));
  for (int s = 0; s < Nopts; ++s)
    if (!fin[s].done) return set_err(ctx, VBMC_ERR_HIP, "vbmc_gp_train_optimize: start %d did not finish", s);
  if (g.fill_fvals) HIP_TRY(ctx, hipMemcpy(g.fill_fvals, a.fsorted, (size_t)Nrows * 8, hipMemcpyDeviceToHost));
  if (g.fill_order) HIP_TRY(ctx, hipMemcpy(g.fill_order, a.order, (size_t)Nrows * sizeof(int), hipMemcpyDeviceToHost));
  if (g.widths_default && fill) HIP_TRY(ctx, hipMemcpy(g.widths_default, a.widths, (size_t)Nhyp * 8, hipMemcpyDeviceToHost));
  if (g.hyp) HIP_TRY(ctx, hipMemcpy(g.hyp, a.x, (size_t)Nopts * Nhyp * 8, hipMemcpyDeviceToHost));
  if (g.nll) HIP_TRY(ctx, hipMemcpy(g.nll, a.res_nll, (size_t)Nopts * 8, hipMemcpyDeviceToHost));
  if (g.best) HIP_TRY(ctx, hipMemcpy(g.best, a.best, sizeof(int), hipMemcpyDeviceToHost));
  if (g.hyp_start) HIP_TRY(ctx, hipMemcpy(g.hyp_start, a.hyp_start, (size_t)Nhyp * 8, hipMemcpyDeviceToHost));
  if (hist_cap) {
    HIP_TRY(ctx, hipMemcpy(g.hist_f, a.hist_f, (size_t)Nopts * hist_cap * 8, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(g.hist_x, a.hist_x, (size_t)Nopts * hist_cap * Nhyp * 8, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(g.hist_k, a.hist_k, (size_t)Nopts * hist_cap * sizeof(int), hipMemcpyDeviceToHost));
  }
  long long performed = 0;
  for (int s = 0; s < Nopts; ++s) {
    if (g.iterations) g.iterations[s] = fin[s].iterations;
    if (g.funccount) g.funccount[s] = fin[s].funccount;
    if (g.exitflag) g.exitflag[s] = fin[s].exitflag;
    performed += fin[s].performed;
  }
  if (g.performed) *g.performed = performed;
  return VBMC_OK;
}

// vbmc_hip_mex.cpp -- MEX gateway from MATLAB to libvbmc_hip.so (include/vbmc_hip.h).
//
// Build (on a machine with MATLAB + ROCm; cannot be built in the development container, which has
// neither MATLAB nor mex.h -- this file is deliberately free of numerics):
//     mex -R2018a vbmc_hip_mex.cpp -I../include -L../vbmc_amd/lib -lvbmc_hip
//
// Usage from the .m shims in this directory:
//     vbmc_hip_mex('open', device)                         -> (context kept in a persistent, mexLock'ed)
//     h  = vbmc_hip_mex('gp_upload', gpstruct)             -> uint64 handle of a device-resident gp.post
//          vbmc_hip_mex('gp_free', h)
//     [F,dF,G,H,varG,dH,varGss,I_sk,J_sjk,dG,G_s,varG_s,dvarG,dG_s,dvarG_s] = vbmc_hip_mex('elbo', h, theta, vp, Ns, compute_grad,
//                                     compute_var, separate_K, beta, thetabnd_or_empty, eps_or_empty, seed, numel(gp.post), no_jacobian)
//                                     (G_s, varG_s, dG_s (T x S): the per-hyper-sample outputs of gplogjoint(...,avg_flag = 0); no_jacobian,
//                                     optional: 1 = gradients with respect to sigma, lambda, w themselves, the JACOBIAN_FLAG = 0
//                                     form of entmc_vbmc / entlb_vbmc / gplogjoint)
//     [F,dF,varG,G,H,varGss,I_sk,J_sjk] = vbmc_hip_mex('elbo_batch', h, Theta /*T x R*/, vp, Ns, compute_grad, compute_var, beta,
//                                thetabnd_or_empty, seed, separate_K, numel(gp.post))
//                                (the R candidates of vpsieve_vbmc.m:74-78, or the 2*Nslowopts eval_fullelcbo calls of
//                                 vpoptimize_vbmc.m:134,165, in one pass; I_sk is S x K x R, J_sjk S x K x K x R)
//     [x,f,iters,xmid,xtab,ftab] = vbmc_hip_mex('adam', h, Theta0 /*T x R*/, vp, Ns, compute_var, beta, thetabnd_or_empty, seed,
//                                TolFun, MaxIter, [step_min step_max step_decay])   (fminadam.m on the device; xmid T x R: each
//                                chain's iterate of smallest recorded objective, vpoptimize_vbmc.m:133; the tables only on
//                                request: xtab T x MaxIter x R, ftab MaxIter x R, the first iters(r) entries of chain r filled)
//     [alpha,L,sW,sn2_mult,Lchol,h] = vbmc_hip_mex('gp_post', hyp, X, y, s2, meanfun, noisefun)
//     [ymu,ys2,fmu,fs2] = vbmc_hip_mex('gp_pred', h, Xstar, s2star, ssflag)
//     [acq,fbar,vtot] = vbmc_hip_mex('acq', h, Xs, acq_id, vp, ymax, var_regularized, TolGPVar, gplengthscale, X_rescaled, sn2new)
//     [acq,fbar,vtot] = vbmc_hip_mex('acq_delta', h, Xs, acq_id, vp, ymax, var_regularized, TolGPVar, delta, gplengthscale, X_rescaled, sn2new)
//                                ('acq' with vp.delta > 0: mean and variance per hyper-sample from gplite_quad(gp,Xs,delta,1),
//                                 acqwrapper_vbmc.m:12-14; delta: D values; the last three only for acqfsn2)
//     [F,varF] = vbmc_hip_mex('gp_quad', h, mu, sigma, ssflag, numel(gp.post))   (gplite_quad: sigma 1 x D, or Nstar x D of equal rows)
//     [xmin,fmin,out] = vbmc_hip_mex('acq_search', h, acq_id, vp, ymax, var_regularized, TolGPVar, x0, insigma, LB, UB, opts, gplengthscale, X_rescaled, sn2new)
//                                                  (the CMA-ES acquisition search on the device: matlab/vbmc_hip_acqsearch.m)
//     [xmin,fmin,out] = vbmc_hip_mex('acq_search_iqr', h, his, acq_id, vp, var_regularized, TolGPVar, x0, insigma, LB, UB, opts, gplengthscale, X_rescaled, sn2new)
//     his = vbmc_hip_mex('is_create', h, Xa, lnw_or_empty, fs2a_or_empty, Ctmp_or_empty)   (ActiveImportanceSampling state)
//     [Xa,lnw,fs2a,his,out] = vbmc_hip_mex('acq_is_sample', h, x0 /*W x D x S*/, LB, UB, Nm, opts)
//                                (the MCMC of the IMIQR importance sampler on the device: vbmc_acq_is_sample, matlab/vbmc_hip_importance_sample.m.
//                                 opts: Thin, Burnin, Spec, MaxSteps, MaxShrink, Seed, Chunk, U (64 x H x S x Mmax: parity mode); out: logp,
//                                 funccount, performed, rounds, behind; his: the state of those device buffers, freed with 'is_free')
//     [Xa,lnw,fs2a,his,out] = vbmc_hip_mex('is_setup', h, vp, Nvp, Nbox, Nm, opts)
//                                (the whole set-up of the IMIQR importance sampler in one call: vbmc_acq_is_setup, matlab/vbmc_hip_importance_setup.m.
//                                 opts: Thin, Burnin, Spec, MaxSteps, MaxShrink, Seed, Chunk, W (0: 2 (D + 1)), B (the Step 1 block: parity mode),
//                                 U (64 x H x S x Mmax, with B); out: Xa1, lnw1, fs2a1, lpdf1, rect_delta, LB, UB, x0 (W x D x S), idx0 (W x S,
//                                 0-based), n_bad, bad (W x S), logp, funccount, performed, rounds, behind; n_bad > 0: Xa, lnw, fs2a are zeros
//                                 and his is 0; Nm = 0: Step 1 alone, his the state of the Na1 shared points)
//           vbmc_hip_mex('is_free', his)
//     [y,dy] = vbmc_hip_mex('vp_pdf', vp, X, origflag, logflag, transflag, df)        (vbmc_pdf through vp.trinfo: vbmc_vp_pdf, matlab/vbmc_hip_pdf.m)
//     [X,I] = vbmc_hip_mex('vp_rnd', vp, N, origflag, balanceflag, df, seed)          (vbmc_rnd, I counted from 0: vbmc_vp_rnd, matlab/vbmc_hip_rnd.m)
//     [mubar,Sigma] = vbmc_hip_mex('vp_moments', vp, Ns, seed)                        (vbmc_moments(vp,1,Ns): vbmc_vp_moments, matlab/vbmc_hip_moments.m)
//     [kls,xx1,xx2] = vbmc_hip_mex('vp_kldiv', vp1, vp2, Ns, seed)                    (vbmc_kldiv(vp1,vp2,Ns,0): vbmc_vp_kldiv, matlab/vbmc_hip_kldiv.m)
//     [mtv,xx1,xx2] = vbmc_hip_mex('vp_mtv', vp1, vp2, Ns, seed)                      (vbmc_mtv(vp1,vp2,Ns): vbmc_vp_mtv, matlab/vbmc_hip_mtv.m)
//     [kl_mat,maxmtv_mat,mtv,xx] = vbmc_hip_mex('vp_diag', Ns, seed, vp1, vp2, ...)   (the pair loop of vbmc_diagnostics: vbmc_vp_diagnostics, matlab/vbmc_hip_diagnostics.m)
//     [acq,fbar,vtot] = vbmc_hip_mex('acq_iqr', h, his, Xs, gplengthscale, X_rescaled, sn2new, var_regularized, TolGPVar)
//     [X,out] = vbmc_hip_mex('gp_surrogate_sample', h, vp, Ns, origflag, LB, UB, noise /*struct X_rescaled, gplengthscale, sn2new or []*/, opts)
//                                (gpsample_vbmc(vp,gp,Ns,origflag): vbmc_gp_surrogate_sample, matlab/gpsample_vbmc.m.  opts: S, E, W, Seed, Thin,
//                                 Burnin, Spec, Chunk, Nnn, Beta, VarThresh, x0 (W x D x E); out: VarThresh, sn2_avg, funccount, performed, rounds, behind)
//     [nlZ,dnlZ] = vbmc_hip_mex('gp_nlz', Hyp /*Nhyp x B*/, X, y, s2, meanfun, noisefun)   (gplite_nlZ for B vectors)
//     [samples,logp,widths,counts] = vbmc_hip_mex('slice_sample', X, y, s2, meanfun, noisefun, prior /*struct mu, sigma, df or []*/, LB, UB,
//                                hyp_start, widths, basewidths_or_empty, [Ns Thin Burnin Adaptive W], seed, perms_or_empty, U_or_empty)
//                                (slicesamplebnd on -gplite_nlZ + log prior, the chain on the device: vbmc_gp_slice_sample.  perms:
//                                 Nhyp x sweeps, column s = randperm(Nhyp)' of sweep s, 1-based; U: (2+Kmax) x Nhyp x sweeps; both
//                                 empty: the device generator keyed by seed.  counts = [funccount performed max_shrink])
//     [hyp,nll,hyp_start,best,widths_default,counts,performed,fill_fvals,fill_order] = vbmc_hip_mex('gp_train_opt', X, y, s2, meanfun,
//                                noisefun, prior /*struct mu, sigma, df or []*/, LB, UB, design /*rows x Nhyp*/,
//                                [Ninit Nopts TolFun MaxIter MaxFunEvals W])
//                                (the optimisation half of gplite_train, gplite_train.m:200-306, on the device: vbmc_gp_train_optimize.
//                                 design: the points fminfill evaluates, hyp0' in its first rows -- the caller builds it, fminfill.m:42-101;
//                                 Ninit = 0: the rows are the caller's hyp0 alone (:249-256) and widths_default comes back NaN.
//                                 hyp Nhyp x Nopts, counts 3 x Nopts = [iterations; funccount; exitflag], best and fill_order 1-based)
//     C = vbmc_hip_mex('sq_dist', a, b)
//     lim = vbmc_hip_mex('limits')                          -> struct max_D, max_K, max_N, max_Na, max_T_vargrad, delta_ok, meanfun: the shapes the
//                                                             library accepts (vbmc_get_limits; no device needed) -- matlab/vbmc_hip_supported.m
//     n3 = vbmc_hip_mex('stats')                            -> [host uploads of a surrogate, device posteriors kept, rank-one appends kept]
// Every GPU of the node from ONE MATLAB process (the communicator inside the library, include/vbmc_hip.h):
//     n  = vbmc_hip_mex('comm_open', ndev)                 -> must be the first command of the session: a context and an RCCL rank
//                                                             per device; the single-device commands then run on device 0.
//                                                             VBMC_HIP_DEVICES=ndev in the environment does the same implicitly.
//     n  = vbmc_hip_mex('comm_size')                       -> devices of the session (1 without a communicator)
//     hs = vbmc_hip_mex('gp_upload_all', gpstruct)         -> 1 x n uint64 handles, one replica per device (hs(1): device 0)
//          vbmc_hip_mex('gp_free_all', hs)
//     [F,dF,varG,G,H,varGss,I_sk,J_sjk] = vbmc_hip_mex('elbo_batch_multi', hs, Theta, vp, Ns, compute_grad, compute_var, beta,
//                                thetabnd_or_empty, seed, separate_K, numel(gp.post))
//                                ('elbo_batch' with the R candidates dealt r = g (mod n) over the devices and their ELCBO values
//                                 all-gathered over xGMI; every value bit-identical to 'elbo_batch' on one device)
//
// Errors: mexErrMsgIdAndTxt long-jumps out of the MEX function without running C++ destructors, so it is called from
// exactly one place -- mexFunction itself, which owns no C++ object -- after dispatch() has RETURNED (all its
// std::vector / std::string temporaries destroyed) with the id and message parked in static character buffers.
// VBMC_ERR_UNSUPPORTED becomes the id 'vbmc_hip:unsupported' which the shims catch to fall through
// to the reference .m implementation (SURVEY.md 8b "Errors").
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "mex.h"
#include "vbmc_hip.h"

static vbmc_ctx* g_ctx = nullptr;
static long long g_stats[3] = {0, 0, 0};   // 'stats': gp_upload(_all) commands, gp_post handles kept, gp_rank1 appends
static vbmc_comm* g_comm = nullptr;   // 'comm_open': owns one context per device; g_ctx is then its device-0 context

static void at_exit() {
  if (g_comm) { vbmc_comm_destroy(g_comm); g_comm = nullptr; g_ctx = nullptr; }
  if (g_ctx) { vbmc_ctx_destroy(g_ctx); g_ctx = nullptr; }
}

// pending error of the current call (plain static storage: survives the long jump, owns nothing)
static char g_err_id[96];
static char g_err_msg[640];

static int raise(const char* id, const char* msg) {
  snprintf(g_err_id, sizeof g_err_id, "%s", id);
  snprintf(g_err_msg, sizeof g_err_msg, "%s", msg);
  return 1;
}

// library status -> pending MATLAB error; returns nonzero so that call sites read `if (st != VBMC_OK) return fail(st);`
static int fail(vbmc_status st) {
  const char* msg = g_ctx ? vbmc_last_error(g_ctx) : "no context";
  if (st == VBMC_ERR_UNSUPPORTED) return raise("vbmc_hip:unsupported", msg);
  // messages of INVALID errors start with the reference's own error id where one exists ("gplogjoint:FullVarianceGradient ...")
  const char* sp = strchr(msg, ' ');
  const char* col = strchr(msg, ':');
  if (st == VBMC_ERR_INVALID && sp && col && col < sp && (size_t)(sp - msg) < sizeof g_err_id) {
    memcpy(g_err_id, msg, (size_t)(sp - msg));
    g_err_id[sp - msg] = 0;
    snprintf(g_err_msg, sizeof g_err_msg, "%s", sp + 1);
    return 1;
  }
  return raise("vbmc_hip:error", msg);
}

// status of a communicator call -> pending MATLAB error
static int fail_comm(vbmc_status st) {
  const char* msg = g_comm ? vbmc_comm_last_error(g_comm) : "no communicator";
  return raise(st == VBMC_ERR_UNSUPPORTED ? "vbmc_hip:unsupported" : "vbmc_hip:error", msg);
}

static int ensure_ctx(int device) {
  if (g_ctx) return 0;
  // VBMC_HIP_DEVICES=n (n >= 2) in the environment: the session opens on n devices, as 'comm_open' n would
  const char* nd = getenv("VBMC_HIP_DEVICES");
  if (nd && atoi(nd) >= 2) {
    vbmc_status st = vbmc_comm_create_all(atoi(nd), nullptr, &g_comm);
    if (st != VBMC_OK) { g_comm = nullptr; return raise("vbmc_hip:nodevice", "libvbmc_hip: VBMC_HIP_DEVICES asks for more gfx950 devices than could be opened (or librccl is missing)"); }
    g_ctx = vbmc_comm_ctx(g_comm, 0);
    mexLock();
    mexAtExit(at_exit);
    return 0;
  }
  vbmc_status st = vbmc_ctx_create(device, nullptr, &g_ctx);
  if (st != VBMC_OK) return raise("vbmc_hip:nodevice", "libvbmc_hip: no gfx950 (MI355X) device available");
  mexLock();
  mexAtExit(at_exit);
  return 0;
}

// device handles travel as uint64 scalars; anything else (a double that lost its class on the way) must not be dereferenced
static bool is_handle(const mxArray* a) { return a && mxGetClassID(a) == mxUINT64_CLASS && mxGetNumberOfElements(a) >= 1; }
static const double* dbl(const mxArray* a) { return (a && !mxIsEmpty(a)) ? mxGetDoubles(a) : nullptr; }
static const mxArray* field(const mxArray* s, const char* name) { return mxGetField(s, 0, name); }
static double scalar_field(const mxArray* s, const char* name, double dflt) {
  const mxArray* f = field(s, name);
  return (f && !mxIsEmpty(f)) ? mxGetScalar(f) : dflt;
}

// vp struct + thetabnd -> the parameter-layout part of vbmc_elbo_args (shared by 'elbo', 'elbo_batch', 'adam').  Returns nonzero with a
// pending 'vbmc_hip:unsupported' error for a vp.delta that is neither a scalar nor a D-vector (the reference cannot evaluate it either)
static int fill_vp_args(vbmc_elbo_args& a, const mxArray* vp, const mxArray* tb, std::vector<double>& delta) {
  memset(&a, 0, sizeof a);
  a.struct_size = sizeof a;
  a.D = (int)scalar_field(vp, "D", 0); a.K = (int)scalar_field(vp, "K", 0); a.R = 1;
  a.optimize[0] = scalar_field(vp, "optimize_mu", 1) != 0; a.optimize[1] = scalar_field(vp, "optimize_sigma", 1) != 0;
  a.optimize[2] = scalar_field(vp, "optimize_lambda", 1) != 0; a.optimize[3] = scalar_field(vp, "optimize_weights", 0) != 0;
  a.vp_mu = dbl(field(vp, "mu")); a.vp_sigma = dbl(field(vp, "sigma")); a.vp_lambda = dbl(field(vp, "lambda")); a.vp_w = dbl(field(vp, "w"));
  const mxArray* dl = field(vp, "delta");
  if (dl && !mxIsEmpty(dl)) {  // scalar or D-vector (gplogjoint.m:85-89)
    const size_t nd = mxGetNumberOfElements(dl);
    if (nd != 1 && nd != (size_t)a.D) return raise("vbmc_hip:unsupported", "vp.delta has neither one entry nor D");
    delta.assign(a.D, mxGetDoubles(dl)[0]);
    if (nd == (size_t)a.D) memcpy(delta.data(), mxGetDoubles(dl), a.D * sizeof(double));
    a.vp_delta = delta.data();
  }
  if (tb && !mxIsEmpty(tb)) {
    a.bnd_lb = dbl(field(tb, "lb")); a.bnd_ub = dbl(field(tb, "ub")); a.TolCon = scalar_field(tb, "TolCon", 0.01);
    a.WeightThreshold = scalar_field(tb, "WeightThreshold", 0); a.WeightPenalty = scalar_field(tb, "WeightPenalty", 0);
  }
  { const char* sc = getenv("VBMC_HIP_SPARSE_CUTOFF"); a.sparse_cutoff = sc ? atof(sc) : 0.0; }
  return 0;
}

// gp struct (gplite_post.m:94-157) -> the flat arrays of vbmc_gp_upload; returns the sizes
struct GpArrays {
  int N = 0, D = 0, S = 0, Nhyp = 0, Ncov = 0, Nnoise = 0, meanfun = 0;
  const double* X = nullptr;
  std::vector<double> hyp, alpha, L, sW1, mult;
  std::vector<uint8_t> lch;
  int32_t nf[3] = {1, 0, 0};
};
static void read_gp(const mxArray* gp, GpArrays& g) {
  const mxArray* X = field(gp, "X");
  const mxArray* post = field(gp, "post");
  g.N = (int)mxGetM(X); g.D = (int)mxGetN(X); g.S = (int)mxGetNumberOfElements(post);
  g.Nhyp = (int)mxGetNumberOfElements(mxGetField(post, 0, "hyp"));
  g.X = mxGetDoubles(X);
  const int N = g.N, S = g.S, Nhyp = g.Nhyp;
  g.hyp.resize((size_t)Nhyp * S); g.alpha.resize((size_t)N * S); g.L.resize((size_t)N * N * S); g.sW1.resize(S); g.mult.resize(S);
  g.lch.resize(S);
  for (int s = 0; s < S; ++s) {
    memcpy(&g.hyp[(size_t)s * Nhyp], mxGetDoubles(mxGetField(post, s, "hyp")), Nhyp * sizeof(double));
    memcpy(&g.alpha[(size_t)s * N], mxGetDoubles(mxGetField(post, s, "alpha")), N * sizeof(double));
    memcpy(&g.L[(size_t)s * N * N], mxGetDoubles(mxGetField(post, s, "L")), (size_t)N * N * sizeof(double));
    g.sW1[s] = mxGetDoubles(mxGetField(post, s, "sW"))[0];
    g.mult[s] = mxGetScalar(mxGetField(post, s, "sn2_mult"));
    g.lch[s] = mxIsLogicalScalarTrue(mxGetField(post, s, "Lchol")) ? 1 : 0;
  }
  const mxArray* nfa = field(gp, "noisefun");
  for (int i = 0; nfa && i < 3 && i < (int)mxGetNumberOfElements(nfa); ++i) g.nf[i] = (int32_t)mxGetDoubles(nfa)[i];
  g.Ncov = (int)scalar_field(gp, "Ncov", g.D + 1); g.Nnoise = (int)scalar_field(gp, "Nnoise", 1);
  g.meanfun = (int)scalar_field(gp, "meanfun", 4);
}

// vp struct with its trinfo (shared/warpvars_vbmc.m: lb_orig, ub_orig, type, mu, delta, scale, R_mat; empty: the identity) -> vbmc_vp_desc
// (shared by 'vp_pdf', 'vp_rnd', 'vp_moments', 'vp_kldiv', 'vp_mtv', 'vp_diag').  The arrays stay MATLAB's; only the types are converted to int32.
static int fill_vp_desc(vbmc_vp_desc& d, const mxArray* vp, std::vector<int32_t>& types) {
  memset(&d, 0, sizeof d);
  d.struct_size = sizeof d;
  if (!vp || !mxIsStruct(vp)) return raise("vbmc_hip:usage", "vp must be a variational-posterior struct");
  const mxArray *mu = field(vp, "mu"), *sg = field(vp, "sigma"), *lm = field(vp, "lambda"), *ww = field(vp, "w");
  if (!mu || !sg || !lm || !ww || mxIsEmpty(mu)) return raise("vbmc_hip:usage", "vp needs mu, sigma, lambda and w");
  d.D = (int32_t)mxGetM(mu); d.K = (int32_t)mxGetN(mu);
  if (mxGetNumberOfElements(sg) != (size_t)d.K || mxGetNumberOfElements(ww) != (size_t)d.K || mxGetNumberOfElements(lm) != (size_t)d.D)
    return raise("vbmc_hip:usage", "vp.mu must be D x K with K sigmas and weights and D lambdas");
  d.mu = mxGetDoubles(mu); d.sigma = mxGetDoubles(sg); d.lambda = mxGetDoubles(lm); d.w = mxGetDoubles(ww);
  const mxArray* tr = field(vp, "trinfo");
  if (!tr || mxIsEmpty(tr) || !mxIsStruct(tr)) return 0;
  const mxArray *ty = field(tr, "type"), *lb = field(tr, "lb_orig"), *ub = field(tr, "ub_orig"), *tm = field(tr, "mu"), *td = field(tr, "delta");
  const mxArray *sc = field(tr, "scale"), *rm = field(tr, "R_mat");
  const size_t D = (size_t)d.D;
  for (const mxArray* a : {ty, lb, ub, tm, td})
    if (!a || mxGetNumberOfElements(a) != D) return raise("vbmc_hip:usage", "vp.trinfo needs type, lb_orig, ub_orig, mu and delta with D entries each");
  if ((sc && !mxIsEmpty(sc) && mxGetNumberOfElements(sc) != D) || (rm && !mxIsEmpty(rm) && mxGetNumberOfElements(rm) != D * D))
    return raise("vbmc_hip:usage", "vp.trinfo.scale must have D entries and vp.trinfo.R_mat D x D");
  types.resize(D);
  for (size_t i = 0; i < D; ++i) types[i] = (int32_t)mxGetDoubles(ty)[i];
  d.type = types.data(); d.lb = mxGetDoubles(lb); d.ub = mxGetDoubles(ub); d.tmu = mxGetDoubles(tm); d.tdelta = mxGetDoubles(td);
  d.scale = dbl(sc); d.R = dbl(rm);
  return 0;
}

// Every command; returns 0 on success, nonzero with g_err_id / g_err_msg set.  All C++ objects live in here.
static int dispatch(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
  if (nrhs < 1 || !mxIsChar(prhs[0])) return raise("vbmc_hip:usage", "first argument must be a command string");
  char cmd[32];
  mxGetString(prhs[0], cmd, sizeof cmd);

  if (!strcmp(cmd, "limits")) {     // the shapes the library accepts (vbmc_get_limits: a host function, no device): struct for vbmc_hip_supported.m
    vbmc_limits lim;
    lim.struct_size = sizeof lim;
    if (vbmc_get_limits(&lim) != VBMC_OK) return raise("vbmc_hip:abi", "vbmc_get_limits refused the struct (ABI mismatch)");
    const char* names[] = {"max_D", "max_K", "max_N", "max_Na", "max_T_vargrad", "delta_ok", "meanfun"};
    plhs[0] = mxCreateStructMatrix(1, 1, 7, names);
    const double v[6] = {(double)lim.max_D, (double)lim.max_K, (double)lim.max_N, (double)lim.max_Na, (double)lim.max_T_vargrad, (double)lim.delta_ok};
    for (int i = 0; i < 6; ++i) { mxArray* a = mxCreateDoubleMatrix(1, 1, mxREAL); mxGetDoubles(a)[0] = v[i]; mxSetField(plhs[0], 0, names[i], a); }
    int nm = 0;
    for (int i = 0; i < 31; ++i) nm += (lim.meanfun_mask >> i) & 1;
    mxArray* mf = mxCreateDoubleMatrix(1, nm, mxREAL);
    for (int i = 0, j = 0; i < 31; ++i) if ((lim.meanfun_mask >> i) & 1) mxGetDoubles(mf)[j++] = i;
    mxSetField(plhs[0], 0, "meanfun", mf);
    return 0;
  }
  if (!strcmp(cmd, "stats")) {      // [surrogates uploaded from the host, posteriors built on the device, rank-one appends] since the gateway was loaded
    plhs[0] = mxCreateDoubleMatrix(1, 3, mxREAL);
    for (int i = 0; i < 3; ++i) mxGetDoubles(plhs[0])[i] = (double)g_stats[i];
    return 0;
  }
  if (!strcmp(cmd, "open")) return ensure_ctx(nrhs > 1 ? (int)mxGetScalar(prhs[1]) : 0);
  if (!strcmp(cmd, "comm_open")) {
    if (g_comm || g_ctx) return raise("vbmc_hip:usage", "comm_open must be the first command of the session");
    const int ndev = nrhs > 1 ? (int)mxGetScalar(prhs[1]) : 1;
    vbmc_status st = vbmc_comm_create_all(ndev, nullptr, &g_comm);
    if (st != VBMC_OK) { g_comm = nullptr; return raise("vbmc_hip:nodevice", "libvbmc_hip: could not open the requested gfx950 devices / librccl"); }
    g_ctx = vbmc_comm_ctx(g_comm, 0);
    mexLock();
    mexAtExit(at_exit);
    plhs[0] = mxCreateDoubleMatrix(1, 1, mxREAL);
    mxGetDoubles(plhs[0])[0] = vbmc_comm_size(g_comm);
    return 0;
  }
  if (ensure_ctx(0)) return 1;
  {  // commands whose first argument is a device handle (the IQR evaluation takes two)
    const char* with_handle[] = {"gp_free", "elbo", "elbo_batch", "elbo_batch_multi", "adam", "gp_rank1", "acq", "is_create", "is_free",
                                 "acq_iqr", "gp_pred", "gp_free_all", "acq_delta", "gp_quad", "acq_search", "acq_search_iqr", "acq_is_sample", "is_setup",
                                 "gp_surrogate_sample"};
    for (const char* w : with_handle)
      if (!strcmp(cmd, w) && (nrhs < 2 || !is_handle(prhs[1]) || ((!strcmp(cmd, "acq_iqr") || !strcmp(cmd, "acq_search_iqr")) && (nrhs < 3 || !is_handle(prhs[2])))))
        return raise("vbmc_hip:usage", "this command takes a uint64 device handle as its first argument");
  }

  if (!strcmp(cmd, "gp_upload")) {
    GpArrays g;
    read_gp(prhs[1], g);
    vbmc_gp* h = nullptr;
    vbmc_status st = vbmc_gp_upload(g_ctx, g.N, g.D, g.S, g.Nhyp, g.Ncov, g.Nnoise, g.meanfun, g.X, g.hyp.data(), g.alpha.data(),
                                    g.L.data(), g.sW1.data(), g.lch.data(), &h);
    if (st == VBMC_OK) st = vbmc_gp_set_noise(g_ctx, h, g.nf, g.mult.data());
    if (st != VBMC_OK) return fail(st);
    ++g_stats[0];
    plhs[0] = mxCreateNumericMatrix(1, 1, mxUINT64_CLASS, mxREAL);
    *(uint64_t*)mxGetData(plhs[0]) = (uint64_t)(uintptr_t)h;
    return 0;
  }
  if (!strcmp(cmd, "comm_size")) { plhs[0] = mxCreateDoubleMatrix(1, 1, mxREAL); mxGetDoubles(plhs[0])[0] = g_comm ? vbmc_comm_size(g_comm) : 1; return 0; }
  if (!strcmp(cmd, "gp_upload_all")) {
    if (!g_comm) return raise("vbmc_hip:usage", "gp_upload_all needs 'comm_open' first");
    GpArrays g;
    read_gp(prhs[1], g);
    const int n = vbmc_comm_local(g_comm);
    std::vector<vbmc_gp*> hs(n, nullptr);
    vbmc_status st = vbmc_gp_upload_all(g_comm, g.N, g.D, g.S, g.Nhyp, g.Ncov, g.Nnoise, g.meanfun, g.X, g.hyp.data(), g.alpha.data(),
                                        g.L.data(), g.sW1.data(), g.lch.data(), hs.data());
    if (st != VBMC_OK) return fail_comm(st);
    for (int i = 0; i < n && st == VBMC_OK; ++i) st = vbmc_gp_set_noise(vbmc_comm_ctx(g_comm, i), hs[i], g.nf, g.mult.data());
    if (st != VBMC_OK) { vbmc_gp_free_all(g_comm, hs.data()); return raise("vbmc_hip:error", "vbmc_gp_set_noise failed on a replica"); }
    ++g_stats[0];
    plhs[0] = mxCreateNumericMatrix(1, n, mxUINT64_CLASS, mxREAL);
    for (int i = 0; i < n; ++i) ((uint64_t*)mxGetData(plhs[0]))[i] = (uint64_t)(uintptr_t)hs[i];
    return 0;
  }
  if (!strcmp(cmd, "gp_free_all")) {
    if (!g_comm) return 0;
    const int n = vbmc_comm_local(g_comm);
    std::vector<vbmc_gp*> hs(n, nullptr);
    for (int i = 0; i < n && i < (int)mxGetNumberOfElements(prhs[1]); ++i) hs[i] = (vbmc_gp*)(uintptr_t)((uint64_t*)mxGetData(prhs[1]))[i];
    vbmc_gp_free_all(g_comm, hs.data());
    return 0;
  }
  if (!strcmp(cmd, "gp_free")) { vbmc_gp_free(g_ctx, (vbmc_gp*)(uintptr_t)(*(uint64_t*)mxGetData(prhs[1]))); return 0; }

  if (!strcmp(cmd, "elbo")) {
    // (h, theta, vp, Ns, compute_grad, compute_var, separate_K, beta, thetabnd, eps)
    vbmc_gp* h = (vbmc_gp*)(uintptr_t)(*(uint64_t*)mxGetData(prhs[1]));
    const mxArray* theta = prhs[2];
    const mxArray* vp = prhs[3];
    vbmc_elbo_args a;
    std::vector<double> delta;
    if (fill_vp_args(a, vp, nrhs > 9 ? prhs[9] : nullptr, delta)) return 1;
    a.theta = mxGetDoubles(theta);
    a.Ns = (int)mxGetScalar(prhs[4]);
    a.compute_grad = (int)mxGetScalar(prhs[5]); a.compute_var = (int)mxGetScalar(prhs[6]); a.separate_K = (int)mxGetScalar(prhs[7]);
    a.beta = mxGetScalar(prhs[8]);
    const mxArray* eps = nrhs > 10 ? prhs[10] : nullptr;  // D x Ns/2 x K block drawn by the shim with randn, or []
    if (eps && !mxIsEmpty(eps)) { a.eps_mode = 1; a.eps = mxGetDoubles(eps); a.eps_shared = 1; }
    else { a.eps_mode = 0; a.seed = (uint64_t)(nrhs > 11 ? mxGetScalar(prhs[11]) : 0); }
    a.no_jacobian = (nrhs > 13 && !mxIsEmpty(prhs[13])) ? (mxGetScalar(prhs[13]) != 0) : 0;
    const size_t T = mxGetNumberOfElements(theta);
    mxArray *F = mxCreateDoubleMatrix(1, 1, mxREAL), *dF = mxCreateDoubleMatrix(a.compute_grad ? T : 0, a.compute_grad ? 1 : 0, mxREAL);
    mxArray *G = mxCreateDoubleMatrix(1, 1, mxREAL), *H = mxCreateDoubleMatrix(1, 1, mxREAL), *vG = mxCreateDoubleMatrix(1, 1, mxREAL);
    mxArray *dH = mxCreateDoubleMatrix(a.compute_grad ? T : 0, a.compute_grad ? 1 : 0, mxREAL), *vss = mxCreateDoubleMatrix(1, 1, mxREAL);
    a.F = mxGetDoubles(F); a.G = mxGetDoubles(G); a.H = mxGetDoubles(H); a.varG = mxGetDoubles(vG); a.varGss = mxGetDoubles(vss);
    mxArray* dG = mxCreateDoubleMatrix(a.compute_grad ? T : 0, a.compute_grad ? 1 : 0, mxREAL);  // 10th output (gplogjoint shim)
    if (a.compute_grad) { a.dF = mxGetDoubles(dF); a.dH = mxGetDoubles(dH); a.dG = mxGetDoubles(dG); }
    mxArray *Isk = nullptr, *Jsjk = nullptr;
    if (a.separate_K) {
      // S is known to the library; query through a first call would cost a launch, so the shim passes numel(gp.post)
      const int S = (int)mxGetScalar(prhs[12]);
      Isk = mxCreateDoubleMatrix(S, a.K, mxREAL);
      a.I_sk = mxGetDoubles(Isk);
      if (a.compute_var) { mwSize dims[3] = {(mwSize)S, (mwSize)a.K, (mwSize)a.K}; Jsjk = mxCreateNumericArray(3, dims, mxDOUBLE_CLASS, mxREAL); a.J_sjk = mxGetDoubles(Jsjk); }
    }
    mxArray *Gs = nullptr, *vGs = nullptr;
    if (nlhs > 10 && nrhs > 12) {   // per-hyper-sample values (gplogjoint avg_flag = 0)
      const int S = (int)mxGetScalar(prhs[12]);
      Gs = mxCreateDoubleMatrix(1, S, mxREAL);
      a.G_s = mxGetDoubles(Gs);
      if (nlhs > 11 && a.compute_var) { vGs = mxCreateDoubleMatrix(1, S, mxREAL); a.varG_s = mxGetDoubles(vGs); }
    }
    mxArray* dvG = nullptr;         // 13th output: gradient of the diagonal variance (dvarF of misc/gplogjoint.m:27)
    if (nlhs > 12 && a.compute_grad && a.compute_var == 2) { dvG = mxCreateDoubleMatrix(T, 1, mxREAL); a.dvarG = mxGetDoubles(dvG); }
    mxArray* dGs = nullptr;         // 14th output: the gradient per hyper-sample, T x S (gplogjoint's dF with avg_flag = 0, misc/gplogjoint.m:411 skipped)
    if (nlhs > 13 && a.compute_grad && nrhs > 12) {
      const int S = (int)mxGetScalar(prhs[12]);
      dGs = mxCreateDoubleMatrix(T, S, mxREAL);
      a.dG_s = mxGetDoubles(dGs);
    }
    mxArray* dvGs = nullptr;        // 15th output (ABI 5): the variance gradient per hyper-sample, T x S (gplogjoint's dvarF with avg_flag = 0, :407-409 skipped)
    if (nlhs > 14 && a.compute_grad && a.compute_var == 2 && nrhs > 12) {
      const int S = (int)mxGetScalar(prhs[12]);
      dvGs = mxCreateDoubleMatrix(T, S, mxREAL);
      a.dvarG_s = mxGetDoubles(dvGs);
    }
    vbmc_status st = vbmc_elbo_batch(g_ctx, h, &a);
    if (st != VBMC_OK) return fail(st);  // MATLAB frees the mxArrays created above on error
    mxArray* outs[15] = {F, dF, G, H, vG, dH, vss, Isk, Jsjk, dG, Gs, vGs, dvG, dGs, dvGs};
    for (int i = 0; i < 15 && (i < nlhs || i == 0); ++i) plhs[i] = outs[i] ? outs[i] : mxCreateDoubleMatrix(0, 0, mxREAL);
    return 0;
  }

  const bool multi = !strcmp(cmd, "elbo_batch_multi");
  if (multi && !g_comm) return raise("vbmc_hip:usage", "elbo_batch_multi needs 'comm_open' first");
  if (multi || !strcmp(cmd, "elbo_batch")) {
    // (h, Theta, vp, Ns, compute_grad, compute_var, beta, thetabnd, seed): R = size(Theta,2) candidates that share
    // vp's flags and its non-optimised groups; device MC stream keyed by (seed, r).  'elbo_batch_multi': h is the 1 x n handle
    // vector of 'gp_upload_all' and the candidates are dealt over the n devices.
    vbmc_gp* h = (vbmc_gp*)(uintptr_t)(*(uint64_t*)mxGetData(prhs[1]));
    std::vector<const vbmc_gp*> hs;
    if (multi) {
      if ((int)mxGetNumberOfElements(prhs[1]) != vbmc_comm_local(g_comm)) return raise("vbmc_hip:usage", "elbo_batch_multi: one handle per device");
      for (int i = 0; i < vbmc_comm_local(g_comm); ++i) hs.push_back((const vbmc_gp*)(uintptr_t)((uint64_t*)mxGetData(prhs[1]))[i]);
    }
    const mxArray* Theta = prhs[2];
    vbmc_elbo_args a;
    std::vector<double> delta;
    if (fill_vp_args(a, prhs[3], nrhs > 8 ? prhs[8] : nullptr, delta)) return 1;
    const size_t T = mxGetM(Theta);
    a.R = (int)mxGetN(Theta);
    a.theta = mxGetDoubles(Theta);
    a.Ns = (int)mxGetScalar(prhs[4]); a.compute_grad = (int)mxGetScalar(prhs[5]); a.compute_var = (int)mxGetScalar(prhs[6]);
    a.beta = mxGetScalar(prhs[7]);
    a.eps_mode = 0; a.seed = (uint64_t)(nrhs > 9 ? mxGetScalar(prhs[9]) : 0);
    mxArray *F = mxCreateDoubleMatrix(1, a.R, mxREAL), *dF = mxCreateDoubleMatrix(a.compute_grad ? T : 0, a.compute_grad ? a.R : 0, mxREAL);
    mxArray* vG = mxCreateDoubleMatrix(1, a.R, mxREAL);
    a.F = mxGetDoubles(F); a.varG = mxGetDoubles(vG);
    if (a.compute_grad) a.dF = mxGetDoubles(dF);
    mxArray *G = nullptr, *H = nullptr, *vss = nullptr, *Isk = nullptr, *Jsjk = nullptr;
    if (nlhs > 3) { G = mxCreateDoubleMatrix(1, a.R, mxREAL); a.G = mxGetDoubles(G); }
    if (nlhs > 4) { H = mxCreateDoubleMatrix(1, a.R, mxREAL); a.H = mxGetDoubles(H); }
    if (nlhs > 5) { vss = mxCreateDoubleMatrix(1, a.R, mxREAL); a.varGss = mxGetDoubles(vss); }
    a.separate_K = (nrhs > 10 && nlhs > 6) ? (int)mxGetScalar(prhs[10]) : 0;
    if (a.separate_K) {
      if (nrhs < 12) return raise("vbmc_hip:usage", "elbo_batch with separate_K needs numel(gp.post) as its 12th argument");
      const mwSize S = (mwSize)mxGetScalar(prhs[11]);
      mwSize d3[3] = {S, (mwSize)a.K, (mwSize)a.R}, d4[4] = {S, (mwSize)a.K, (mwSize)a.K, (mwSize)a.R};
      Isk = mxCreateNumericArray(3, d3, mxDOUBLE_CLASS, mxREAL);
      a.I_sk = mxGetDoubles(Isk);
      if (a.compute_var && nlhs > 7) { Jsjk = mxCreateNumericArray(4, d4, mxDOUBLE_CLASS, mxREAL); a.J_sjk = mxGetDoubles(Jsjk); }
    }
    if (multi) {
      vbmc_status st = vbmc_elbo_batch_multi(g_comm, hs.data(), &a);
      if (st != VBMC_OK) return fail_comm(st);
    } else {
      vbmc_status st = vbmc_elbo_batch(g_ctx, h, &a);
      if (st != VBMC_OK) return fail(st);
    }
    mxArray* outs[8] = {F, dF, vG, G, H, vss, Isk, Jsjk};
    for (int i = 0; i < 8 && (i < nlhs || i == 0); ++i) plhs[i] = outs[i] ? outs[i] : mxCreateDoubleMatrix(0, 0, mxREAL);
    return 0;
  }

  if (!strcmp(cmd, "adam")) {
    // (h, Theta0, vp, Ns, compute_var, beta, thetabnd, seed, TolFun, MaxIter, [step_min step_max step_decay])
    vbmc_gp* h = (vbmc_gp*)(uintptr_t)(*(uint64_t*)mxGetData(prhs[1]));
    const mxArray* Theta = prhs[2];
    vbmc_elbo_args a;
    std::vector<double> delta;
    if (fill_vp_args(a, prhs[3], nrhs > 7 ? prhs[7] : nullptr, delta)) return 1;
    const size_t T = mxGetM(Theta);
    a.R = (int)mxGetN(Theta);
    a.theta = mxGetDoubles(Theta);
    a.Ns = (int)mxGetScalar(prhs[4]); a.compute_grad = 1; a.compute_var = (int)mxGetScalar(prhs[5]); a.beta = mxGetScalar(prhs[6]);
    a.eps_mode = 0; a.seed = (uint64_t)mxGetScalar(prhs[8]);
    const double TolFun = mxGetScalar(prhs[9]);
    const int MaxIter = (int)mxGetScalar(prhs[10]);
    double step[3] = {0.001, 0.1, 200.0};  // fminadam.m:28-31 defaults
    for (int i = 0; nrhs > 11 && i < 3 && i < (int)mxGetNumberOfElements(prhs[11]); ++i) step[i] = mxGetDoubles(prhs[11])[i];
    mxArray *x = mxCreateDoubleMatrix(T, a.R, mxREAL), *f = mxCreateDoubleMatrix(1, a.R, mxREAL);
    mxArray* it = mxCreateNumericMatrix(1, a.R, mxINT32_CLASS, mxREAL);
    mxArray *xmid = nullptr, *xtab = nullptr, *ftab = nullptr;
    if (nlhs > 3) xmid = mxCreateDoubleMatrix(T, a.R, mxREAL);
    if (nlhs > 4) { mwSize d3[3] = {(mwSize)T, (mwSize)MaxIter, (mwSize)a.R}; xtab = mxCreateNumericArray(3, d3, mxDOUBLE_CLASS, mxREAL); }
    if (nlhs > 5) ftab = mxCreateDoubleMatrix(MaxIter, a.R, mxREAL);
    vbmc_status st = vbmc_adam_batch(g_ctx, h, &a, TolFun, MaxIter, step[0], step[1], step[2], mxGetDoubles(x), mxGetDoubles(f),
                                     (int32_t*)mxGetData(it), xtab ? mxGetDoubles(xtab) : nullptr, ftab ? mxGetDoubles(ftab) : nullptr,
                                     xmid ? mxGetDoubles(xmid) : nullptr);
    if (st != VBMC_OK) return fail(st);
    plhs[0] = x;
    if (nlhs > 1) plhs[1] = f;
    if (nlhs > 2) plhs[2] = it;
    if (nlhs > 3) plhs[3] = xmid;
    if (nlhs > 4) plhs[4] = xtab;
    if (nlhs > 5) plhs[5] = ftab;
    return 0;
  }

  if (!strcmp(cmd, "gp_post")) {
    // (hyp, X, y, s2, meanfun, noisefun) -> alpha, L, sW, sn2_mult, Lchol, handle
    const mxArray *hyp = prhs[1], *X = prhs[2], *y = prhs[3], *s2 = prhs[4];
    const int N = (int)mxGetM(X), D = (int)mxGetN(X), Nhyp = (int)mxGetM(hyp), S = (int)mxGetN(hyp);
    int32_t nf[3] = {1, 0, 0};
    for (int i = 0; i < 3 && i < (int)mxGetNumberOfElements(prhs[6]); ++i) nf[i] = (int32_t)mxGetDoubles(prhs[6])[i];
    mwSize ld[3] = {(mwSize)N, (mwSize)N, (mwSize)S};
    plhs[0] = mxCreateDoubleMatrix(N, S, mxREAL);
    mxArray* L = mxCreateNumericArray(3, ld, mxDOUBLE_CLASS, mxREAL);
    mxArray* sW = mxCreateDoubleMatrix(N, S, mxREAL);
    mxArray* mult = mxCreateDoubleMatrix(S, 1, mxREAL);
    mxArray* lch = mxCreateNumericMatrix(S, 1, mxUINT8_CLASS, mxREAL);
    vbmc_gp* h = nullptr;
    vbmc_status st = vbmc_gp_post(g_ctx, N, D, S, Nhyp, (int)mxGetScalar(prhs[5]), nf, mxGetDoubles(X), mxGetDoubles(y), dbl(s2),
                                  mxGetDoubles(hyp), mxGetDoubles(plhs[0]), mxGetDoubles(L), mxGetDoubles(sW), mxGetDoubles(mult),
                                  (uint8_t*)mxGetData(lch), &h);
    if (st != VBMC_OK) return fail(st);
    if (nlhs > 1) plhs[1] = L;
    if (nlhs > 2) plhs[2] = sW;
    if (nlhs > 3) plhs[3] = mult;
    if (nlhs > 4) plhs[4] = lch;
    if (nlhs > 5) { plhs[5] = mxCreateNumericMatrix(1, 1, mxUINT64_CLASS, mxREAL); *(uint64_t*)mxGetData(plhs[5]) = (uint64_t)(uintptr_t)h; ++g_stats[1]; }
    else vbmc_gp_free(g_ctx, h);
    return 0;
  }

  if (!strcmp(cmd, "gp_rank1")) {
    // (h, Xnew, ystar, mstar | [], vstar | [], sn2_eff) -> alpha (N+1 x S), L (N+1 x N+1 x S), new handle
    vbmc_gp* h = (vbmc_gp*)(uintptr_t)(*(uint64_t*)mxGetData(prhs[1]));
    const mxArray* Xn = prhs[2];
    const int N1 = (int)mxGetM(Xn), S = (int)mxGetNumberOfElements(prhs[6]);
    mwSize ld[3] = {(mwSize)N1, (mwSize)N1, (mwSize)S};
    plhs[0] = mxCreateDoubleMatrix(N1, S, mxREAL);
    mxArray* L = mxCreateNumericArray(3, ld, mxDOUBLE_CLASS, mxREAL);
    vbmc_gp* hn = nullptr;
    vbmc_status st = vbmc_gp_rank1_update(g_ctx, h, mxGetDoubles(Xn), mxGetScalar(prhs[3]), dbl(prhs[4]), dbl(prhs[5]),
                                          mxGetDoubles(prhs[6]), mxGetDoubles(plhs[0]), nlhs > 1 ? mxGetDoubles(L) : nullptr, &hn);
    if (st != VBMC_OK) return fail(st);
    if (nlhs > 1) plhs[1] = L;
    if (nlhs > 2) { plhs[2] = mxCreateNumericMatrix(1, 1, mxUINT64_CLASS, mxREAL); *(uint64_t*)mxGetData(plhs[2]) = (uint64_t)(uintptr_t)hn; ++g_stats[2]; }
    else vbmc_gp_free(g_ctx, hn);
    return 0;
  }

  if (!strcmp(cmd, "acq")) {
    vbmc_gp* h = (vbmc_gp*)(uintptr_t)(*(uint64_t*)mxGetData(prhs[1]));
    const mxArray *Xs = prhs[2], *vp = prhs[4];
    const int Nstar = (int)mxGetM(Xs);
    plhs[0] = mxCreateDoubleMatrix(Nstar, 1, mxREAL);
    mxArray *fb = mxCreateDoubleMatrix(Nstar, 1, mxREAL), *vt = mxCreateDoubleMatrix(Nstar, 1, mxREAL);
    vbmc_status st = vbmc_acq_eval(g_ctx, h, Nstar, mxGetDoubles(Xs), (int)mxGetScalar(prhs[3]), (int)scalar_field(vp, "K", 0),
                                   dbl(field(vp, "mu")), dbl(field(vp, "sigma")), dbl(field(vp, "lambda")), dbl(field(vp, "w")),
                                   mxGetScalar(prhs[5]), (int)mxGetScalar(prhs[6]), mxGetScalar(prhs[7]),
                                   nrhs > 8 ? dbl(prhs[8]) : nullptr, nrhs > 9 ? dbl(prhs[9]) : nullptr, nrhs > 10 ? dbl(prhs[10]) : nullptr,
                                   mxGetDoubles(plhs[0]), mxGetDoubles(fb), mxGetDoubles(vt));
    if (st != VBMC_OK) return fail(st);
    if (nlhs > 1) plhs[1] = fb;
    if (nlhs > 2) plhs[2] = vt;
    return 0;
  }

  if (!strcmp(cmd, "acq_delta")) {
    if (nrhs < 9) return raise("vbmc_hip:usage", "acq_delta: h, Xs, acq_id, vp, ymax, var_regularized, TolGPVar, delta");
    vbmc_gp* h = (vbmc_gp*)(uintptr_t)(*(uint64_t*)mxGetData(prhs[1]));
    const mxArray *Xs = prhs[2], *vp = prhs[4];
    const int Nstar = (int)mxGetM(Xs), D = (int)mxGetN(Xs);
    if ((int)mxGetNumberOfElements(prhs[8]) != D) return raise("vbmc_hip:usage", "acq_delta: delta must hold one value per dimension");
    plhs[0] = mxCreateDoubleMatrix(Nstar, 1, mxREAL);
    mxArray *fb = mxCreateDoubleMatrix(Nstar, 1, mxREAL), *vt = mxCreateDoubleMatrix(Nstar, 1, mxREAL);
    vbmc_status st = vbmc_acq_eval_delta(g_ctx, h, Nstar, mxGetDoubles(Xs), (int)mxGetScalar(prhs[3]), (int)scalar_field(vp, "K", 0),
                                         dbl(field(vp, "mu")), dbl(field(vp, "sigma")), dbl(field(vp, "lambda")), dbl(field(vp, "w")),
                                         mxGetScalar(prhs[5]), (int)mxGetScalar(prhs[6]), mxGetScalar(prhs[7]),
                                         nrhs > 9 ? dbl(prhs[9]) : nullptr, nrhs > 10 ? dbl(prhs[10]) : nullptr, nrhs > 11 ? dbl(prhs[11]) : nullptr,
                                         mxGetDoubles(plhs[0]), mxGetDoubles(fb), mxGetDoubles(vt), mxGetDoubles(prhs[8]));
    if (nlhs > 1) plhs[1] = fb; else mxDestroyArray(fb);
    if (nlhs > 2) plhs[2] = vt; else mxDestroyArray(vt);
    if (st != VBMC_OK) return fail(st);
    return 0;
  }

  // [xmin, fmin, out] = acq_search(h, acq_id, vp, ymax, var_regularized, TolGPVar, x0, insigma, LB, UB, opts [, gplengthscale, X_rescaled, sn2new])
  // opts: TolX, TolFun, TolHistFun, MaxFunEvals, MaxIter, PopSize, Seed, Chunk, Z (D x lambda x Gmax: parity mode); out: the bestever
  // point and value, the final xmean / sigma / C, evals, generations, stop (1 TolX .. 5 MaxIter), behind
  // [xmin, fmin, out] = acq_search_iqr(h, his, acq_id, vp, var_regularized, TolGPVar, x0, insigma, LB, UB, opts, gplengthscale, X_rescaled, sn2new)
  // the same opts and out on the IQR functions (vbmc_acq_search_iqr): from var_regularized on the arguments sit where acq_search has them
  const bool search_iqr = !strcmp(cmd, "acq_search_iqr");
  if (!strcmp(cmd, "acq_search") || search_iqr) {
    if (search_iqr && (nrhs < 15 || !mxIsStruct(prhs[4]) || !mxIsStruct(prhs[11])))
      return raise("vbmc_hip:usage", "acq_search_iqr: h, his, acq_id, vp, var_regularized, TolGPVar, x0, insigma, LB, UB, opts, gplengthscale, X_rescaled, sn2new");
    if (!search_iqr && (nrhs < 12 || !mxIsStruct(prhs[3]) || !mxIsStruct(prhs[11])))
      return raise("vbmc_hip:usage", "acq_search: h, acq_id, vp, ymax, var_regularized, TolGPVar, x0, insigma, LB, UB, opts [, gplengthscale, X_rescaled, sn2new]");
    vbmc_gp* h = (vbmc_gp*)(uintptr_t)(*(uint64_t*)mxGetData(prhs[1]));
    const mxArray *vp = prhs[search_iqr ? 4 : 3], *op = prhs[11];
    const int D = (int)mxGetNumberOfElements(prhs[7]);
    for (int i = 8; i <= 10; ++i)
      if ((int)mxGetNumberOfElements(prhs[i]) != D) return raise("vbmc_hip:usage", "acq_search: x0, insigma, LB and UB must hold one value per dimension");
    if (D < 1 || !field(vp, "lambda") || (int)mxGetNumberOfElements(field(vp, "lambda")) != D)
      return raise("vbmc_hip:usage", "acq_search: vp.lambda must hold one value per dimension");
    vbmc_acqsearch_args a;
    memset(&a, 0, sizeof a);
    a.struct_size = sizeof a;
    a.acq_id = (int)mxGetScalar(prhs[search_iqr ? 3 : 2]); a.K = (int)scalar_field(vp, "K", 0);
    a.vp_mu = dbl(field(vp, "mu")); a.vp_sigma = dbl(field(vp, "sigma")); a.vp_lambda = dbl(field(vp, "lambda")); a.vp_w = dbl(field(vp, "w"));
    std::vector<double> delta;
    if (const mxArray* dl = field(vp, "delta")) {
      const int nd = (int)mxGetNumberOfElements(dl);
      if (nd == 1) delta.assign(D, mxGetScalar(dl));
      else if (nd == D) delta.assign(mxGetDoubles(dl), mxGetDoubles(dl) + D);
      else if (nd != 0) return raise("vbmc_hip:unsupported", "acq_search: vp.delta must be empty, a scalar or one value per dimension");
      if (!delta.empty()) a.vp_delta = delta.data();
    }
    a.ymax = search_iqr ? 0.0 : mxGetScalar(prhs[4]); a.var_regularized = (int)mxGetScalar(prhs[5]); a.TolGPVar = mxGetScalar(prhs[6]);
    a.x0 = dbl(prhs[7]); a.insigma = dbl(prhs[8]); a.LB = dbl(prhs[9]); a.UB = dbl(prhs[10]);
    a.gplengthscale = nrhs > 12 ? dbl(prhs[12]) : nullptr; a.X_rescaled = nrhs > 13 ? dbl(prhs[13]) : nullptr; a.sn2new = nrhs > 14 ? dbl(prhs[14]) : nullptr;
    a.TolX = scalar_field(op, "TolX", 0.0); a.TolFun = scalar_field(op, "TolFun", 0.0); a.TolHistFun = scalar_field(op, "TolHistFun", 0.0);
    const double mfe = scalar_field(op, "MaxFunEvals", 0.0);
    a.MaxFunEvals = (mfe > 0.0 && mfe < 9e18) ? (int64_t)mfe : 0;
    a.MaxIter = (int)scalar_field(op, "MaxIter", 0.0); a.popsize = (int)scalar_field(op, "PopSize", 0.0); a.chunk = (int)scalar_field(op, "Chunk", 0.0);
    a.seed = (uint64_t)scalar_field(op, "Seed", 0.0);
    if (const mxArray* z = field(op, "Z")) {
      if (!mxIsEmpty(z)) {
        const int lam = a.popsize ? a.popsize : 4 + (int)std::floor(3.0 * std::log((double)D));
        const size_t nz = mxGetNumberOfElements(z);
        if (nz % ((size_t)D * lam) != 0) return raise("vbmc_hip:usage", "acq_search: opts.Z must be D x lambda x Gmax");
        a.rng_mode = 1; a.Z = mxGetDoubles(z); a.Gmax = (int)(nz / ((size_t)D * lam));
      }
    }
    const char* names[] = {"xbest", "fbest", "xmean", "sigma", "C", "evals", "generations", "stop", "behind"};
    mxArray* out = mxCreateStructMatrix(1, 1, 9, names);
    mxArray* f[9];
    const int rows[9] = {D, 1, D, 1, D, 1, 1, 1, 1}, cols[9] = {1, 1, 1, 1, D, 1, 1, 1, 1};
    for (int i = 0; i < 9; ++i) { f[i] = mxCreateDoubleMatrix(rows[i], cols[i], mxREAL); mxSetField(out, 0, names[i], f[i]); }
    plhs[0] = mxCreateDoubleMatrix(D, 1, mxREAL);
    mxArray* fmin = mxCreateDoubleMatrix(1, 1, mxREAL);
    int64_t evals = 0, rounds[2] = {0, 0};
    int32_t gens = 0, stop = 0;
    a.xmin = mxGetDoubles(plhs[0]); a.fmin = mxGetDoubles(fmin);
    a.xbest = mxGetDoubles(f[0]); a.fbest = mxGetDoubles(f[1]); a.xmean = mxGetDoubles(f[2]); a.sigma = mxGetDoubles(f[3]); a.C = mxGetDoubles(f[4]);
    a.evals = &evals; a.generations = &gens; a.stop = &stop; a.rounds = rounds;
    vbmc_status st = search_iqr ? vbmc_acq_search_iqr(g_ctx, h, (vbmc_acq_is*)(uintptr_t)(*(uint64_t*)mxGetData(prhs[2])), &a) : vbmc_acq_search(g_ctx, h, &a);
    mxGetDoubles(f[5])[0] = (double)evals; mxGetDoubles(f[6])[0] = gens; mxGetDoubles(f[7])[0] = stop; mxGetDoubles(f[8])[0] = (double)rounds[1];
    if (nlhs > 1) plhs[1] = fmin; else mxDestroyArray(fmin);
    if (nlhs > 2) plhs[2] = out; else mxDestroyArray(out);
    if (st != VBMC_OK) return fail(st);
    return 0;
  }

  if (!strcmp(cmd, "gp_quad")) {
    if (nrhs < 6) return raise("vbmc_hip:usage", "gp_quad: h, mu, sigma, ssflag, numel(gp.post)");
    vbmc_gp* h = (vbmc_gp*)(uintptr_t)(*(uint64_t*)mxGetData(prhs[1]));
    const mxArray *mu = prhs[2], *sg = prhs[3];
    const int Nstar = (int)mxGetM(mu), D = (int)mxGetN(mu), ss = (int)mxGetScalar(prhs[4]), S = (int)mxGetScalar(prhs[5]);
    const int rows = (int)mxGetM(sg);
    if ((int)mxGetN(sg) != D || (rows != 1 && rows != Nstar)) return raise("vbmc_hip:usage", "gp_quad: sigma must be 1 x D or Nstar x D");
    const int nc = (ss && S > 1) ? S : 1;
    plhs[0] = mxCreateDoubleMatrix(Nstar, nc, mxREAL);
    mxArray* vf = nlhs > 1 ? mxCreateDoubleMatrix(Nstar, nc, mxREAL) : nullptr;
    vbmc_status st = vbmc_gp_quad(g_ctx, h, Nstar, mxGetDoubles(mu), mxGetDoubles(sg), rows, ss || S == 1, mxGetDoubles(plhs[0]),
                                  vf ? mxGetDoubles(vf) : nullptr);
    if (vf) plhs[1] = vf;
    if (st != VBMC_OK) return fail(st);
    return 0;
  }

  if (!strcmp(cmd, "acq_is_sample")) {
    if (nrhs < 7 || !mxIsStruct(prhs[6])) return raise("vbmc_hip:usage", "acq_is_sample: h, x0, LB, UB, Nm, opts");
    vbmc_gp* h = (vbmc_gp*)(uintptr_t)(*(uint64_t*)mxGetData(prhs[1]));
    const mxArray *x0 = prhs[2], *op = prhs[6];
    const mwSize nd = mxGetNumberOfDimensions(x0);
    const mwSize* dm = mxGetDimensions(x0);
    const int W = (int)dm[0], D = (int)dm[1], S = nd > 2 ? (int)dm[2] : 1, Nm = (int)mxGetScalar(prhs[5]);
    if ((int)mxGetNumberOfElements(prhs[3]) != D || (int)mxGetNumberOfElements(prhs[4]) != D || Nm < 1)
      return raise("vbmc_hip:usage", "acq_is_sample: x0 must be W x D x S, LB and UB must hold one value per dimension, Nm must be positive");
    vbmc_is_sample_args a;
    memset(&a, 0, sizeof a);
    a.struct_size = sizeof a;
    a.W = W; a.D = D; a.S = S; a.Nm = Nm; a.thin = (int)scalar_field(op, "Thin", 1.0); a.burnin = (int)scalar_field(op, "Burnin", -1.0);
    a.spec = (int)scalar_field(op, "Spec", 0.0); a.max_steps = (int)scalar_field(op, "MaxSteps", 0.0); a.max_shrink = (int)scalar_field(op, "MaxShrink", 0.0);
    a.chunk = (int)scalar_field(op, "Chunk", 0.0); a.seed = (uint64_t)scalar_field(op, "Seed", 0.0);
    a.x0 = mxGetDoubles(x0); a.LB = dbl(prhs[3]); a.UB = dbl(prhs[4]);
    if (const mxArray* u = field(op, "U")) {
      if (!mxIsEmpty(u)) {
        const size_t nu = mxGetNumberOfElements(u), per = (size_t)64 * (size_t)(W / 2) * (size_t)S;
        if (per == 0 || nu % per != 0) return raise("vbmc_hip:usage", "acq_is_sample: opts.U must be 64 x H x S x Mmax");
        a.rng_mode = 1; a.U = mxGetDoubles(u); a.Mmax = (int)(nu / per);
      }
    }
    const mwSize dx[3] = {(mwSize)Nm, (mwSize)D, (mwSize)S};
    mxArray* Xa = mxCreateNumericArray(3, dx, mxDOUBLE_CLASS, mxREAL);
    mxArray* lnw = mxCreateDoubleMatrix(S, Nm, mxREAL);
    mxArray* fs2a = mxCreateDoubleMatrix(Nm, S, mxREAL);
    const char* names[] = {"logp", "funccount", "performed", "rounds", "behind"};
    mxArray* out = mxCreateStructMatrix(1, 1, 5, names);
    mxArray* f[5];
    for (int i = 0; i < 5; ++i) { f[i] = mxCreateDoubleMatrix(i == 0 ? S : 1, i == 0 ? Nm : 1, mxREAL); mxSetField(out, 0, names[i], f[i]); }
    int64_t funccount = 0, performed = 0, rounds[2] = {0, 0};
    vbmc_acq_is* is = nullptr;
    a.Xa = mxGetDoubles(Xa); a.lnw = mxGetDoubles(lnw); a.fs2a = mxGetDoubles(fs2a); a.logp = mxGetDoubles(f[0]);
    a.funccount = &funccount; a.performed = &performed; a.rounds = rounds;
    if (nlhs > 3) a.state = &is;
    vbmc_status st = vbmc_acq_is_sample(g_ctx, h, &a);
    mxGetDoubles(f[1])[0] = (double)funccount; mxGetDoubles(f[2])[0] = (double)performed;
    mxGetDoubles(f[3])[0] = (double)rounds[0]; mxGetDoubles(f[4])[0] = (double)rounds[1];
    plhs[0] = Xa;
    if (nlhs > 1) plhs[1] = lnw; else mxDestroyArray(lnw);
    if (nlhs > 2) plhs[2] = fs2a; else mxDestroyArray(fs2a);
    if (nlhs > 3) {
      plhs[3] = mxCreateNumericMatrix(1, 1, mxUINT64_CLASS, mxREAL);
      *(uint64_t*)mxGetData(plhs[3]) = (uint64_t)(uintptr_t)is;
    }
    if (nlhs > 4) plhs[4] = out; else mxDestroyArray(out);
    if (st != VBMC_OK) return fail(st);
    return 0;
  }

  if (!strcmp(cmd, "is_create")) {
    vbmc_gp* h = (vbmc_gp*)(uintptr_t)(*(uint64_t*)mxGetData(prhs[1]));
    const mxArray* Xa = prhs[2];
    const mwSize nd = mxGetNumberOfDimensions(Xa);
    const int Na = (int)mxGetDimensions(Xa)[0];
    vbmc_acq_is* is = nullptr;
    vbmc_status st = vbmc_acq_is_create(g_ctx, h, Na, mxGetDoubles(Xa), nd > 2 ? 1 : 0, nrhs > 3 ? dbl(prhs[3]) : nullptr,
                                        nrhs > 4 ? dbl(prhs[4]) : nullptr, nrhs > 5 ? dbl(prhs[5]) : nullptr, &is);
    if (st != VBMC_OK) return fail(st);
    plhs[0] = mxCreateNumericMatrix(1, 1, mxUINT64_CLASS, mxREAL);
    *(uint64_t*)mxGetData(plhs[0]) = (uint64_t)(uintptr_t)is;
    return 0;
  }
  if (!strcmp(cmd, "is_free")) { vbmc_acq_is_free(g_ctx, (vbmc_acq_is*)(uintptr_t)(*(uint64_t*)mxGetData(prhs[1]))); return 0; }

  if (!strcmp(cmd, "is_setup")) {
    if (nrhs < 7 || !mxIsStruct(prhs[2]) || !mxIsStruct(prhs[6])) return raise("vbmc_hip:usage", "is_setup: h, vp, Nvp, Nbox, Nm, opts");
    vbmc_gp* h = (vbmc_gp*)(uintptr_t)(*(uint64_t*)mxGetData(prhs[1]));
    const mxArray *vp = prhs[2], *op = prhs[6];
    const mxArray *mu = field(vp, "mu"), *sg = field(vp, "sigma"), *lm = field(vp, "lambda"), *ww = field(vp, "w");
    if (!mu || !sg || !lm || !ww || mxIsEmpty(mu)) return raise("vbmc_hip:usage", "is_setup: vp needs mu, sigma, lambda and w");
    const int D = (int)mxGetM(mu), K = (int)mxGetN(mu), S = (int)scalar_field(op, "S", 0.0);
    const int Nvp = (int)mxGetScalar(prhs[3]), Nbox = (int)mxGetScalar(prhs[4]), Nm = (int)mxGetScalar(prhs[5]);
    if ((int)mxGetNumberOfElements(sg) != K || (int)mxGetNumberOfElements(ww) != K || (int)mxGetNumberOfElements(lm) != D || S < 1 || Nm < 0 || Nvp < 0 ||
        Nbox < 0 || Nvp + Nbox < 1)
      return raise("vbmc_hip:usage", "is_setup: vp.mu must be D x K with K sigmas and weights and D lambdas, opts.S = numel(gp.post), the counts non-negative");
    vbmc_is_setup_args a;
    memset(&a, 0, sizeof a);
    a.struct_size = sizeof a;
    a.D = D; a.S = S; a.K = K; a.Nvp = Nvp; a.Nbox = Nbox; a.Nm = Nm;
    a.vp_mu = mxGetDoubles(mu); a.vp_sigma = mxGetDoubles(sg); a.vp_lambda = mxGetDoubles(lm); a.vp_w = mxGetDoubles(ww);
    a.W = (int)scalar_field(op, "W", 0.0);
    if (a.W == 0) a.W = 2 * (D + 1);
    const int W = a.W, Na1 = Nvp + Nbox;
    if (W < 0) return raise("vbmc_hip:usage", "is_setup: opts.W must be positive");
    a.thin = (int)scalar_field(op, "Thin", 1.0); a.burnin = (int)scalar_field(op, "Burnin", -1.0);
    a.spec = (int)scalar_field(op, "Spec", 0.0); a.max_steps = (int)scalar_field(op, "MaxSteps", 0.0); a.max_shrink = (int)scalar_field(op, "MaxShrink", 0.0);
    a.chunk = (int)scalar_field(op, "Chunk", 0.0); a.seed = (uint64_t)scalar_field(op, "Seed", 0.0);
    if (const mxArray* b = field(op, "B")) {
      if (!mxIsEmpty(b)) {
        if (mxGetNumberOfElements(b) != (size_t)(D + 1) * Na1 + (Nm > 0 ? (size_t)W * S : 0)) return raise("vbmc_hip:usage", "is_setup: opts.B must hold (D + 1) (Nvp + Nbox) + W S values");
        a.rng_mode = 1; a.B = mxGetDoubles(b);
        const mxArray* u = field(op, "U");
        if (u && !mxIsEmpty(u)) {
          const size_t nu = mxGetNumberOfElements(u), per = (size_t)64 * (size_t)(W / 2) * (size_t)S;
          if (per == 0 || nu % per != 0) return raise("vbmc_hip:usage", "is_setup: opts.U must be 64 x H x S x Mmax");
          a.U = mxGetDoubles(u); a.Mmax = (int)(nu / per);
        }
      }
    }
    const mwSize dx[3] = {(mwSize)Nm, (mwSize)D, (mwSize)S}, d0[3] = {(mwSize)W, (mwSize)D, (mwSize)S};
    mxArray* Xa = mxCreateNumericArray(3, dx, mxDOUBLE_CLASS, mxREAL);
    mxArray* lnw = mxCreateDoubleMatrix(S, Nm, mxREAL);
    mxArray* fs2a = mxCreateDoubleMatrix(Nm, S, mxREAL);
    const char* names[] = {"Xa1", "lnw1", "fs2a1", "lpdf1", "rect_delta", "LB", "UB", "x0", "idx0", "n_bad", "bad", "logp", "funccount", "performed", "rounds", "behind"};
    enum { oXa1, oLnw1, oFs2a1, oLpdf1, oRd, oLB, oUB, oX0, oIdx0, oNbad, oBad, oLogp, oFc, oPf, oRounds, oBehind, oCount };
    mxArray* out = mxCreateStructMatrix(1, 1, oCount, names);
    mxArray* f[oCount];
    const int rows[oCount] = {Na1, S, Na1, Na1, D, D, D, 0, W, 1, W, S, 1, 1, 1, 1}, cols[oCount] = {D, Na1, S, 1, 1, 1, 1, 0, S, 1, S, Nm, 1, 1, 1, 1};
    for (int i = 0; i < oCount; ++i) {
      f[i] = i == oX0 ? mxCreateNumericArray(3, d0, mxDOUBLE_CLASS, mxREAL) : mxCreateDoubleMatrix(rows[i], cols[i], mxREAL);
      mxSetField(out, 0, names[i], f[i]);
    }
    std::vector<int32_t> idx0((size_t)W * S + 1, 0);
    std::vector<uint8_t> bad((size_t)W * S + 1, 0);
    int32_t n_bad = 0;
    int64_t funccount = 0, performed = 0, rounds[2] = {0, 0};
    vbmc_acq_is* is = nullptr;
    a.Xa1 = mxGetDoubles(f[oXa1]); a.lnw1 = mxGetDoubles(f[oLnw1]); a.fs2a1 = mxGetDoubles(f[oFs2a1]); a.lpdf1 = mxGetDoubles(f[oLpdf1]);
    a.rect_delta = mxGetDoubles(f[oRd]); a.LB = mxGetDoubles(f[oLB]); a.UB = mxGetDoubles(f[oUB]); a.x0 = mxGetDoubles(f[oX0]);
    a.idx0 = idx0.data(); a.n_bad = &n_bad; a.bad = bad.data();
    if (Nm > 0) { a.Xa = mxGetDoubles(Xa); a.lnw = mxGetDoubles(lnw); a.fs2a = mxGetDoubles(fs2a); a.logp = mxGetDoubles(f[oLogp]); }
    a.funccount = &funccount; a.performed = &performed; a.rounds = rounds;
    if (nlhs > 3) a.state = &is;
    vbmc_status st = vbmc_acq_is_setup(g_ctx, h, &a);
    for (size_t j = 0; j < (size_t)W * S; ++j) { mxGetDoubles(f[oIdx0])[j] = (double)idx0[j]; mxGetDoubles(f[oBad])[j] = (double)bad[j]; }
    mxGetDoubles(f[oNbad])[0] = (double)n_bad;
    mxGetDoubles(f[oFc])[0] = (double)funccount; mxGetDoubles(f[oPf])[0] = (double)performed;
    mxGetDoubles(f[oRounds])[0] = (double)rounds[0]; mxGetDoubles(f[oBehind])[0] = (double)rounds[1];
    plhs[0] = Xa;
    if (nlhs > 1) plhs[1] = lnw; else mxDestroyArray(lnw);
    if (nlhs > 2) plhs[2] = fs2a; else mxDestroyArray(fs2a);
    if (nlhs > 3) {
      plhs[3] = mxCreateNumericMatrix(1, 1, mxUINT64_CLASS, mxREAL);
      *(uint64_t*)mxGetData(plhs[3]) = (uint64_t)(uintptr_t)is;
    }
    if (nlhs > 4) plhs[4] = out; else mxDestroyArray(out);
    if (st != VBMC_OK) return fail(st);
    return 0;
  }

  if (!strcmp(cmd, "vp_pdf")) {      // [y,dy] = vbmc_pdf(vp,X,origflag,logflag,transflag,df): vbmc_vp_pdf
    if (nrhs < 7) return raise("vbmc_hip:usage", "vp_pdf: vp, X, origflag, logflag, transflag, df");
    vbmc_vp_desc d;
    std::vector<int32_t> ty;
    if (fill_vp_desc(d, prhs[1], ty)) return 1;
    const mxArray* X = prhs[2];
    if (!mxIsDouble(X) || (int)mxGetN(X) != d.D) return raise("vbmc_hip:usage", "vp_pdf: X must be N x D");
    const mwSize N = mxGetM(X);
    plhs[0] = mxCreateDoubleMatrix(N, 1, mxREAL);
    mxArray* dy = nlhs > 1 ? mxCreateDoubleMatrix(N, d.D, mxREAL) : nullptr;
    if (dy) plhs[1] = dy;
    vbmc_status st = vbmc_vp_pdf(g_ctx, &d, (int64_t)N, dbl(X), mxGetScalar(prhs[3]) != 0, mxGetScalar(prhs[4]) != 0, mxGetScalar(prhs[5]) != 0, mxGetScalar(prhs[6]),
                                 mxGetDoubles(plhs[0]), dy ? mxGetDoubles(dy) : nullptr);
    if (st != VBMC_OK) return fail(st);
    return 0;
  }

  if (!strcmp(cmd, "vp_rnd")) {      // [X,I] = vbmc_rnd(vp,N,origflag,balanceflag,df) with the library's draws for seed (I from 0): vbmc_vp_rnd
    if (nrhs < 7) return raise("vbmc_hip:usage", "vp_rnd: vp, N, origflag, balanceflag, df, seed");
    vbmc_vp_desc d;
    std::vector<int32_t> ty;
    if (fill_vp_desc(d, prhs[1], ty)) return 1;
    const double n = mxGetScalar(prhs[2]);
    if (!(n >= 0)) return raise("vbmc_hip:usage", "vp_rnd: N must be non-negative");
    const mwSize N = (mwSize)n;
    plhs[0] = mxCreateDoubleMatrix(N, d.D, mxREAL);
    std::vector<int32_t> I(N);
    vbmc_status st = vbmc_vp_rnd(g_ctx, &d, (int64_t)N, mxGetScalar(prhs[3]) != 0, (int)mxGetScalar(prhs[4]), mxGetScalar(prhs[5]), (uint64_t)mxGetScalar(prhs[6]), nullptr,
                                 mxGetDoubles(plhs[0]), I.data());
    if (nlhs > 1) {
      plhs[1] = mxCreateDoubleMatrix(N, 1, mxREAL);
      for (mwSize i = 0; i < N; ++i) mxGetDoubles(plhs[1])[i] = (double)I[i];
    }
    if (st != VBMC_OK) return fail(st);
    return 0;
  }

  if (!strcmp(cmd, "vp_moments")) {  // [mubar,Sigma] = vbmc_moments(vp,1,Ns) with the library's draws for seed: vbmc_vp_moments
    if (nrhs < 4) return raise("vbmc_hip:usage", "vp_moments: vp, Ns, seed");
    vbmc_vp_desc d;
    std::vector<int32_t> ty;
    if (fill_vp_desc(d, prhs[1], ty)) return 1;
    plhs[0] = mxCreateDoubleMatrix(1, d.D, mxREAL);
    mxArray* S = nlhs > 1 ? mxCreateDoubleMatrix(d.D, d.D, mxREAL) : nullptr;
    if (S) plhs[1] = S;
    vbmc_status st = vbmc_vp_moments(g_ctx, &d, (int64_t)mxGetScalar(prhs[2]), (uint64_t)mxGetScalar(prhs[3]), nullptr, mxGetDoubles(plhs[0]), S ? mxGetDoubles(S) : nullptr);
    if (st != VBMC_OK) return fail(st);
    return 0;
  }

  if (!strcmp(cmd, "vp_kldiv")) {    // [kls,xx1,xx2] = vbmc_kldiv(vp1,vp2,Ns,0) with the library's draws for seed: vbmc_vp_kldiv
    if (nrhs < 5) return raise("vbmc_hip:usage", "vp_kldiv: vp1, vp2, Ns, seed");
    vbmc_vp_desc d1, d2;
    std::vector<int32_t> t1, t2;
    if (fill_vp_desc(d1, prhs[1], t1) || fill_vp_desc(d2, prhs[2], t2)) return 1;
    const double n = mxGetScalar(prhs[3]);
    if (!(n >= 1)) return raise("vbmc_hip:usage", "vp_kldiv: Ns must be positive");
    const mwSize Ns = (mwSize)n;
    plhs[0] = mxCreateDoubleMatrix(1, 2, mxREAL);
    mxArray *x1 = nlhs > 1 ? mxCreateDoubleMatrix(Ns, d1.D, mxREAL) : nullptr, *x2 = nlhs > 2 ? mxCreateDoubleMatrix(Ns, d1.D, mxREAL) : nullptr;
    if (x1) plhs[1] = x1;
    if (x2) plhs[2] = x2;
    vbmc_status st = vbmc_vp_kldiv(g_ctx, &d1, &d2, (int64_t)Ns, (uint64_t)mxGetScalar(prhs[4]), nullptr, nullptr, mxGetDoubles(plhs[0]), x1 ? mxGetDoubles(x1) : nullptr,
                                   x2 ? mxGetDoubles(x2) : nullptr);
    if (st != VBMC_OK) return fail(st);
    return 0;
  }

  if (!strcmp(cmd, "vp_mtv")) {      // [mtv,xx1,xx2] = vbmc_mtv(vp1,vp2,Ns) with the library's draws for seed: vbmc_vp_mtv
    if (nrhs < 5) return raise("vbmc_hip:usage", "vp_mtv: vp1, vp2, Ns, seed");
    vbmc_vp_desc d1, d2;
    std::vector<int32_t> t1, t2;
    if (fill_vp_desc(d1, prhs[1], t1) || fill_vp_desc(d2, prhs[2], t2)) return 1;
    const double n = mxGetScalar(prhs[3]);
    if (!(n >= 1)) return raise("vbmc_hip:usage", "vp_mtv: Ns must be positive");
    const mwSize Ns = (mwSize)n;
    plhs[0] = mxCreateDoubleMatrix(1, d1.D, mxREAL);
    mxArray *x1 = nlhs > 1 ? mxCreateDoubleMatrix(Ns, d1.D, mxREAL) : nullptr, *x2 = nlhs > 2 ? mxCreateDoubleMatrix(Ns, d1.D, mxREAL) : nullptr;
    if (x1) plhs[1] = x1;
    if (x2) plhs[2] = x2;
    vbmc_mtv_args a;
    memset(&a, 0, sizeof a);
    a.struct_size = sizeof a;
    a.Ns = (int64_t)Ns;
    a.seed = (uint64_t)mxGetScalar(prhs[4]);
    a.mtv = mxGetDoubles(plhs[0]);
    a.xx1 = x1 ? mxGetDoubles(x1) : nullptr;
    a.xx2 = x2 ? mxGetDoubles(x2) : nullptr;
    vbmc_status st = vbmc_vp_mtv(g_ctx, &d1, &d2, &a);
    if (st != VBMC_OK) return fail(st);
    return 0;
  }

  if (!strcmp(cmd, "acq_iqr")) {
    vbmc_gp* h = (vbmc_gp*)(uintptr_t)(*(uint64_t*)mxGetData(prhs[1]));
    vbmc_acq_is* is = (vbmc_acq_is*)(uintptr_t)(*(uint64_t*)mxGetData(prhs[2]));
    const mxArray* Xs = prhs[3];
    const int Nstar = (int)mxGetM(Xs);
    plhs[0] = mxCreateDoubleMatrix(Nstar, 1, mxREAL);
    mxArray *fb = mxCreateDoubleMatrix(Nstar, 1, mxREAL), *vt = mxCreateDoubleMatrix(Nstar, 1, mxREAL);
    vbmc_status st = vbmc_acq_iqr_eval(g_ctx, h, is, Nstar, mxGetDoubles(Xs), dbl(prhs[4]), dbl(prhs[5]), dbl(prhs[6]),
                                       (int)mxGetScalar(prhs[7]), mxGetScalar(prhs[8]), mxGetDoubles(plhs[0]), mxGetDoubles(fb), mxGetDoubles(vt));
    if (st != VBMC_OK) return fail(st);
    if (nlhs > 1) plhs[1] = fb;
    if (nlhs > 2) plhs[2] = vt;
    return 0;
  }

  if (!strcmp(cmd, "gp_surrogate_sample")) {   // X = gpsample_vbmc(vp,gp,Ns,origflag) with the library's draws for opts.Seed: vbmc_gp_surrogate_sample
    if (nrhs < 9 || !mxIsStruct(prhs[8])) return raise("vbmc_hip:usage", "gp_surrogate_sample: h, vp, Ns, origflag, LB, UB, noise, opts");
    vbmc_gp* h = (vbmc_gp*)(uintptr_t)(*(uint64_t*)mxGetData(prhs[1]));
    vbmc_vp_desc d;
    std::vector<int32_t> ty;
    const bool have_vp = mxIsStruct(prhs[2]);
    if (have_vp && fill_vp_desc(d, prhs[2], ty)) return 1;
    const mxArray *nz = prhs[7], *op = prhs[8];
    const double n = mxGetScalar(prhs[3]);
    const int D = (int)mxGetNumberOfElements(prhs[5]);
    if (!(n >= 1) || D < 1 || (int)mxGetNumberOfElements(prhs[6]) != D || (have_vp && d.D != D))
      return raise("vbmc_hip:usage", "gp_surrogate_sample: Ns must be positive, LB and UB must hold one value per dimension of vp");
    vbmc_gs_args a;
    memset(&a, 0, sizeof a);
    a.struct_size = sizeof a;
    a.D = D; a.S = (int)scalar_field(op, "S", 1.0); a.Ns = (int64_t)n; a.origflag = mxGetScalar(prhs[4]) != 0;
    a.E = (int)scalar_field(op, "E", 1.0); a.W = (int)scalar_field(op, "W", 0.0);
    a.thin = (int)scalar_field(op, "Thin", 1.0); a.burnin = (int)scalar_field(op, "Burnin", -1.0);
    a.spec = (int)scalar_field(op, "Spec", 0.0); a.max_steps = (int)scalar_field(op, "MaxSteps", 0.0); a.max_shrink = (int)scalar_field(op, "MaxShrink", 0.0);
    a.chunk = (int)scalar_field(op, "Chunk", 0.0); a.seed = (uint64_t)scalar_field(op, "Seed", 0.0); a.Nnn = (int)scalar_field(op, "Nnn", 0.0);
    a.beta = scalar_field(op, "Beta", 0.0); a.VarThresh = scalar_field(op, "VarThresh", std::numeric_limits<double>::infinity());
    a.LB = dbl(prhs[5]); a.UB = dbl(prhs[6]);
    if (const mxArray* x0 = field(op, "x0")) {
      if (!mxIsEmpty(x0)) {
        const mwSize* dm = mxGetDimensions(x0);
        if ((int)dm[1] != D || mxGetNumberOfElements(x0) != (size_t)dm[0] * D * a.E) return raise("vbmc_hip:usage", "gp_surrogate_sample: opts.x0 must be W x D x E");
        a.W = (int)dm[0]; a.x0 = mxGetDoubles(x0);
      }
    }
    if (mxIsStruct(nz)) {
      const mxArray *xr = field(nz, "X_rescaled"), *gl = field(nz, "gplengthscale"), *sn = field(nz, "sn2new");
      if (!xr || !gl || !sn || (int)mxGetNumberOfElements(gl) != D || mxGetNumberOfElements(xr) != mxGetNumberOfElements(sn) * D)
        return raise("vbmc_hip:usage", "gp_surrogate_sample: noise needs X_rescaled (N x D), gplengthscale (D) and sn2new (N)");
      a.X_rescaled = mxGetDoubles(xr); a.gplengthscale = mxGetDoubles(gl); a.sn2new = mxGetDoubles(sn);
    }
    plhs[0] = mxCreateDoubleMatrix((mwSize)n, D, mxREAL);
    const char* names[] = {"VarThresh", "sn2_avg", "funccount", "performed", "rounds", "behind"};
    mxArray* out = mxCreateStructMatrix(1, 1, 6, names);
    mxArray* f[6];
    for (int i = 0; i < 6; ++i) { f[i] = mxCreateDoubleMatrix(1, 1, mxREAL); mxSetField(out, 0, names[i], f[i]); }
    int64_t funccount = 0, performed = 0, rounds[2] = {0, 0};
    a.X = mxGetDoubles(plhs[0]); a.varthresh_out = mxGetDoubles(f[0]); a.sn2_avg_out = mxGetDoubles(f[1]);
    a.funccount = &funccount; a.performed = &performed; a.rounds = rounds;
    vbmc_status st = vbmc_gp_surrogate_sample(g_ctx, h, have_vp ? &d : nullptr, &a);
    mxGetDoubles(f[2])[0] = (double)funccount; mxGetDoubles(f[3])[0] = (double)performed;
    mxGetDoubles(f[4])[0] = (double)rounds[0]; mxGetDoubles(f[5])[0] = (double)rounds[1];
    if (nlhs > 1) plhs[1] = out; else mxDestroyArray(out);
    if (st != VBMC_OK) return fail(st);
    return 0;
  }

  if (!strcmp(cmd, "gp_nlz")) {
    const mxArray *hyp = prhs[1], *X = prhs[2], *y = prhs[3], *s2 = prhs[4];
    const int N = (int)mxGetM(X), D = (int)mxGetN(X), Nhyp = (int)mxGetM(hyp), B = (int)mxGetN(hyp);
    int32_t nf[3] = {1, 0, 0};
    for (int i = 0; i < 3 && i < (int)mxGetNumberOfElements(prhs[6]); ++i) nf[i] = (int32_t)mxGetDoubles(prhs[6])[i];
    plhs[0] = mxCreateDoubleMatrix(1, B, mxREAL);
    mxArray* g = nlhs > 1 ? mxCreateDoubleMatrix(Nhyp, B, mxREAL) : nullptr;
    vbmc_status st = vbmc_gp_nlz(g_ctx, N, D, B, Nhyp, (int)mxGetScalar(prhs[5]), nf, mxGetDoubles(X), mxGetDoubles(y), dbl(s2),
                                 mxGetDoubles(hyp), g ? 1 : 0, mxGetDoubles(plhs[0]), g ? mxGetDoubles(g) : nullptr);
    if (st != VBMC_OK) return fail(st);
    if (g) plhs[1] = g;
    return 0;
  }

  if (!strcmp(cmd, "slice_sample")) {
    if (nrhs < 16) return raise("vbmc_hip:usage", "slice_sample: X, y, s2, meanfun, noisefun, prior, LB, UB, hyp_start, widths, basewidths, options, seed, perms, U");
    const mxArray *X = prhs[1], *pr = prhs[6], *opt = prhs[12], *pm = prhs[14], *U = prhs[15];
    if (mxGetNumberOfElements(opt) < 5) return raise("vbmc_hip:usage", "slice_sample: options are [Ns Thin Burnin Adaptive W]");
    vbmc_slice_args a;
    memset(&a, 0, sizeof a);
    a.struct_size = sizeof a;
    a.N = (int)mxGetM(X); a.D = (int)mxGetN(X); a.Nhyp = (int)mxGetNumberOfElements(prhs[9]); a.meanfun = (int)mxGetScalar(prhs[4]);
    a.noisefun[0] = 1;
    for (int i = 0; i < 3 && i < (int)mxGetNumberOfElements(prhs[5]); ++i) a.noisefun[i] = (int32_t)mxGetDoubles(prhs[5])[i];
    a.X = mxGetDoubles(X); a.y = dbl(prhs[2]); a.s2 = dbl(prhs[3]);
    if (pr && !mxIsEmpty(pr) && mxIsStruct(pr)) { a.prior_mu = dbl(field(pr, "mu")); a.prior_sigma = dbl(field(pr, "sigma")); a.prior_df = dbl(field(pr, "df")); }
    a.LB = dbl(prhs[7]); a.UB = dbl(prhs[8]); a.hyp_start = dbl(prhs[9]); a.widths = dbl(prhs[10]); a.basewidths = dbl(prhs[11]);
    const double* o = mxGetDoubles(opt);
    a.Ns = (int)o[0]; a.Thin = (int)o[1]; a.Burnin = (int)o[2]; a.Adaptive = (int)o[3]; a.W = (int)o[4];
    const double seed = mxGetScalar(prhs[13]);
    if (!(seed >= 0.0 && seed <= 9007199254740992.0)) return raise("vbmc_hip:usage", "slice_sample: the seed must be an integer in 0 .. 2^53");
    a.seed = (uint64_t)seed;
    const size_t nh = (size_t)a.Nhyp;
    for (int i : {7, 8, 10})
      if (mxGetNumberOfElements(prhs[i]) != nh) return raise("vbmc_hip:usage", "slice_sample: LB, UB and widths need numel(hyp_start) entries");
    if (!mxIsEmpty(prhs[11]) && mxGetNumberOfElements(prhs[11]) != nh) return raise("vbmc_hip:usage", "slice_sample: basewidths needs numel(hyp_start) entries");
    if (pr && !mxIsEmpty(pr) && mxIsStruct(pr))
      for (const char* fn : {"mu", "sigma", "df"})
        if (field(pr, fn) && !mxIsEmpty(field(pr, fn)) && mxGetNumberOfElements(field(pr, fn)) != nh)
          return raise("vbmc_hip:usage", "slice_sample: prior.mu / sigma / df need numel(hyp_start) entries");
    std::vector<int32_t> perms;
    if (!mxIsEmpty(pm) && !mxIsEmpty(U)) {
      const size_t np = mxGetNumberOfElements(pm);
      const double sweeps = o[2] + o[0] + (o[0] - 1.0) * (o[1] - 1.0);
      if (o[0] < 1.0 || o[1] < 1.0 || o[2] < 0.0 || (double)np != sweeps * (double)nh || mxGetDimensions(U)[0] < 3 ||
          (double)mxGetNumberOfElements(U) != sweeps * (double)nh * (double)mxGetDimensions(U)[0])
        return raise("vbmc_hip:usage", "slice_sample: perms must be Nhyp x sweeps and U (2+Kmax) x Nhyp x sweeps, sweeps = Burnin + Ns + (Ns-1)*(Thin-1)");
      perms.resize(np);
      for (size_t i = 0; i < np; ++i) perms[i] = (int32_t)mxGetDoubles(pm)[i] - 1;
      a.rng_mode = 1; a.perms = perms.data(); a.uniforms = mxGetDoubles(U);
      a.Kmax = (int)mxGetDimensions(U)[0] - 2;
    }
    if (a.Ns < 1 || a.Nhyp < 1) return raise("vbmc_hip:usage", "slice_sample: Ns and numel(hyp_start) must be positive");
    plhs[0] = mxCreateDoubleMatrix(a.Ns, a.Nhyp, mxREAL);
    mxArray* lp = mxCreateDoubleMatrix(a.Ns, 1, mxREAL);
    mxArray* wo = mxCreateDoubleMatrix(1, a.Nhyp, mxREAL);
    mxArray* cn = mxCreateDoubleMatrix(1, 3, mxREAL);
    int64_t fc = 0, pf = 0;
    int32_t ms = 0;
    a.samples = mxGetDoubles(plhs[0]); a.logp = mxGetDoubles(lp); a.widths_out = mxGetDoubles(wo);
    a.funccount = &fc; a.performed = &pf; a.max_shrink = &ms;
    vbmc_status st = vbmc_gp_slice_sample(g_ctx, &a);
    if (st != VBMC_OK) { mxDestroyArray(lp); mxDestroyArray(wo); mxDestroyArray(cn); return fail(st); }
    mxGetDoubles(cn)[0] = (double)fc; mxGetDoubles(cn)[1] = (double)pf; mxGetDoubles(cn)[2] = (double)ms;
    if (nlhs > 1) plhs[1] = lp; else mxDestroyArray(lp);
    if (nlhs > 2) plhs[2] = wo; else mxDestroyArray(wo);
    if (nlhs > 3) plhs[3] = cn; else mxDestroyArray(cn);
    return 0;
  }

  if (!strcmp(cmd, "gp_train_opt")) {
    if (nrhs < 11) return raise("vbmc_hip:usage", "gp_train_opt: X, y, s2, meanfun, noisefun, prior, LB, UB, design, options");
    const mxArray *X = prhs[1], *pr = prhs[6], *des = prhs[9], *opt = prhs[10];
    if (mxGetNumberOfElements(opt) < 6) return raise("vbmc_hip:usage", "gp_train_opt: options are [Ninit Nopts TolFun MaxIter MaxFunEvals W]");
    const double* o = mxGetDoubles(opt);
    vbmc_gptrain_args a;
    memset(&a, 0, sizeof a);
    a.struct_size = sizeof a;
    a.N = (int)mxGetM(X); a.D = (int)mxGetN(X); a.Nhyp = (int)mxGetN(des); a.meanfun = (int)mxGetScalar(prhs[4]);
    a.noisefun[0] = 1;
    for (int i = 0; i < 3 && i < (int)mxGetNumberOfElements(prhs[5]); ++i) a.noisefun[i] = (int32_t)mxGetDoubles(prhs[5])[i];
    a.X = mxGetDoubles(X); a.y = dbl(prhs[2]); a.s2 = dbl(prhs[3]);
    if (pr && !mxIsEmpty(pr) && mxIsStruct(pr)) { a.prior_mu = dbl(field(pr, "mu")); a.prior_sigma = dbl(field(pr, "sigma")); a.prior_df = dbl(field(pr, "df")); }
    a.LB = dbl(prhs[7]); a.UB = dbl(prhs[8]); a.design = mxGetDoubles(des);
    const int rows = (int)mxGetM(des);
    a.Ninit = (int)o[0]; a.N0 = rows; a.Nopts = (int)o[1]; a.Ncov = a.D + 1; a.TolFun = o[2]; a.MaxIter = (int)o[3]; a.MaxFunEvals = (int)o[4];
    a.W = (int)o[5];
    const size_t nh = (size_t)a.Nhyp;
    if (a.Nhyp < 1 || rows < 1 || a.Nopts < 1 || (a.Ninit != 0 && a.Ninit != rows))
      return raise("vbmc_hip:usage", "gp_train_opt: the design is Ninit x Nhyp (Ninit = 0: hyp0' alone), Nopts is positive");
    for (int i : {7, 8})
      if (mxGetNumberOfElements(prhs[i]) != nh) return raise("vbmc_hip:usage", "gp_train_opt: LB and UB need one entry per column of the design");
    if (pr && !mxIsEmpty(pr) && mxIsStruct(pr))
      for (const char* fn : {"mu", "sigma", "df"})
        if (field(pr, fn) && !mxIsEmpty(field(pr, fn)) && mxGetNumberOfElements(field(pr, fn)) != nh)
          return raise("vbmc_hip:usage", "gp_train_opt: prior.mu / sigma / df need one entry per column of the design");
    mxArray* out[9];
    out[0] = mxCreateDoubleMatrix(a.Nhyp, a.Nopts, mxREAL);
    out[1] = mxCreateDoubleMatrix(1, a.Nopts, mxREAL);
    out[2] = mxCreateDoubleMatrix(a.Nhyp, 1, mxREAL);
    out[3] = mxCreateDoubleMatrix(1, 1, mxREAL);
    out[4] = mxCreateDoubleMatrix(1, a.Nhyp, mxREAL);
    out[5] = mxCreateDoubleMatrix(3, a.Nopts, mxREAL);
    out[6] = mxCreateDoubleMatrix(1, 1, mxREAL);
    out[7] = mxCreateDoubleMatrix(1, rows, mxREAL);
    out[8] = mxCreateDoubleMatrix(1, rows, mxREAL);
    vbmc_status st;
    {
      std::vector<int32_t> its(a.Nopts), ef(a.Nopts), ord(rows);
      std::vector<int64_t> fc(a.Nopts);
      int32_t best = 0;
      int64_t perf = 0;
      for (size_t i = 0; i < nh; ++i) mxGetDoubles(out[4])[i] = std::numeric_limits<double>::quiet_NaN();
      a.hyp = mxGetDoubles(out[0]); a.nll = mxGetDoubles(out[1]); a.hyp_start = mxGetDoubles(out[2]); a.best = &best;
      a.widths_default = mxGetDoubles(out[4]); a.iterations = its.data(); a.funccount = fc.data(); a.exitflag = ef.data(); a.performed = &perf;
      a.fill_fvals = mxGetDoubles(out[7]); a.fill_order = ord.data();
      st = vbmc_gp_train_optimize(g_ctx, &a);
      if (st == VBMC_OK) {
        mxGetDoubles(out[3])[0] = (double)best + 1.0;
        mxGetDoubles(out[6])[0] = (double)perf;
        for (int s = 0; s < a.Nopts; ++s) {
          mxGetDoubles(out[5])[3 * s] = (double)its[s]; mxGetDoubles(out[5])[3 * s + 1] = (double)fc[s]; mxGetDoubles(out[5])[3 * s + 2] = (double)ef[s];
        }
        for (int r = 0; r < rows; ++r) mxGetDoubles(out[8])[r] = (double)ord[r] + 1.0;
      }
    }
    if (st != VBMC_OK) { for (mxArray* m : out) mxDestroyArray(m); return fail(st); }
    plhs[0] = out[0];
    for (int i = 1; i < 9; ++i) { if (nlhs > i) plhs[i] = out[i]; else mxDestroyArray(out[i]); }
    return 0;
  }

  if (!strcmp(cmd, "gp_pred")) {
    vbmc_gp* h = (vbmc_gp*)(uintptr_t)(*(uint64_t*)mxGetData(prhs[1]));
    const mxArray* Xs = prhs[2];
    // vbmc_hip_mex('gp_pred', h, Xstar, ystar, s2star, ssflag, numel(gp.post))
    const int Nstar = (int)mxGetM(Xs), ss = (int)mxGetScalar(prhs[5]), S = (int)mxGetScalar(prhs[6]);
    const int nc = (ss && S > 1) ? S : 1;
    for (int i = 0; i < 4; ++i) plhs[i] = mxCreateDoubleMatrix(Nstar, nc, mxREAL);
    vbmc_status st = vbmc_gp_pred(g_ctx, h, Nstar, mxGetDoubles(Xs), dbl(prhs[3]), dbl(prhs[4]), ss || S == 1, mxGetDoubles(plhs[0]), mxGetDoubles(plhs[1]),
                                  mxGetDoubles(plhs[2]), mxGetDoubles(plhs[3]));
    if (st != VBMC_OK) return fail(st);
    return 0;
  }

  if (!strcmp(cmd, "sq_dist")) {
    const mxArray* a = prhs[1];
    const mxArray* b = (nrhs > 2 && !mxIsEmpty(prhs[2])) ? prhs[2] : nullptr;
    const int D = (int)mxGetM(a), n = (int)mxGetN(a), m = b ? (int)mxGetN(b) : n;
    if (b && (int)mxGetM(b) != D) return raise("vbmc_hip:sq_dist", "Error: column lengths must agree.");
    plhs[0] = mxCreateDoubleMatrix(n, m, mxREAL);
    vbmc_status st = vbmc_sq_dist(g_ctx, D, n, m, mxGetDoubles(a), b ? mxGetDoubles(b) : nullptr, mxGetDoubles(plhs[0]));
    if (st != VBMC_OK) return fail(st);
    return 0;
  }
  if (!strcmp(cmd, "vp_diag")) {     // [kl_mat,maxmtv_mat,mtv,xx] of vbmc_diagnostics.m:116-127 over the runs vp1, vp2, ... with the library's draws for seed: vbmc_vp_diagnostics
    if (nrhs < 4) return raise("vbmc_hip:usage", "vp_diag: Ns, seed, vp1, vp2, ...");
    const int R = nrhs - 3;
    std::vector<vbmc_vp_desc> d(R);
    std::vector<std::vector<int32_t>> t(R);
    std::vector<const vbmc_vp_desc*> p(R);
    for (int i = 0; i < R; ++i) {
      if (fill_vp_desc(d[i], prhs[3 + i], t[i])) return 1;
      p[i] = &d[i];
    }
    const double n = mxGetScalar(prhs[1]);
    if (!(n >= 1)) return raise("vbmc_hip:usage", "vp_diag: Ns must be positive");
    const mwSize Ns = (mwSize)n, dm[3] = {(mwSize)d[0].D, (mwSize)R, (mwSize)R}, dx[3] = {Ns, (mwSize)d[0].D, (mwSize)R};
    plhs[0] = mxCreateDoubleMatrix(R, R, mxREAL);
    if (nlhs > 1) plhs[1] = mxCreateDoubleMatrix(R, R, mxREAL);
    if (nlhs > 2) plhs[2] = mxCreateNumericArray(3, dm, mxDOUBLE_CLASS, mxREAL);
    if (nlhs > 3) plhs[3] = mxCreateNumericArray(3, dx, mxDOUBLE_CLASS, mxREAL);
    vbmc_diag_args a;
    memset(&a, 0, sizeof a);
    a.struct_size = sizeof a;
    a.Ns = (int64_t)Ns;
    a.seed = (uint64_t)mxGetScalar(prhs[2]);
    a.kl_mat = mxGetDoubles(plhs[0]);
    a.maxmtv_mat = nlhs > 1 ? mxGetDoubles(plhs[1]) : nullptr;
    a.mtv = nlhs > 2 ? mxGetDoubles(plhs[2]) : nullptr;
    a.xx = nlhs > 3 ? mxGetDoubles(plhs[3]) : nullptr;
    vbmc_status st = vbmc_vp_diagnostics(g_ctx, R, p.data(), &a);
    if (st != VBMC_OK) return fail(st);
    return 0;
  }
  return raise("vbmc_hip:usage", "unknown command");
}

void mexFunction(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
  g_err_id[0] = 0;
  if (dispatch(nlhs, plhs, nrhs, prhs)) mexErrMsgIdAndTxt(g_err_id, "%s", g_err_msg);   // no C++ object alive here
}

// vbmc_hip_mex.cpp -- MEX gateway from MATLAB to libvbmc_hip.so (include/vbmc_hip.h).
//
// Build (on a machine with MATLAB + ROCm; cannot be built in the development container, which has
// neither MATLAB nor mex.h -- this file is deliberately free of numerics):
//     mex -R2018a vbmc_hip_mex.cpp -I../include -L../vbmc_amd/lib -lvbmc_hip
//
// The .m shims in this directory call [out1, ...] = vbmc_hip_mex('<command>', arg1, ...).  The commands are the rows of commands[] near the end of
// this file: name, least argument count, leading device handles, usage string (the arguments, by name), handler, flags.  The comment above each handler
// cmd_<name> says what the command returns and what its arguments mean.  A new command is a handler and a row.
//  * Handles: a device-resident gp.post and the state of the importance sampler travel as uint64 scalars, the replicas of 'gp_upload_all' as a
//    1 x n uint64 row; dispatch() refuses anything else in a handle slot.  The context is kept in a persistent, mexLock'ed.
//  * Error ids: 'vbmc_hip:usage' for a call the gateway refuses itself (too few arguments: the message is "<command>: <usage>"), 'vbmc_hip:nodevice',
//    'vbmc_hip:abi', 'vbmc_hip:error', or the reference's own id where the library's message starts with one.  VBMC_ERR_UNSUPPORTED becomes
//    'vbmc_hip:unsupported', which the shims catch to fall through to the reference .m implementation (SURVEY.md 8b "Errors").
//  * mexErrMsgIdAndTxt long-jumps out of the MEX function without running C++ destructors, so it is called from exactly one place -- mexFunction
//    itself, which owns no C++ object -- after dispatch() has RETURNED (all std::vector / std::string temporaries of the handler destroyed) with
//    the id and message parked in static character buffers.
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
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

static int raise(const char* id, const char* fmt, ...) {   // printf-style message
  snprintf(g_err_id, sizeof g_err_id, "%s", id);
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err_msg, sizeof g_err_msg, fmt, ap);
  va_end(ap);
  return 1;
}

// "<name>: <usage>" of the command that dispatch() is running (defined below the table)
static int usage_error();

// library status -> pending MATLAB error; returns nonzero so that call sites read `if (st != VBMC_OK) return fail(st);`
static int fail(vbmc_status st) {
  const char* msg = g_ctx ? vbmc_last_error(g_ctx) : "no context";
  if (st == VBMC_ERR_UNSUPPORTED) return raise("vbmc_hip:unsupported", "%s", msg);
  // messages of INVALID errors start with the reference's own error id where one exists ("gplogjoint:FullVarianceGradient ...")
  const char* sp = strchr(msg, ' ');
  const char* col = strchr(msg, ':');
  if (st == VBMC_ERR_INVALID && sp && col && col < sp && (size_t)(sp - msg) < sizeof g_err_id) {
    memcpy(g_err_id, msg, (size_t)(sp - msg));
    g_err_id[sp - msg] = 0;
    snprintf(g_err_msg, sizeof g_err_msg, "%s", sp + 1);
    return 1;
  }
  return raise("vbmc_hip:error", "%s", msg);
}

static int done(vbmc_status st) { return st == VBMC_OK ? 0 : fail(st); }   // the last line of a handler

// status of a communicator call -> pending MATLAB error
static int fail_comm(vbmc_status st) {
  const char* msg = g_comm ? vbmc_comm_last_error(g_comm) : "no communicator";
  return raise(st == VBMC_ERR_UNSUPPORTED ? "vbmc_hip:unsupported" : "vbmc_hip:error", "%s", msg);
}

// the session on ndev devices: the communicator owns one context per device, g_ctx is its device-0 context
static int open_comm(int ndev, const char* why_not) {
  if (vbmc_comm_create_all(ndev, nullptr, &g_comm) != VBMC_OK) { g_comm = nullptr; return raise("vbmc_hip:nodevice", "%s", why_not); }
  g_ctx = vbmc_comm_ctx(g_comm, 0);
  mexLock();
  mexAtExit(at_exit);
  return 0;
}

static int ensure_ctx(int device) {
  if (g_ctx) return 0;
  // VBMC_HIP_DEVICES=n (n >= 2) in the environment: the session opens on n devices, as 'comm_open' n would
  const char* nd = getenv("VBMC_HIP_DEVICES");
  if (nd && atoi(nd) >= 2) return open_comm(atoi(nd), "libvbmc_hip: VBMC_HIP_DEVICES asks for more gfx950 devices than could be opened (or librccl is missing)");
  vbmc_status st = vbmc_ctx_create(device, nullptr, &g_ctx);
  if (st != VBMC_OK) return raise("vbmc_hip:nodevice", "libvbmc_hip: no gfx950 (MI355X) device available");
  mexLock();
  mexAtExit(at_exit);
  return 0;
}

// ---- helpers shared by the handlers

// device handles travel as uint64 scalars; anything else (a double that lost its class on the way) must not be dereferenced
static bool is_handle(const mxArray* a) { return a && mxGetClassID(a) == mxUINT64_CLASS && mxGetNumberOfElements(a) >= 1; }
template <class T> static T* handle_in(const mxArray* a, size_t i = 0) { return (T*)(uintptr_t)((const uint64_t*)mxGetData(a))[i]; }
template <class T> static mxArray* handles_out(T* const* p, int n = 1) {   // 1 x n uint64
  mxArray* a = mxCreateNumericMatrix(1, n, mxUINT64_CLASS, mxREAL);
  for (int i = 0; i < n; ++i) ((uint64_t*)mxGetData(a))[i] = (uint64_t)(uintptr_t)p[i];
  return a;
}

// outputs i, i + 1, ... go to the caller as far as it asked for them; the others are destroyed here
static void give(int nlhs, mxArray* plhs[], int i, std::initializer_list<mxArray*> xs) {
  for (mxArray* x : xs) {
    if (nlhs > i) plhs[i] = x;
    else if (x) mxDestroyArray(x);
    ++i;
  }
}

static const double* dbl(const mxArray* a) { return (a && !mxIsEmpty(a)) ? mxGetDoubles(a) : nullptr; }
static const mxArray* field(const mxArray* s, const char* name) { return mxGetField(s, 0, name); }
static double scalar_field(const mxArray* s, const char* name, double dflt) {
  const mxArray* f = field(s, name);
  return (f && !mxIsEmpty(f)) ? mxGetScalar(f) : dflt;
}

// an args struct of the C ABI, zeroed, with its struct_size set
template <class A> static A zeroed() {
  A a;
  memset(&a, 0, sizeof a);
  a.struct_size = sizeof a;
  return a;
}

// gp.noisefun (up to three entries; missing ones are those of the constant-noise model) -> int32_t[3]
static void read_noisefun(const mxArray* nfa, int32_t nf[3]) {
  nf[0] = 1; nf[1] = 0; nf[2] = 0;
  for (int i = 0; nfa && i < 3 && i < (int)mxGetNumberOfElements(nfa); ++i) nf[i] = (int32_t)mxGetDoubles(nfa)[i];
}

// the options of the ensemble sampler -> the members that every args struct which runs it has; the defaults mean "the library's own"
template <class A> static void read_sampler_opts(A& a, const mxArray* op) {
  a.thin = (int)scalar_field(op, "Thin", 1.0); a.burnin = (int)scalar_field(op, "Burnin", -1.0);
  a.spec = (int)scalar_field(op, "Spec", 0.0); a.max_steps = (int)scalar_field(op, "MaxSteps", 0.0); a.max_shrink = (int)scalar_field(op, "MaxShrink", 0.0);
  a.chunk = (int)scalar_field(op, "Chunk", 0.0); a.seed = (uint64_t)scalar_field(op, "Seed", 0.0);
}

// opts.U, the uniforms of the ensemble sampler in parity mode (64 x H x S x Mmax, H = W / 2) -> a.U and a.Mmax; a.U stays null without one
template <class A> static int read_sampler_uniforms(A& a, const mxArray* op, int W, int S, const char* cmd) {
  const mxArray* u = field(op, "U");
  if (!u || mxIsEmpty(u)) return 0;
  const size_t nu = mxGetNumberOfElements(u), per = (size_t)64 * (size_t)(W / 2) * (size_t)S;
  if (per == 0 || nu % per != 0) return raise("vbmc_hip:usage", "%s: opts.U must be 64 x H x S x Mmax", cmd);
  a.U = mxGetDoubles(u); a.Mmax = (int)(nu / per);
  return 0;
}

// the hyper-prior struct (mu, sigma, df; anything but a non-empty struct: no prior) -> a.prior_mu / prior_sigma / prior_df, each empty or of nh entries
template <class A> static int read_prior(A& a, const mxArray* pr, size_t nh, const char* cmd, const char* need) {
  if (!pr || mxIsEmpty(pr) || !mxIsStruct(pr)) return 0;
  for (const char* fn : {"mu", "sigma", "df"})
    if (field(pr, fn) && !mxIsEmpty(field(pr, fn)) && mxGetNumberOfElements(field(pr, fn)) != nh)
      return raise("vbmc_hip:usage", "%s: prior.mu / sigma / df need %s", cmd, need);
  a.prior_mu = dbl(field(pr, "mu")); a.prior_sigma = dbl(field(pr, "sigma")); a.prior_df = dbl(field(pr, "df"));
  return 0;
}

// the mixture of a vp struct: K and its four arrays
struct Mixture { int K; const double *mu, *sigma, *lambda, *w; };
// ... with K as vp.K says it (null where a field is missing or empty; the library refuses those)
static Mixture mixture(const mxArray* vp) {
  return {(int)scalar_field(vp, "K", 0), dbl(field(vp, "mu")), dbl(field(vp, "sigma")), dbl(field(vp, "lambda")), dbl(field(vp, "w"))};
}
// ... with D and K as the size of vp.mu says them.  Returns 0, 1 if a field is missing, 2 if sigma, w (K) or lambda (D) disagree with mu
static int sized_mixture(const mxArray* vp, int& D, Mixture& m) {
  const mxArray *mu = field(vp, "mu"), *sg = field(vp, "sigma"), *lm = field(vp, "lambda"), *ww = field(vp, "w");
  if (!mu || !sg || !lm || !ww || mxIsEmpty(mu)) return 1;
  D = (int)mxGetM(mu);
  m = {(int)mxGetN(mu), nullptr, nullptr, nullptr, nullptr};
  if (mxGetNumberOfElements(sg) != (size_t)m.K || mxGetNumberOfElements(ww) != (size_t)m.K || mxGetNumberOfElements(lm) != (size_t)D) return 2;
  m.mu = mxGetDoubles(mu); m.sigma = mxGetDoubles(sg); m.lambda = mxGetDoubles(lm); m.w = mxGetDoubles(ww);
  return 0;
}
// vp.delta (gplogjoint.m:85-89) -> D values, none for an empty field; neither a scalar nor a D-vector: 'vbmc_hip:unsupported', the reference cannot evaluate it either
static int read_delta(const mxArray* vp, int D, std::vector<double>& delta, const char* msg) {
  const mxArray* dl = field(vp, "delta");
  const size_t nd = dl ? mxGetNumberOfElements(dl) : 0;
  if (nd == 0) return 0;
  if (nd != 1 && nd != (size_t)D) return raise("vbmc_hip:unsupported", "%s", msg);
  if (nd == 1) delta.assign(D, mxGetScalar(dl));
  else delta.assign(mxGetDoubles(dl), mxGetDoubles(dl) + D);
  return 0;
}

// a 1 x 1 struct of n double fields, field i rows[i] x cols[i] and returned in f[i]; rows[i] < 0: left to the caller (f[i] null)
static mxArray* out_struct(int n, const char** names, const int* rows, const int* cols, mxArray** f) {
  mxArray* out = mxCreateStructMatrix(1, 1, n, names);
  for (int i = 0; i < n; ++i) {
    f[i] = rows[i] < 0 ? nullptr : mxCreateDoubleMatrix(rows[i], cols[i], mxREAL);
    if (f[i]) mxSetField(out, 0, names[i], f[i]);
  }
  return out;
}

// vp struct + thetabnd -> the parameter-layout part of vbmc_elbo_args (shared by 'elbo', 'elbo_batch', 'adam')
static int fill_vp_args(vbmc_elbo_args& a, const mxArray* vp, const mxArray* tb, std::vector<double>& delta) {
  a = zeroed<vbmc_elbo_args>();
  const Mixture m = mixture(vp);
  a.D = (int)scalar_field(vp, "D", 0); a.K = m.K; a.R = 1;
  a.optimize[0] = scalar_field(vp, "optimize_mu", 1) != 0; a.optimize[1] = scalar_field(vp, "optimize_sigma", 1) != 0;
  a.optimize[2] = scalar_field(vp, "optimize_lambda", 1) != 0; a.optimize[3] = scalar_field(vp, "optimize_weights", 0) != 0;
  a.vp_mu = m.mu; a.vp_sigma = m.sigma; a.vp_lambda = m.lambda; a.vp_w = m.w;
  if (read_delta(vp, a.D, delta, "vp.delta has neither one entry nor D")) return 1;
  if (!delta.empty()) a.vp_delta = delta.data();
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
  read_noisefun(field(gp, "noisefun"), g.nf);
  g.Ncov = (int)scalar_field(gp, "Ncov", g.D + 1); g.Nnoise = (int)scalar_field(gp, "Nnoise", 1);
  g.meanfun = (int)scalar_field(gp, "meanfun", 4);
}

// vp struct with its trinfo (shared/warpvars_vbmc.m: lb_orig, ub_orig, type, mu, delta, scale, R_mat; empty: the identity) -> vbmc_vp_desc
// (shared by 'vp_pdf', 'vp_rnd', 'vp_moments', 'vp_kldiv', 'vp_mtv', 'vp_diag', 'vp_corner').  The arrays stay MATLAB's; only the types are converted to int32.
static int fill_vp_desc(vbmc_vp_desc& d, const mxArray* vp, std::vector<int32_t>& types) {
  d = zeroed<vbmc_vp_desc>();
  if (!vp || !mxIsStruct(vp)) return raise("vbmc_hip:usage", "vp must be a variational-posterior struct");
  int D0 = 0;
  Mixture m;
  const int bad = sized_mixture(vp, D0, m);
  if (bad == 1) return raise("vbmc_hip:usage", "vp needs mu, sigma, lambda and w");
  d.D = (int32_t)D0; d.K = (int32_t)m.K;
  if (bad) return raise("vbmc_hip:usage", "vp.mu must be D x K with K sigmas and weights and D lambdas");
  d.mu = m.mu; d.sigma = m.sigma; d.lambda = m.lambda; d.w = m.w;
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

// ---- the commands.  A handler returns 0 on success, nonzero with g_err_id / g_err_msg set.  dispatch() has counted the arguments
// (min_nrhs of the row), checked the handle slots and, unless the row says NO_CTX, created the context before it is called.

// -> struct max_D, max_K, max_N, max_Na, max_T_vargrad, delta_ok, meanfun: the shapes the library accepts (vbmc_get_limits: a host function, no device), for vbmc_hip_supported.m
static int cmd_limits(int, mxArray* plhs[], int, const mxArray*[]) {
  vbmc_limits lim = zeroed<vbmc_limits>();
  if (vbmc_get_limits(&lim) != VBMC_OK) return raise("vbmc_hip:abi", "vbmc_get_limits refused the struct (ABI mismatch)");
  int nm = 0;
  for (int i = 0; i < 31; ++i) nm += (lim.meanfun_mask >> i) & 1;
  const char* names[] = {"max_D", "max_K", "max_N", "max_Na", "max_T_vargrad", "delta_ok", "meanfun"};
  const int rows[7] = {1, 1, 1, 1, 1, 1, 1}, cols[7] = {1, 1, 1, 1, 1, 1, nm};
  mxArray* f[7];
  plhs[0] = out_struct(7, names, rows, cols, f);
  const double v[6] = {(double)lim.max_D, (double)lim.max_K, (double)lim.max_N, (double)lim.max_Na, (double)lim.max_T_vargrad, (double)lim.delta_ok};
  for (int i = 0; i < 6; ++i) mxGetDoubles(f[i])[0] = v[i];
  for (int i = 0, j = 0; i < 31; ++i) if ((lim.meanfun_mask >> i) & 1) mxGetDoubles(f[6])[j++] = i;
  return 0;
}

// -> [surrogates uploaded from the host, posteriors built on the device and kept, rank-one appends kept] since the gateway was loaded
static int cmd_stats(int, mxArray* plhs[], int, const mxArray*[]) {
  plhs[0] = mxCreateDoubleMatrix(1, 3, mxREAL);
  for (int i = 0; i < 3; ++i) mxGetDoubles(plhs[0])[i] = (double)g_stats[i];
  return 0;
}

// creates the context on the given device (0 without one); nothing to do once there is a context
static int cmd_open(int, mxArray*[], int nrhs, const mxArray* prhs[]) { return ensure_ctx(nrhs > 1 ? (int)mxGetScalar(prhs[1]) : 0); }

// -> n, the devices opened.  Every GPU of the node from ONE MATLAB process (the communicator inside the library, include/vbmc_hip.h): a context and an RCCL rank per device.
// Must be the first command of the session; the single-device commands then run on device 0.  VBMC_HIP_DEVICES=ndev in the environment does the same implicitly
static int cmd_comm_open(int, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
  if (g_comm || g_ctx) return raise("vbmc_hip:usage", "comm_open must be the first command of the session");
  if (open_comm(nrhs > 1 ? (int)mxGetScalar(prhs[1]) : 1, "libvbmc_hip: could not open the requested gfx950 devices / librccl")) return 1;
  plhs[0] = mxCreateDoubleScalar(vbmc_comm_size(g_comm));
  return 0;
}

// -> n, the devices of the session (1 without a communicator)
static int cmd_comm_size(int, mxArray* plhs[], int, const mxArray*[]) {
  plhs[0] = mxCreateDoubleScalar(g_comm ? vbmc_comm_size(g_comm) : 1);
  return 0;
}

// -> h, the uint64 handle of a device-resident gp.post made from the gp struct of gplite_post.m; freed with 'gp_free'
static int cmd_gp_upload(int, mxArray* plhs[], int, const mxArray* prhs[]) {
  GpArrays g;
  read_gp(prhs[1], g);
  vbmc_gp* h = nullptr;
  vbmc_status st = vbmc_gp_upload(g_ctx, g.N, g.D, g.S, g.Nhyp, g.Ncov, g.Nnoise, g.meanfun, g.X, g.hyp.data(), g.alpha.data(),
                                  g.L.data(), g.sW1.data(), g.lch.data(), &h);
  if (st == VBMC_OK) st = vbmc_gp_set_noise(g_ctx, h, g.nf, g.mult.data());
  if (st != VBMC_OK) return fail(st);
  ++g_stats[0];
  plhs[0] = handles_out(&h);
  return 0;
}

// -> hs, 1 x n uint64 handles, one replica per device of the communicator (hs(1): device 0); freed with 'gp_free_all'
static int cmd_gp_upload_all(int, mxArray* plhs[], int, const mxArray* prhs[]) {
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
  plhs[0] = handles_out(hs.data(), n);
  return 0;
}

// frees the replicas of 'gp_upload_all' (nothing to do without a communicator)
static int cmd_gp_free_all(int, mxArray*[], int, const mxArray* prhs[]) {
  if (!g_comm) return 0;
  const int n = vbmc_comm_local(g_comm);
  std::vector<vbmc_gp*> hs(n, nullptr);
  for (int i = 0; i < n && i < (int)mxGetNumberOfElements(prhs[1]); ++i) hs[i] = handle_in<vbmc_gp>(prhs[1], i);
  vbmc_gp_free_all(g_comm, hs.data());
  return 0;
}

// frees the device posterior of 'gp_upload', 'gp_post' or 'gp_rank1'
static int cmd_gp_free(int, mxArray*[], int, const mxArray* prhs[]) { vbmc_gp_free(g_ctx, handle_in<vbmc_gp>(prhs[1])); return 0; }

// -> [F,dF,G,H,varG,dH,varGss,I_sk,J_sjk,dG,G_s,varG_s,dvarG,dG_s,dvarG_s], those not computed 0 x 0: one ELCBO evaluation at theta.  thetabnd, eps: or [].  eps: the D x Ns/2 x K
// block the shim drew with randn (parity mode); without one the device stream keyed by seed.  numel(gp.post) sizes I_sk (S x K) and J_sjk (S x K x K), and G_s, varG_s, dG_s, dvarG_s
// (T x S): the per-hyper-sample outputs of gplogjoint(...,avg_flag = 0).  no_jacobian = 1: gradients with respect to sigma, lambda, w themselves, the JACOBIAN_FLAG = 0 form of
// entmc_vbmc / entlb_vbmc / gplogjoint
static int cmd_elbo(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
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
  const auto nS = [&] { return (int)mxGetScalar(prhs[12]); };   // numel(gp.post), read only where an output is sized by it
  mxArray *Isk = nullptr, *Jsjk = nullptr;
  if (a.separate_K) {
    // S is known to the library; query through a first call would cost a launch, so the shim passes numel(gp.post)
    if (nrhs < 13) return raise("vbmc_hip:usage", "elbo with separate_K needs numel(gp.post) as its 13th argument");
    const int S = nS();
    Isk = mxCreateDoubleMatrix(S, a.K, mxREAL);
    a.I_sk = mxGetDoubles(Isk);
    if (a.compute_var) { mwSize dims[3] = {(mwSize)S, (mwSize)a.K, (mwSize)a.K}; Jsjk = mxCreateNumericArray(3, dims, mxDOUBLE_CLASS, mxREAL); a.J_sjk = mxGetDoubles(Jsjk); }
  }
  mxArray *Gs = nullptr, *vGs = nullptr;
  if (nlhs > 10 && nrhs > 12) {   // per-hyper-sample values (gplogjoint avg_flag = 0)
    Gs = mxCreateDoubleMatrix(1, nS(), mxREAL);
    a.G_s = mxGetDoubles(Gs);
    if (nlhs > 11 && a.compute_var) { vGs = mxCreateDoubleMatrix(1, nS(), mxREAL); a.varG_s = mxGetDoubles(vGs); }
  }
  mxArray* dvG = nullptr;         // 13th output: gradient of the diagonal variance (dvarF of misc/gplogjoint.m:27)
  if (nlhs > 12 && a.compute_grad && a.compute_var == 2) { dvG = mxCreateDoubleMatrix(T, 1, mxREAL); a.dvarG = mxGetDoubles(dvG); }
  mxArray* dGs = nullptr;         // 14th output: the gradient per hyper-sample, T x S (gplogjoint's dF with avg_flag = 0, misc/gplogjoint.m:411 skipped)
  if (nlhs > 13 && a.compute_grad && nrhs > 12) { dGs = mxCreateDoubleMatrix(T, nS(), mxREAL); a.dG_s = mxGetDoubles(dGs); }
  mxArray* dvGs = nullptr;        // 15th output (ABI 5): the variance gradient per hyper-sample, T x S (gplogjoint's dvarF with avg_flag = 0, :407-409 skipped)
  if (nlhs > 14 && a.compute_grad && a.compute_var == 2 && nrhs > 12) { dvGs = mxCreateDoubleMatrix(T, nS(), mxREAL); a.dvarG_s = mxGetDoubles(dvGs); }
  vbmc_status st = vbmc_elbo_batch(g_ctx, handle_in<vbmc_gp>(prhs[1]), &a);
  if (st != VBMC_OK) return fail(st);  // MATLAB frees the mxArrays created above on error
  mxArray* outs[15] = {F, dF, G, H, vG, dH, vss, Isk, Jsjk, dG, Gs, vGs, dvG, dGs, dvGs};
  for (int i = 0; i < 15 && (i < nlhs || i == 0); ++i) plhs[i] = outs[i] ? outs[i] : mxCreateDoubleMatrix(0, 0, mxREAL);
  return 0;
}

// -> [F,dF,varG,G,H,varGss,I_sk,J_sjk] of the R = size(Theta,2) candidates of vpsieve_vbmc.m:74-78, or of the 2*Nslowopts eval_fullelcbo calls of vpoptimize_vbmc.m:134,165, in
// one pass.  The candidates share vp's flags and its non-optimised groups; the device MC stream is keyed by (seed, r).  thetabnd: or [].  I_sk is S x K x R, J_sjk S x K x K x R.
// 'elbo_batch_multi' takes the 1 x n handles of 'gp_upload_all': the candidates are dealt r = g (mod n) over the devices and their ELCBO values all-gathered over xGMI; every
// value is bit-identical to 'elbo_batch' on one device
static int elbo_batch_body(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[], bool multi) {
  if (multi && !g_comm) return raise("vbmc_hip:usage", "elbo_batch_multi needs 'comm_open' first");
  std::vector<const vbmc_gp*> hs;
  if (multi) {
    if ((int)mxGetNumberOfElements(prhs[1]) != vbmc_comm_local(g_comm)) return raise("vbmc_hip:usage", "elbo_batch_multi: one handle per device");
    for (int i = 0; i < vbmc_comm_local(g_comm); ++i) hs.push_back(handle_in<vbmc_gp>(prhs[1], i));
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
    vbmc_status st = vbmc_elbo_batch(g_ctx, handle_in<vbmc_gp>(prhs[1]), &a);
    if (st != VBMC_OK) return fail(st);
  }
  mxArray* outs[8] = {F, dF, vG, G, H, vss, Isk, Jsjk};
  for (int i = 0; i < 8 && (i < nlhs || i == 0); ++i) plhs[i] = outs[i] ? outs[i] : mxCreateDoubleMatrix(0, 0, mxREAL);
  return 0;
}
static int cmd_elbo_batch(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) { return elbo_batch_body(nlhs, plhs, nrhs, prhs, false); }
static int cmd_elbo_batch_multi(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) { return elbo_batch_body(nlhs, plhs, nrhs, prhs, true); }

// -> [x,f,iters,xmid,xtab,ftab]: fminadam.m on the device, one chain per column of Theta0 (T x R).  thetabnd: or [].  steps: [step_min step_max step_decay].  xmid T x R: each
// chain's iterate of smallest recorded objective, vpoptimize_vbmc.m:133; the tables only on request: xtab T x MaxIter x R, ftab MaxIter x R, the first iters(r) entries of chain r filled
static int cmd_adam(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
  const mxArray* Theta = prhs[2];
  vbmc_elbo_args a;
  std::vector<double> delta;
  if (fill_vp_args(a, prhs[3], prhs[7], delta)) return 1;
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
  vbmc_status st = vbmc_adam_batch(g_ctx, handle_in<vbmc_gp>(prhs[1]), &a, TolFun, MaxIter, step[0], step[1], step[2], mxGetDoubles(x), mxGetDoubles(f),
                                   (int32_t*)mxGetData(it), xtab ? mxGetDoubles(xtab) : nullptr, ftab ? mxGetDoubles(ftab) : nullptr,
                                   xmid ? mxGetDoubles(xmid) : nullptr);
  if (st != VBMC_OK) return fail(st);
  plhs[0] = x;
  give(nlhs, plhs, 1, {f, it, xmid, xtab, ftab});
  return 0;
}

// -> [alpha,L,sW,sn2_mult,Lchol,h]: gplite_post for the S columns of hyp (s2: or []).  The device posterior is kept only if its handle h is asked for
static int cmd_gp_post(int nlhs, mxArray* plhs[], int, const mxArray* prhs[]) {
  const mxArray *hyp = prhs[1], *X = prhs[2], *y = prhs[3], *s2 = prhs[4];
  const int N = (int)mxGetM(X), D = (int)mxGetN(X), Nhyp = (int)mxGetM(hyp), S = (int)mxGetN(hyp);
  int32_t nf[3];
  read_noisefun(prhs[6], nf);
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
  give(nlhs, plhs, 1, {L, sW, mult, lch});
  if (nlhs > 5) { plhs[5] = handles_out(&h); ++g_stats[1]; }
  else vbmc_gp_free(g_ctx, h);
  return 0;
}

// -> [alpha (N+1 x S), L (N+1 x N+1 x S), hnew]: one training point appended by a rank-one update.  Xnew: all N+1 points; mstar, vstar: or []; sn2_eff: one per hyper-sample.
// The new device posterior is kept only if hnew is asked for
static int cmd_gp_rank1(int nlhs, mxArray* plhs[], int, const mxArray* prhs[]) {
  const mxArray* Xn = prhs[2];
  const int N1 = (int)mxGetM(Xn), S = (int)mxGetNumberOfElements(prhs[6]);
  mwSize ld[3] = {(mwSize)N1, (mwSize)N1, (mwSize)S};
  plhs[0] = mxCreateDoubleMatrix(N1, S, mxREAL);
  mxArray* L = mxCreateNumericArray(3, ld, mxDOUBLE_CLASS, mxREAL);
  vbmc_gp* hn = nullptr;
  vbmc_status st = vbmc_gp_rank1_update(g_ctx, handle_in<vbmc_gp>(prhs[1]), mxGetDoubles(Xn), mxGetScalar(prhs[3]), dbl(prhs[4]), dbl(prhs[5]),
                                        mxGetDoubles(prhs[6]), mxGetDoubles(plhs[0]), nlhs > 1 ? mxGetDoubles(L) : nullptr, &hn);
  if (st != VBMC_OK) return fail(st);
  give(nlhs, plhs, 1, {L});
  if (nlhs > 2) { plhs[2] = handles_out(&hn); ++g_stats[2]; }
  else vbmc_gp_free(g_ctx, hn);
  return 0;
}

// -> [acq,fbar,vtot], Nstar x 1 each: the acquisition function acq_id at the rows of Xs; the last three arguments only for acqfsn2
static int cmd_acq(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
  const mxArray* Xs = prhs[2];
  const Mixture m = mixture(prhs[4]);
  const int Nstar = (int)mxGetM(Xs);
  plhs[0] = mxCreateDoubleMatrix(Nstar, 1, mxREAL);
  mxArray *fb = mxCreateDoubleMatrix(Nstar, 1, mxREAL), *vt = mxCreateDoubleMatrix(Nstar, 1, mxREAL);
  vbmc_status st = vbmc_acq_eval(g_ctx, handle_in<vbmc_gp>(prhs[1]), Nstar, mxGetDoubles(Xs), (int)mxGetScalar(prhs[3]), m.K, m.mu, m.sigma, m.lambda, m.w,
                                 mxGetScalar(prhs[5]), (int)mxGetScalar(prhs[6]), mxGetScalar(prhs[7]),
                                 nrhs > 8 ? dbl(prhs[8]) : nullptr, nrhs > 9 ? dbl(prhs[9]) : nullptr, nrhs > 10 ? dbl(prhs[10]) : nullptr,
                                 mxGetDoubles(plhs[0]), mxGetDoubles(fb), mxGetDoubles(vt));
  if (st != VBMC_OK) return fail(st);
  give(nlhs, plhs, 1, {fb, vt});
  return 0;
}

// -> [acq,fbar,vtot]: 'acq' with vp.delta > 0: mean and variance per hyper-sample from gplite_quad(gp,Xs,delta,1), acqwrapper_vbmc.m:12-14; delta: D values; the last three only for acqfsn2
static int cmd_acq_delta(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
  const mxArray* Xs = prhs[2];
  const Mixture m = mixture(prhs[4]);
  const int Nstar = (int)mxGetM(Xs), D = (int)mxGetN(Xs);
  if ((int)mxGetNumberOfElements(prhs[8]) != D) return raise("vbmc_hip:usage", "acq_delta: delta must hold one value per dimension");
  plhs[0] = mxCreateDoubleMatrix(Nstar, 1, mxREAL);
  mxArray *fb = mxCreateDoubleMatrix(Nstar, 1, mxREAL), *vt = mxCreateDoubleMatrix(Nstar, 1, mxREAL);
  vbmc_status st = vbmc_acq_eval_delta(g_ctx, handle_in<vbmc_gp>(prhs[1]), Nstar, mxGetDoubles(Xs), (int)mxGetScalar(prhs[3]), m.K, m.mu, m.sigma, m.lambda, m.w,
                                       mxGetScalar(prhs[5]), (int)mxGetScalar(prhs[6]), mxGetScalar(prhs[7]),
                                       nrhs > 9 ? dbl(prhs[9]) : nullptr, nrhs > 10 ? dbl(prhs[10]) : nullptr, nrhs > 11 ? dbl(prhs[11]) : nullptr,
                                       mxGetDoubles(plhs[0]), mxGetDoubles(fb), mxGetDoubles(vt), mxGetDoubles(prhs[8]));
  give(nlhs, plhs, 1, {fb, vt});
  return done(st);
}

// -> [xmin,fmin,out]: the CMA-ES acquisition search on the device (vbmc_acq_search, matlab/vbmc_hip_acqsearch.m).  opts: TolX, TolFun, TolHistFun, MaxFunEvals, MaxIter, PopSize, Seed,
// Chunk, Z (D x lambda x Gmax: parity mode); out: the bestever point and value, the final xmean / sigma / C, evals, generations, stop (1 TolX .. 5 MaxIter), behind.
// 'acq_search_iqr': the same opts and out on the IQR functions (vbmc_acq_search_iqr, matlab/vbmc_hip_acqsearch_iqr.m); from var_regularized on the arguments sit where acq_search has them
static int acq_search_body(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[], bool search_iqr) {
  if (!mxIsStruct(prhs[search_iqr ? 4 : 3]) || !mxIsStruct(prhs[11])) return usage_error();
  vbmc_gp* h = handle_in<vbmc_gp>(prhs[1]);
  const mxArray *vp = prhs[search_iqr ? 4 : 3], *op = prhs[11];
  const int D = (int)mxGetNumberOfElements(prhs[7]);
  for (int i = 8; i <= 10; ++i)
    if ((int)mxGetNumberOfElements(prhs[i]) != D) return raise("vbmc_hip:usage", "acq_search: x0, insigma, LB and UB must hold one value per dimension");
  if (D < 1 || !field(vp, "lambda") || (int)mxGetNumberOfElements(field(vp, "lambda")) != D)
    return raise("vbmc_hip:usage", "acq_search: vp.lambda must hold one value per dimension");
  vbmc_acqsearch_args a = zeroed<vbmc_acqsearch_args>();
  const Mixture m = mixture(vp);
  a.acq_id = (int)mxGetScalar(prhs[search_iqr ? 3 : 2]); a.K = m.K;
  a.vp_mu = m.mu; a.vp_sigma = m.sigma; a.vp_lambda = m.lambda; a.vp_w = m.w;
  std::vector<double> delta;
  if (read_delta(vp, D, delta, "acq_search: vp.delta must be empty, a scalar or one value per dimension")) return 1;
  if (!delta.empty()) a.vp_delta = delta.data();
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
  const int rows[9] = {D, 1, D, 1, D, 1, 1, 1, 1}, cols[9] = {1, 1, 1, 1, D, 1, 1, 1, 1};
  mxArray* f[9];
  mxArray* out = out_struct(9, names, rows, cols, f);
  plhs[0] = mxCreateDoubleMatrix(D, 1, mxREAL);
  mxArray* fmin = mxCreateDoubleMatrix(1, 1, mxREAL);
  int64_t evals = 0, rounds[2] = {0, 0};
  int32_t gens = 0, stop = 0;
  a.xmin = mxGetDoubles(plhs[0]); a.fmin = mxGetDoubles(fmin);
  a.xbest = mxGetDoubles(f[0]); a.fbest = mxGetDoubles(f[1]); a.xmean = mxGetDoubles(f[2]); a.sigma = mxGetDoubles(f[3]); a.C = mxGetDoubles(f[4]);
  a.evals = &evals; a.generations = &gens; a.stop = &stop; a.rounds = rounds;
  vbmc_status st = search_iqr ? vbmc_acq_search_iqr(g_ctx, h, handle_in<vbmc_acq_is>(prhs[2]), &a) : vbmc_acq_search(g_ctx, h, &a);
  mxGetDoubles(f[5])[0] = (double)evals; mxGetDoubles(f[6])[0] = gens; mxGetDoubles(f[7])[0] = stop; mxGetDoubles(f[8])[0] = (double)rounds[1];
  give(nlhs, plhs, 1, {fmin, out});
  return done(st);
}
static int cmd_acq_search(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) { return acq_search_body(nlhs, plhs, nrhs, prhs, false); }
static int cmd_acq_search_iqr(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) { return acq_search_body(nlhs, plhs, nrhs, prhs, true); }

// -> [F,varF]: gplite_quad at the rows of mu; sigma 1 x D, or Nstar x D of equal rows
static int cmd_gp_quad(int nlhs, mxArray* plhs[], int, const mxArray* prhs[]) {
  const mxArray *mu = prhs[2], *sg = prhs[3];
  const int Nstar = (int)mxGetM(mu), D = (int)mxGetN(mu), ss = (int)mxGetScalar(prhs[4]), S = (int)mxGetScalar(prhs[5]);
  const int rows = (int)mxGetM(sg);
  if ((int)mxGetN(sg) != D || (rows != 1 && rows != Nstar)) return raise("vbmc_hip:usage", "gp_quad: sigma must be 1 x D or Nstar x D");
  const int nc = (ss && S > 1) ? S : 1;
  plhs[0] = mxCreateDoubleMatrix(Nstar, nc, mxREAL);
  mxArray* vf = nlhs > 1 ? mxCreateDoubleMatrix(Nstar, nc, mxREAL) : nullptr;
  vbmc_status st = vbmc_gp_quad(g_ctx, handle_in<vbmc_gp>(prhs[1]), Nstar, mxGetDoubles(mu), mxGetDoubles(sg), rows, ss || S == 1, mxGetDoubles(plhs[0]),
                                vf ? mxGetDoubles(vf) : nullptr);
  if (vf) plhs[1] = vf;
  return done(st);
}

// -> [Xa,lnw,fs2a,his,out]: the MCMC of the IMIQR importance sampler on the device (vbmc_acq_is_sample, matlab/vbmc_hip_importance_sample.m).  x0: W x D x S.  opts: Thin, Burnin, Spec,
// MaxSteps, MaxShrink, Seed, Chunk, U (64 x H x S x Mmax: parity mode); out: logp, funccount, performed, rounds, behind; his: the state of those device buffers, freed with 'is_free'
static int cmd_acq_is_sample(int nlhs, mxArray* plhs[], int, const mxArray* prhs[]) {
  if (!mxIsStruct(prhs[6])) return usage_error();
  const mxArray *x0 = prhs[2], *op = prhs[6];
  const mwSize nd = mxGetNumberOfDimensions(x0);
  const mwSize* dm = mxGetDimensions(x0);
  const int W = (int)dm[0], D = (int)dm[1], S = nd > 2 ? (int)dm[2] : 1, Nm = (int)mxGetScalar(prhs[5]);
  if ((int)mxGetNumberOfElements(prhs[3]) != D || (int)mxGetNumberOfElements(prhs[4]) != D || Nm < 1)
    return raise("vbmc_hip:usage", "acq_is_sample: x0 must be W x D x S, LB and UB must hold one value per dimension, Nm must be positive");
  vbmc_is_sample_args a = zeroed<vbmc_is_sample_args>();
  a.W = W; a.D = D; a.S = S; a.Nm = Nm;
  read_sampler_opts(a, op);
  a.x0 = mxGetDoubles(x0); a.LB = dbl(prhs[3]); a.UB = dbl(prhs[4]);
  if (read_sampler_uniforms(a, op, W, S, "acq_is_sample")) return 1;
  if (a.U) a.rng_mode = 1;
  const mwSize dx[3] = {(mwSize)Nm, (mwSize)D, (mwSize)S};
  mxArray* Xa = mxCreateNumericArray(3, dx, mxDOUBLE_CLASS, mxREAL);
  mxArray* lnw = mxCreateDoubleMatrix(S, Nm, mxREAL);
  mxArray* fs2a = mxCreateDoubleMatrix(Nm, S, mxREAL);
  const char* names[] = {"logp", "funccount", "performed", "rounds", "behind"};
  const int rows[5] = {S, 1, 1, 1, 1}, cols[5] = {Nm, 1, 1, 1, 1};
  mxArray* f[5];
  mxArray* out = out_struct(5, names, rows, cols, f);
  int64_t funccount = 0, performed = 0, rounds[2] = {0, 0};
  vbmc_acq_is* is = nullptr;
  a.Xa = mxGetDoubles(Xa); a.lnw = mxGetDoubles(lnw); a.fs2a = mxGetDoubles(fs2a); a.logp = mxGetDoubles(f[0]);
  a.funccount = &funccount; a.performed = &performed; a.rounds = rounds;
  if (nlhs > 3) a.state = &is;
  vbmc_status st = vbmc_acq_is_sample(g_ctx, handle_in<vbmc_gp>(prhs[1]), &a);
  mxGetDoubles(f[1])[0] = (double)funccount; mxGetDoubles(f[2])[0] = (double)performed;
  mxGetDoubles(f[3])[0] = (double)rounds[0]; mxGetDoubles(f[4])[0] = (double)rounds[1];
  plhs[0] = Xa;
  give(nlhs, plhs, 1, {lnw, fs2a});
  if (nlhs > 3) plhs[3] = handles_out(&is);
  give(nlhs, plhs, 4, {out});
  return done(st);
}

// -> his: the ActiveImportanceSampling state (Xa and, each or [], lnw, fs2a, Ctmp) on the device, for 'acq_iqr' and 'acq_search_iqr'; freed with 'is_free'
static int cmd_is_create(int, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
  const mxArray* Xa = prhs[2];
  const mwSize nd = mxGetNumberOfDimensions(Xa);
  const int Na = (int)mxGetDimensions(Xa)[0];
  vbmc_acq_is* is = nullptr;
  vbmc_status st = vbmc_acq_is_create(g_ctx, handle_in<vbmc_gp>(prhs[1]), Na, mxGetDoubles(Xa), nd > 2 ? 1 : 0, nrhs > 3 ? dbl(prhs[3]) : nullptr,
                                      nrhs > 4 ? dbl(prhs[4]) : nullptr, nrhs > 5 ? dbl(prhs[5]) : nullptr, &is);
  if (st != VBMC_OK) return fail(st);
  plhs[0] = handles_out(&is);
  return 0;
}

// frees the state of 'is_create', 'acq_is_sample' or 'is_setup'
static int cmd_is_free(int, mxArray*[], int, const mxArray* prhs[]) { vbmc_acq_is_free(g_ctx, handle_in<vbmc_acq_is>(prhs[1])); return 0; }

// -> [Xa,lnw,fs2a,his,out]: the whole set-up of the IMIQR importance sampler in one call (vbmc_acq_is_setup, matlab/vbmc_hip_importance_setup.m).  opts: S, Thin, Burnin, Spec, MaxSteps,
// MaxShrink, Seed, Chunk, W (0: 2 (D + 1)), B (the Step 1 block: parity mode), U (64 x H x S x Mmax, with B); out: Xa1, lnw1, fs2a1, lpdf1, rect_delta, LB, UB, x0 (W x D x S), idx0
// (W x S, 0-based), n_bad, bad (W x S), logp, funccount, performed, rounds, behind; n_bad > 0: Xa, lnw, fs2a are zeros and his is 0; Nm = 0: Step 1 alone, his the state of the Na1 shared points
static int cmd_is_setup(int nlhs, mxArray* plhs[], int, const mxArray* prhs[]) {
  if (!mxIsStruct(prhs[2]) || !mxIsStruct(prhs[6])) return usage_error();
  const mxArray *vp = prhs[2], *op = prhs[6];
  int D = 0;
  Mixture m;
  const int bad_vp = sized_mixture(vp, D, m);
  if (bad_vp == 1) return raise("vbmc_hip:usage", "is_setup: vp needs mu, sigma, lambda and w");
  const int K = m.K, S = (int)scalar_field(op, "S", 0.0);
  const int Nvp = (int)mxGetScalar(prhs[3]), Nbox = (int)mxGetScalar(prhs[4]), Nm = (int)mxGetScalar(prhs[5]);
  if (bad_vp || S < 1 || Nm < 0 || Nvp < 0 || Nbox < 0 || Nvp + Nbox < 1)
    return raise("vbmc_hip:usage", "is_setup: vp.mu must be D x K with K sigmas and weights and D lambdas, opts.S = numel(gp.post), the counts non-negative");
  vbmc_is_setup_args a = zeroed<vbmc_is_setup_args>();
  a.D = D; a.S = S; a.K = K; a.Nvp = Nvp; a.Nbox = Nbox; a.Nm = Nm;
  a.vp_mu = m.mu; a.vp_sigma = m.sigma; a.vp_lambda = m.lambda; a.vp_w = m.w;
  a.W = (int)scalar_field(op, "W", 0.0);
  if (a.W == 0) a.W = 2 * (D + 1);
  const int W = a.W, Na1 = Nvp + Nbox;
  if (W < 0) return raise("vbmc_hip:usage", "is_setup: opts.W must be positive");
  read_sampler_opts(a, op);
  if (const mxArray* b = field(op, "B")) {
    if (!mxIsEmpty(b)) {
      if (mxGetNumberOfElements(b) != (size_t)(D + 1) * Na1 + (Nm > 0 ? (size_t)W * S : 0)) return raise("vbmc_hip:usage", "is_setup: opts.B must hold (D + 1) (Nvp + Nbox) + W S values");
      a.rng_mode = 1; a.B = mxGetDoubles(b);
      if (read_sampler_uniforms(a, op, W, S, "is_setup")) return 1;
    }
  }
  const mwSize dx[3] = {(mwSize)Nm, (mwSize)D, (mwSize)S}, d0[3] = {(mwSize)W, (mwSize)D, (mwSize)S};
  mxArray* Xa = mxCreateNumericArray(3, dx, mxDOUBLE_CLASS, mxREAL);
  mxArray* lnw = mxCreateDoubleMatrix(S, Nm, mxREAL);
  mxArray* fs2a = mxCreateDoubleMatrix(Nm, S, mxREAL);
  const char* names[] = {"Xa1", "lnw1", "fs2a1", "lpdf1", "rect_delta", "LB", "UB", "x0", "idx0", "n_bad", "bad", "logp", "funccount", "performed", "rounds", "behind"};
  enum { oXa1, oLnw1, oFs2a1, oLpdf1, oRd, oLB, oUB, oX0, oIdx0, oNbad, oBad, oLogp, oFc, oPf, oRounds, oBehind, oCount };
  const int rows[oCount] = {Na1, S, Na1, Na1, D, D, D, -1, W, 1, W, S, 1, 1, 1, 1}, cols[oCount] = {D, Na1, S, 1, 1, 1, 1, -1, S, 1, S, Nm, 1, 1, 1, 1};
  mxArray* f[oCount];
  mxArray* out = out_struct(oCount, names, rows, cols, f);
  f[oX0] = mxCreateNumericArray(3, d0, mxDOUBLE_CLASS, mxREAL);   // the one field of three dimensions
  mxSetField(out, 0, names[oX0], f[oX0]);
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
  vbmc_status st = vbmc_acq_is_setup(g_ctx, handle_in<vbmc_gp>(prhs[1]), &a);
  for (size_t j = 0; j < (size_t)W * S; ++j) { mxGetDoubles(f[oIdx0])[j] = (double)idx0[j]; mxGetDoubles(f[oBad])[j] = (double)bad[j]; }
  mxGetDoubles(f[oNbad])[0] = (double)n_bad;
  mxGetDoubles(f[oFc])[0] = (double)funccount; mxGetDoubles(f[oPf])[0] = (double)performed;
  mxGetDoubles(f[oRounds])[0] = (double)rounds[0]; mxGetDoubles(f[oBehind])[0] = (double)rounds[1];
  plhs[0] = Xa;
  give(nlhs, plhs, 1, {lnw, fs2a});
  if (nlhs > 3) plhs[3] = handles_out(&is);
  give(nlhs, plhs, 4, {out});
  return done(st);
}

// -> [y,dy] = vbmc_pdf(vp,X,origflag,logflag,transflag,df) through vp.trinfo: vbmc_vp_pdf, matlab/vbmc_hip_pdf.m
static int cmd_vp_pdf(int nlhs, mxArray* plhs[], int, const mxArray* prhs[]) {
  vbmc_vp_desc d;
  std::vector<int32_t> ty;
  if (fill_vp_desc(d, prhs[1], ty)) return 1;
  const mxArray* X = prhs[2];
  if (!mxIsDouble(X) || (int)mxGetN(X) != d.D) return raise("vbmc_hip:usage", "vp_pdf: X must be N x D");
  const mwSize N = mxGetM(X);
  plhs[0] = mxCreateDoubleMatrix(N, 1, mxREAL);
  double* dy = nlhs > 1 ? mxGetDoubles(plhs[1] = mxCreateDoubleMatrix(N, d.D, mxREAL)) : nullptr;
  return done(vbmc_vp_pdf(g_ctx, &d, (int64_t)N, dbl(X), mxGetScalar(prhs[3]) != 0, mxGetScalar(prhs[4]) != 0, mxGetScalar(prhs[5]) != 0, mxGetScalar(prhs[6]),
                          mxGetDoubles(plhs[0]), dy));
}

// -> [X,I] = vbmc_rnd(vp,N,origflag,balanceflag,df) with the library's draws for seed, I counted from 0: vbmc_vp_rnd, matlab/vbmc_hip_rnd.m
static int cmd_vp_rnd(int nlhs, mxArray* plhs[], int, const mxArray* prhs[]) {
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
  return done(st);
}

// -> [mubar,Sigma] = vbmc_moments(vp,1,Ns) with the library's draws for seed: vbmc_vp_moments, matlab/vbmc_hip_moments.m
static int cmd_vp_moments(int nlhs, mxArray* plhs[], int, const mxArray* prhs[]) {
  vbmc_vp_desc d;
  std::vector<int32_t> ty;
  if (fill_vp_desc(d, prhs[1], ty)) return 1;
  plhs[0] = mxCreateDoubleMatrix(1, d.D, mxREAL);
  double* S = nlhs > 1 ? mxGetDoubles(plhs[1] = mxCreateDoubleMatrix(d.D, d.D, mxREAL)) : nullptr;
  return done(vbmc_vp_moments(g_ctx, &d, (int64_t)mxGetScalar(prhs[2]), (uint64_t)mxGetScalar(prhs[3]), nullptr, mxGetDoubles(plhs[0]), S));
}

// 'vp_kldiv' -> [kls,xx1,xx2] = vbmc_kldiv(vp1,vp2,Ns,0), 'vp_mtv' -> [mtv,xx1,xx2] = vbmc_mtv(vp1,vp2,Ns), with the library's draws for seed: vbmc_vp_kldiv and
// vbmc_vp_mtv, matlab/vbmc_hip_kldiv.m and matlab/vbmc_hip_mtv.m.  xx1, xx2: the Ns draws from either posterior
static int vp_pair_body(int nlhs, mxArray* plhs[], const mxArray* prhs[], bool mtv) {
  vbmc_vp_desc d1, d2;
  std::vector<int32_t> t1, t2;
  if (fill_vp_desc(d1, prhs[1], t1) || fill_vp_desc(d2, prhs[2], t2)) return 1;
  const double n = mxGetScalar(prhs[3]);
  if (!(n >= 1)) return raise("vbmc_hip:usage", "%s: Ns must be positive", mtv ? "vp_mtv" : "vp_kldiv");
  const mwSize Ns = (mwSize)n;
  const uint64_t seed = (uint64_t)mxGetScalar(prhs[4]);
  plhs[0] = mxCreateDoubleMatrix(1, mtv ? d1.D : 2, mxREAL);
  double *x1 = nullptr, *x2 = nullptr;
  if (nlhs > 1) x1 = mxGetDoubles(plhs[1] = mxCreateDoubleMatrix(Ns, d1.D, mxREAL));
  if (nlhs > 2) x2 = mxGetDoubles(plhs[2] = mxCreateDoubleMatrix(Ns, d1.D, mxREAL));
  if (!mtv) return done(vbmc_vp_kldiv(g_ctx, &d1, &d2, (int64_t)Ns, seed, nullptr, nullptr, mxGetDoubles(plhs[0]), x1, x2));
  vbmc_mtv_args a = zeroed<vbmc_mtv_args>();
  a.Ns = (int64_t)Ns; a.seed = seed; a.mtv = mxGetDoubles(plhs[0]); a.xx1 = x1; a.xx2 = x2;
  return done(vbmc_vp_mtv(g_ctx, &d1, &d2, &a));
}
static int cmd_vp_kldiv(int nlhs, mxArray* plhs[], int, const mxArray* prhs[]) { return vp_pair_body(nlhs, plhs, prhs, false); }
static int cmd_vp_mtv(int nlhs, mxArray* plhs[], int, const mxArray* prhs[]) { return vp_pair_body(nlhs, plhs, prhs, true); }

// -> [kl_mat,maxmtv_mat,mtv,xx] of vbmc_diagnostics.m:116-127 over the runs vp1, vp2, ... with the library's draws for seed: vbmc_vp_diagnostics, matlab/vbmc_hip_diagnostics.m
static int cmd_vp_diag(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
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
  vbmc_diag_args a = zeroed<vbmc_diag_args>();
  a.Ns = (int64_t)Ns; a.seed = (uint64_t)mxGetScalar(prhs[2]);
  a.kl_mat = mxGetDoubles(plhs[0]); a.maxmtv_mat = nlhs > 1 ? mxGetDoubles(plhs[1]) : nullptr;
  a.mtv = nlhs > 2 ? mxGetDoubles(plhs[2]) : nullptr; a.xx = nlhs > 3 ? mxGetDoubles(plhs[3]) : nullptr;
  return done(vbmc_vp_diagnostics(g_ctx, R, p.data(), &a));
}

// -> [x,fval,idx] of vbmc_mode(vp,nmax,origflag): the mode (1 x D), its log density and the winning start (from 0): vbmc_vp_mode, matlab/vbmc_hip_mode.m
static int cmd_vp_mode(int nlhs, mxArray* plhs[], int, const mxArray* prhs[]) {
  vbmc_vp_desc d;
  std::vector<int32_t> ty;
  if (fill_vp_desc(d, prhs[1], ty)) return 1;
  plhs[0] = mxCreateDoubleMatrix(1, d.D, mxREAL);
  mxArray* fval = mxCreateDoubleMatrix(1, 1, mxREAL);
  mxArray* idx = mxCreateDoubleMatrix(1, 1, mxREAL);
  int32_t won = 0;
  vbmc_mode_args a = zeroed<vbmc_mode_args>();
  a.nmax = (int32_t)mxGetScalar(prhs[2]); a.origflag = mxGetScalar(prhs[3]) != 0; a.tol_grad = mxGetScalar(prhs[4]);
  a.x = mxGetDoubles(plhs[0]); a.fval = mxGetDoubles(fval); a.idx = &won;
  const vbmc_status st = vbmc_vp_mode(g_ctx, &d, &a);
  mxGetDoubles(idx)[0] = (double)won;
  give(nlhs, plhs, 1, {fval, idx});
  return done(st);
}

// -> [xx,bounds,hist,quant,density,bandwidth,tstar,counts2]: the data of cornerplot (utils/cornerplot.m:113-156) for Ns draws of vp with the library's draws for
// seed, or, with vp = [], for the rows of the sample matrix X (else X = []): vbmc_vp_corner, matlab/vbmc_hip_cornerdata.m.  bounds: [] or 2 x D as cornerplot takes
// them; res, nbins: 0 for cornerplot's own 64 and 40; p: the probabilities of quant (nq x D).  hist (nbins x D) and counts2 (res x res x P) are counts as doubles;
// density is res x res x P, page pp what kde2d returns for pair pp; bandwidth 2 x P; tstar 1 x P
static int cmd_vp_corner(int nlhs, mxArray* plhs[], int, const mxArray* prhs[]) {
  vbmc_vp_desc d;
  std::vector<int32_t> ty;
  const bool given = mxIsEmpty(prhs[1]);
  vbmc_corner_args a = zeroed<vbmc_corner_args>();
  if (given) {
    if (mxIsEmpty(prhs[2]) || !mxIsDouble(prhs[2])) return raise("vbmc_hip:usage", "vp_corner: a variational posterior or a matrix of samples");
    a.X_in = mxGetDoubles(prhs[2]); a.D = (int32_t)mxGetN(prhs[2]); a.Ns = (int64_t)mxGetM(prhs[2]);
  } else {
    if (fill_vp_desc(d, prhs[1], ty)) return 1;
    if (!mxIsEmpty(prhs[2])) return raise("vbmc_hip:usage", "vp_corner: a variational posterior or a matrix of samples, not both");
    const double n = mxGetScalar(prhs[3]);
    if (!(n >= 1)) return raise("vbmc_hip:usage", "vp_corner: Ns must be positive");
    a.D = d.D; a.Ns = (int64_t)n;
  }
  const mwSize D = (mwSize)a.D, Ns = (mwSize)a.Ns, P = D * (D - 1) / 2;
  if (D < 1 || D > 32) return raise("vbmc_hip:unsupported", "vp_corner: D = %d outside 1 .. 32 not accelerated", (int)D);
  a.seed = (uint64_t)mxGetScalar(prhs[4]); a.origflag = 1; a.balanceflag = mxGetScalar(prhs[5]) != 0;
  if (!mxIsEmpty(prhs[6])) {
    if (mxGetNumberOfElements(prhs[6]) != 2 * D) return raise("vbmc_hip:usage", "vp_corner: bounds must be 2 x D");
    a.bounds = mxGetDoubles(prhs[6]);
  }
  a.res = (int32_t)mxGetScalar(prhs[7]); a.nbins = (int32_t)mxGetScalar(prhs[8]);
  a.nq = (int32_t)mxGetNumberOfElements(prhs[9]); a.p = dbl(prhs[9]);
  const mwSize n = a.res == 0 ? 64 : (mwSize)a.res, nb = a.nbins == 0 ? 40 : (mwSize)a.nbins;
  if ((n != 16 && n != 32 && n != 64) || nb < 1 || nb > 1024 || a.nq > 16) {   // the library words the refusal; nothing is sized from these
    const vbmc_status st = vbmc_vp_corner(g_ctx, given ? nullptr : &d, &a);
    return st == VBMC_OK ? raise("vbmc_hip:error", "vp_corner: the library accepted res = %d, nbins = %d", a.res, a.nbins) : fail(st);
  }
  const mwSize d3[3] = {n, n, P};
  std::vector<int32_t> hist((size_t)nb * D), cnt(nlhs > 7 ? (size_t)n * n * P : 0);
  plhs[0] = mxCreateDoubleMatrix(Ns, D, mxREAL);
  mxArray *bo = mxCreateDoubleMatrix(2, D, mxREAL), *hi = mxCreateDoubleMatrix(nb, D, mxREAL), *qu = mxCreateDoubleMatrix(a.nq, D, mxREAL);
  mxArray *de = mxCreateNumericArray(3, d3, mxDOUBLE_CLASS, mxREAL), *bw = mxCreateDoubleMatrix(2, P, mxREAL), *ts = mxCreateDoubleMatrix(1, P, mxREAL);
  mxArray* c2 = nlhs > 7 ? mxCreateNumericArray(3, d3, mxDOUBLE_CLASS, mxREAL) : nullptr;
  a.xx = mxGetDoubles(plhs[0]); a.bounds_out = mxGetDoubles(bo); a.hist = hist.data(); a.quant = mxGetDoubles(qu);
  a.density = mxGetDoubles(de); a.bandwidth = mxGetDoubles(bw); a.tstar = mxGetDoubles(ts); a.counts2 = c2 ? cnt.data() : nullptr;
  const vbmc_status st = vbmc_vp_corner(g_ctx, given ? nullptr : &d, &a);
  for (size_t i = 0; i < hist.size(); ++i) mxGetDoubles(hi)[i] = (double)hist[i];
  for (size_t i = 0; i < cnt.size(); ++i) mxGetDoubles(c2)[i] = (double)cnt[i];
  give(nlhs, plhs, 1, {bo, hi, qu, de, bw, ts, c2});
  return done(st);
}

// -> [acq,fbar,vtot], Nstar x 1 each: the IQR acquisition functions at the rows of Xs; his: the state of 'is_create'
static int cmd_acq_iqr(int nlhs, mxArray* plhs[], int, const mxArray* prhs[]) {
  vbmc_acq_is* is = handle_in<vbmc_acq_is>(prhs[2]);
  const mxArray* Xs = prhs[3];
  const int Nstar = (int)mxGetM(Xs);
  plhs[0] = mxCreateDoubleMatrix(Nstar, 1, mxREAL);
  mxArray *fb = mxCreateDoubleMatrix(Nstar, 1, mxREAL), *vt = mxCreateDoubleMatrix(Nstar, 1, mxREAL);
  vbmc_status st = vbmc_acq_iqr_eval(g_ctx, handle_in<vbmc_gp>(prhs[1]), is, Nstar, mxGetDoubles(Xs), dbl(prhs[4]), dbl(prhs[5]), dbl(prhs[6]),
                                     (int)mxGetScalar(prhs[7]), mxGetScalar(prhs[8]), mxGetDoubles(plhs[0]), mxGetDoubles(fb), mxGetDoubles(vt));
  if (st != VBMC_OK) return fail(st);
  give(nlhs, plhs, 1, {fb, vt});
  return 0;
}

// -> [X,out]: gpsample_vbmc(vp,gp,Ns,origflag) with the library's draws for opts.Seed (vbmc_gp_surrogate_sample, matlab/gpsample_vbmc.m).  noise: struct X_rescaled, gplengthscale, sn2new,
// or [].  opts: S, E, W, Seed, Thin, Burnin, Spec, Chunk, Nnn, Beta, VarThresh, x0 (W x D x E); out: VarThresh, sn2_avg, funccount, performed, rounds, behind
static int cmd_gp_surrogate_sample(int nlhs, mxArray* plhs[], int, const mxArray* prhs[]) {
  if (!mxIsStruct(prhs[8])) return usage_error();
  vbmc_vp_desc d;
  std::vector<int32_t> ty;
  const bool have_vp = mxIsStruct(prhs[2]);
  if (have_vp && fill_vp_desc(d, prhs[2], ty)) return 1;
  const mxArray *nz = prhs[7], *op = prhs[8];
  const double n = mxGetScalar(prhs[3]);
  const int D = (int)mxGetNumberOfElements(prhs[5]);
  if (!(n >= 1) || D < 1 || (int)mxGetNumberOfElements(prhs[6]) != D || (have_vp && d.D != D))
    return raise("vbmc_hip:usage", "gp_surrogate_sample: Ns must be positive, LB and UB must hold one value per dimension of vp");
  vbmc_gs_args a = zeroed<vbmc_gs_args>();
  a.D = D; a.S = (int)scalar_field(op, "S", 1.0); a.Ns = (int64_t)n; a.origflag = mxGetScalar(prhs[4]) != 0;
  a.E = (int)scalar_field(op, "E", 1.0); a.W = (int)scalar_field(op, "W", 0.0);
  read_sampler_opts(a, op);
  a.Nnn = (int)scalar_field(op, "Nnn", 0.0);
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
  const int ones[6] = {1, 1, 1, 1, 1, 1};
  mxArray* f[6];
  mxArray* out = out_struct(6, names, ones, ones, f);
  int64_t funccount = 0, performed = 0, rounds[2] = {0, 0};
  a.X = mxGetDoubles(plhs[0]); a.varthresh_out = mxGetDoubles(f[0]); a.sn2_avg_out = mxGetDoubles(f[1]);
  a.funccount = &funccount; a.performed = &performed; a.rounds = rounds;
  vbmc_status st = vbmc_gp_surrogate_sample(g_ctx, handle_in<vbmc_gp>(prhs[1]), have_vp ? &d : nullptr, &a);
  mxGetDoubles(f[2])[0] = (double)funccount; mxGetDoubles(f[3])[0] = (double)performed;
  mxGetDoubles(f[4])[0] = (double)rounds[0]; mxGetDoubles(f[5])[0] = (double)rounds[1];
  give(nlhs, plhs, 1, {out});
  return done(st);
}

// -> [nlZ,dnlZ]: gplite_nlZ for the B columns of Hyp (s2: or [])
static int cmd_gp_nlz(int nlhs, mxArray* plhs[], int, const mxArray* prhs[]) {
  const mxArray *hyp = prhs[1], *X = prhs[2], *y = prhs[3], *s2 = prhs[4];
  const int N = (int)mxGetM(X), D = (int)mxGetN(X), Nhyp = (int)mxGetM(hyp), B = (int)mxGetN(hyp);
  int32_t nf[3];
  read_noisefun(prhs[6], nf);
  plhs[0] = mxCreateDoubleMatrix(1, B, mxREAL);
  mxArray* g = nlhs > 1 ? mxCreateDoubleMatrix(Nhyp, B, mxREAL) : nullptr;
  vbmc_status st = vbmc_gp_nlz(g_ctx, N, D, B, Nhyp, (int)mxGetScalar(prhs[5]), nf, mxGetDoubles(X), mxGetDoubles(y), dbl(s2),
                               mxGetDoubles(hyp), g ? 1 : 0, mxGetDoubles(plhs[0]), g ? mxGetDoubles(g) : nullptr);
  if (st != VBMC_OK) return fail(st);
  if (g) plhs[1] = g;
  return 0;
}

// -> [samples,logp,widths,counts]: slicesamplebnd on -gplite_nlZ + log prior, the chain on the device (vbmc_gp_slice_sample).  prior: struct mu, sigma, df, or []; basewidths: or [];
// options: [Ns Thin Burnin Adaptive W]; perms: Nhyp x sweeps, column s = randperm(Nhyp)' of sweep s, 1-based; U: (2+Kmax) x Nhyp x sweeps; both empty: the device generator keyed
// by seed.  counts = [funccount performed max_shrink]
static int cmd_slice_sample(int nlhs, mxArray* plhs[], int, const mxArray* prhs[]) {
  const mxArray *X = prhs[1], *opt = prhs[12], *pm = prhs[14], *U = prhs[15];
  if (mxGetNumberOfElements(opt) < 5) return raise("vbmc_hip:usage", "slice_sample: options are [Ns Thin Burnin Adaptive W]");
  vbmc_slice_args a = zeroed<vbmc_slice_args>();
  a.N = (int)mxGetM(X); a.D = (int)mxGetN(X); a.Nhyp = (int)mxGetNumberOfElements(prhs[9]); a.meanfun = (int)mxGetScalar(prhs[4]);
  read_noisefun(prhs[5], a.noisefun);
  a.X = mxGetDoubles(X); a.y = dbl(prhs[2]); a.s2 = dbl(prhs[3]);
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
  if (read_prior(a, prhs[6], nh, "slice_sample", "numel(hyp_start) entries")) return 1;
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
  give(nlhs, plhs, 1, {lp, wo, cn});
  return 0;
}

// -> [hyp,nll,hyp_start,best,widths_default,counts,performed,fill_fvals,fill_order]: the optimisation half of gplite_train, gplite_train.m:200-306, on the device
// (vbmc_gp_train_optimize).  prior: struct mu, sigma, df, or []; options: [Ninit Nopts TolFun MaxIter MaxFunEvals W]; design (rows x Nhyp): the points fminfill evaluates, hyp0' in its
// first rows -- the caller builds it, fminfill.m:42-101; Ninit = 0: the rows are the caller's hyp0 alone (:249-256) and widths_default comes back NaN.  hyp Nhyp x Nopts, counts
// 3 x Nopts = [iterations; funccount; exitflag], best and fill_order 1-based
static int cmd_gp_train_opt(int nlhs, mxArray* plhs[], int, const mxArray* prhs[]) {
  const mxArray *X = prhs[1], *des = prhs[9], *opt = prhs[10];
  if (mxGetNumberOfElements(opt) < 6) return raise("vbmc_hip:usage", "gp_train_opt: options are [Ninit Nopts TolFun MaxIter MaxFunEvals W]");
  const double* o = mxGetDoubles(opt);
  vbmc_gptrain_args a = zeroed<vbmc_gptrain_args>();
  a.N = (int)mxGetM(X); a.D = (int)mxGetN(X); a.Nhyp = (int)mxGetN(des); a.meanfun = (int)mxGetScalar(prhs[4]);
  read_noisefun(prhs[5], a.noisefun);
  a.X = mxGetDoubles(X); a.y = dbl(prhs[2]); a.s2 = dbl(prhs[3]);
  a.LB = dbl(prhs[7]); a.UB = dbl(prhs[8]); a.design = mxGetDoubles(des);
  const int rows = (int)mxGetM(des);
  a.Ninit = (int)o[0]; a.N0 = rows; a.Nopts = (int)o[1]; a.Ncov = a.D + 1; a.TolFun = o[2]; a.MaxIter = (int)o[3]; a.MaxFunEvals = (int)o[4];
  a.W = (int)o[5];
  const size_t nh = (size_t)a.Nhyp;
  if (a.Nhyp < 1 || rows < 1 || a.Nopts < 1 || (a.Ninit != 0 && a.Ninit != rows))
    return raise("vbmc_hip:usage", "gp_train_opt: the design is Ninit x Nhyp (Ninit = 0: hyp0' alone), Nopts is positive");
  for (int i : {7, 8})
    if (mxGetNumberOfElements(prhs[i]) != nh) return raise("vbmc_hip:usage", "gp_train_opt: LB and UB need one entry per column of the design");
  if (read_prior(a, prhs[6], nh, "gp_train_opt", "one entry per column of the design")) return 1;
  const int orows[9] = {a.Nhyp, 1, a.Nhyp, 1, 1, 3, 1, 1, 1}, ocols[9] = {a.Nopts, a.Nopts, 1, 1, a.Nhyp, a.Nopts, 1, rows, rows};
  mxArray* out[9];
  for (int i = 0; i < 9; ++i) out[i] = mxCreateDoubleMatrix(orows[i], ocols[i], mxREAL);
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
  give(nlhs, plhs, 1, {out[1], out[2], out[3], out[4], out[5], out[6], out[7], out[8]});
  return 0;
}

// -> [ymu,ys2,fmu,fs2]: gplite_pred at the rows of Xstar (ystar, s2star: or [])
static int cmd_gp_pred(int, mxArray* plhs[], int, const mxArray* prhs[]) {
  const mxArray* Xs = prhs[2];
  const int Nstar = (int)mxGetM(Xs), ss = (int)mxGetScalar(prhs[5]), S = (int)mxGetScalar(prhs[6]);
  const int nc = (ss && S > 1) ? S : 1;
  for (int i = 0; i < 4; ++i) plhs[i] = mxCreateDoubleMatrix(Nstar, nc, mxREAL);
  return done(vbmc_gp_pred(g_ctx, handle_in<vbmc_gp>(prhs[1]), Nstar, mxGetDoubles(Xs), dbl(prhs[3]), dbl(prhs[4]), ss || S == 1, mxGetDoubles(plhs[0]), mxGetDoubles(plhs[1]),
                           mxGetDoubles(plhs[2]), mxGetDoubles(plhs[3])));
}

// -> C (n x m): the squared distances between the columns of a (D x n) and those of b (D x m; without b: of a itself)
static int cmd_sq_dist(int, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
  const mxArray* a = prhs[1];
  const mxArray* b = (nrhs > 2 && !mxIsEmpty(prhs[2])) ? prhs[2] : nullptr;
  const int D = (int)mxGetM(a), n = (int)mxGetN(a), m = b ? (int)mxGetN(b) : n;
  if (b && (int)mxGetM(b) != D) return raise("vbmc_hip:sq_dist", "Error: column lengths must agree.");
  plhs[0] = mxCreateDoubleMatrix(n, m, mxREAL);
  return done(vbmc_sq_dist(g_ctx, D, n, m, mxGetDoubles(a), b ? mxGetDoubles(b) : nullptr, mxGetDoubles(plhs[0])));
}

// ---- the command table: one row per command.  min_nrhs counts the command string itself: one more than the highest prhs index the
// handler reads unconditionally, which is one more than the names of the usage string in front of its first '['.  handles: how many
// leading arguments are uint64 device handles.  flags: NO_CTX where the command runs without a device context, else 0
enum { NO_CTX = 1 };
struct Command {
  const char* name;
  int min_nrhs, handles;
  const char* usage;
  int (*handler)(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]);
  int flags;
};
static const Command commands[] = {
    {"limits", 1, 0, "", cmd_limits, NO_CTX},
    {"stats", 1, 0, "", cmd_stats, NO_CTX},
    {"open", 1, 0, "[device]", cmd_open, NO_CTX},
    {"comm_open", 1, 0, "[ndev]", cmd_comm_open, NO_CTX},
    {"comm_size", 1, 0, "", cmd_comm_size, 0},
    {"gp_upload", 2, 0, "gp", cmd_gp_upload, 0},
    {"gp_upload_all", 2, 0, "gp", cmd_gp_upload_all, 0},
    {"gp_free_all", 2, 1, "hs", cmd_gp_free_all, 0},
    {"gp_free", 2, 1, "h", cmd_gp_free, 0},
    {"elbo", 9, 1, "h, theta, vp, Ns, compute_grad, compute_var, separate_K, beta [, thetabnd, eps, seed, numel(gp.post), no_jacobian]", cmd_elbo, 0},
    {"elbo_batch", 8, 1, "h, Theta, vp, Ns, compute_grad, compute_var, beta [, thetabnd, seed, separate_K, numel(gp.post)]", cmd_elbo_batch, 0},
    {"elbo_batch_multi", 8, 1, "hs, Theta, vp, Ns, compute_grad, compute_var, beta [, thetabnd, seed, separate_K, numel(gp.post)]", cmd_elbo_batch_multi, 0},
    {"adam", 11, 1, "h, Theta0, vp, Ns, compute_var, beta, thetabnd, seed, TolFun, MaxIter [, steps]", cmd_adam, 0},
    {"gp_post", 7, 0, "hyp, X, y, s2, meanfun, noisefun", cmd_gp_post, 0},
    {"gp_rank1", 7, 1, "h, Xnew, ystar, mstar, vstar, sn2_eff", cmd_gp_rank1, 0},
    {"acq", 8, 1, "h, Xs, acq_id, vp, ymax, var_regularized, TolGPVar [, gplengthscale, X_rescaled, sn2new]", cmd_acq, 0},
    {"acq_delta", 9, 1, "h, Xs, acq_id, vp, ymax, var_regularized, TolGPVar, delta [, gplengthscale, X_rescaled, sn2new]", cmd_acq_delta, 0},
    {"acq_search", 12, 1, "h, acq_id, vp, ymax, var_regularized, TolGPVar, x0, insigma, LB, UB, opts [, gplengthscale, X_rescaled, sn2new]", cmd_acq_search, 0},
    {"acq_search_iqr", 15, 2, "h, his, acq_id, vp, var_regularized, TolGPVar, x0, insigma, LB, UB, opts, gplengthscale, X_rescaled, sn2new", cmd_acq_search_iqr, 0},
    {"gp_quad", 6, 1, "h, mu, sigma, ssflag, numel(gp.post)", cmd_gp_quad, 0},
    {"acq_is_sample", 7, 1, "h, x0, LB, UB, Nm, opts", cmd_acq_is_sample, 0},
    {"is_create", 3, 1, "h, Xa [, lnw, fs2a, Ctmp]", cmd_is_create, 0},
    {"is_free", 2, 1, "his", cmd_is_free, 0},
    {"is_setup", 7, 1, "h, vp, Nvp, Nbox, Nm, opts", cmd_is_setup, 0},
    {"vp_pdf", 7, 0, "vp, X, origflag, logflag, transflag, df", cmd_vp_pdf, 0},
    {"vp_rnd", 7, 0, "vp, N, origflag, balanceflag, df, seed", cmd_vp_rnd, 0},
    {"vp_moments", 4, 0, "vp, Ns, seed", cmd_vp_moments, 0},
    {"vp_kldiv", 5, 0, "vp1, vp2, Ns, seed", cmd_vp_kldiv, 0},
    {"vp_mtv", 5, 0, "vp1, vp2, Ns, seed", cmd_vp_mtv, 0},
    {"vp_diag", 4, 0, "Ns, seed, vp1 [, vp2, ...]", cmd_vp_diag, 0},
    {"vp_mode", 5, 0, "vp, nmax, origflag, tol_grad", cmd_vp_mode, 0},
    {"vp_corner", 10, 0, "vp, X, Ns, seed, balanceflag, bounds, res, nbins, p", cmd_vp_corner, 0},
    {"acq_iqr", 9, 2, "h, his, Xs, gplengthscale, X_rescaled, sn2new, var_regularized, TolGPVar", cmd_acq_iqr, 0},
    {"gp_surrogate_sample", 9, 1, "h, vp, Ns, origflag, LB, UB, noise, opts", cmd_gp_surrogate_sample, 0},
    {"gp_nlz", 7, 0, "Hyp, X, y, s2, meanfun, noisefun", cmd_gp_nlz, 0},
    {"slice_sample", 16, 0, "X, y, s2, meanfun, noisefun, prior, LB, UB, hyp_start, widths, basewidths, options, seed, perms, U", cmd_slice_sample, 0},
    {"gp_train_opt", 11, 0, "X, y, s2, meanfun, noisefun, prior, LB, UB, design, options", cmd_gp_train_opt, 0},
    {"gp_pred", 7, 1, "h, Xstar, ystar, s2star, ssflag, numel(gp.post)", cmd_gp_pred, 0},
    {"sq_dist", 2, 0, "a [, b]", cmd_sq_dist, 0},
};

static const Command* find_command(const char* name) {
  for (const Command& c : commands)
    if (!strcmp(name, c.name)) return &c;
  return nullptr;
}

static const Command* g_cmd = nullptr;   // the row of the running command
static int usage_error() { return raise("vbmc_hip:usage", "%s: %s", g_cmd->name, g_cmd->usage); }

// Looks the command up, refuses a call that is too short or has no handle where one belongs -- before anything touches a device --,
// makes sure of the context and calls the handler.  Returns 0 on success, nonzero with g_err_id / g_err_msg set.  All C++ objects of
// a call live in the handler it reaches.
static int dispatch(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
  if (nrhs < 1 || !mxIsChar(prhs[0])) return raise("vbmc_hip:usage", "first argument must be a command string");
  char cmd[32];
  mxGetString(prhs[0], cmd, sizeof cmd);
  const Command* c = g_cmd = find_command(cmd);
  if (!c) return raise("vbmc_hip:usage", "unknown command");
  if (nrhs < c->min_nrhs) return usage_error();
  for (int i = 1; i <= c->handles; ++i)
    if (!is_handle(prhs[i])) return raise("vbmc_hip:usage", "this command takes a uint64 device handle as its first argument");
  if (!(c->flags & NO_CTX) && ensure_ctx(0)) return 1;
  return c->handler(nlhs, plhs, nrhs, prhs);
}

void mexFunction(int nlhs, mxArray* plhs[], int nrhs, const mxArray* prhs[]) {
  g_err_id[0] = 0;
  if (dispatch(nlhs, plhs, nrhs, prhs)) mexErrMsgIdAndTxt(g_err_id, "%s", g_err_msg);   // no C++ object alive here
}

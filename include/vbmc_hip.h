/*
 * vbmc_hip.h -- C ABI of libvbmc_hip.so: the MI355X (gfx950) implementation of the VBMC
 * ELBO inner loop.  This is the drop-in boundary: the reference (acerbilab/vbmc v1.0.12)
 * is pure MATLAB with no FFI seam, so these entry points are what a MEX
 * gateway (matlab/vbmc_hip_mex.cpp) or a ctypes binding (vbmc_amd/_lib.py) binds, one per
 * reference function on the path.  Each declaration cites the reference interface it
 * replaces (paths relative to the reference checkout).
 *
 * Conventions
 *   - all arrays are column-major IEEE fp64 exactly as MATLAB stores them, caller-owned,
 *     non-aliasing; the library never keeps a host pointer after the call returns;
 *   - every function returns a vbmc_status (0 = OK) and never throws across the ABI;
 *     vbmc_last_error(ctx) gives the message of the last failure on that context;
 *   - a context owns one HIP stream and all device scratch; calls on one context are
 *     serialised by the caller (the MATLAB interpreter thread / one Python process per GPU);
 *   - the library FAILS (VBMC_ERR_NO_DEVICE) when no gfx950 device is present: there is no
 *     CPU fallback anywhere behind this ABI.
 */
#ifndef VBMC_HIP_H
#define VBMC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VBMC_ABI_VERSION 8

typedef int vbmc_status;
enum {
  VBMC_OK = 0,
  VBMC_ERR_INVALID = 1,      /* bad argument (message says which)                         */
  VBMC_ERR_NO_DEVICE = 2,    /* no HIP device / not gfx950                                */
  VBMC_ERR_HIP = 3,          /* a HIP runtime call failed                                 */
  VBMC_ERR_UNSUPPORTED = 4,  /* option outside the accelerated path: caller must fall     */
                             /* through to the reference .m (e.g. meanfun not in {0,1,4}) */
  VBMC_ERR_NOT_POSDEF = 5    /* Cholesky failed after the reference's 10 jitter retries   */
};

typedef struct vbmc_ctx vbmc_ctx; /* device context: stream + scratch                      */
typedef struct vbmc_gp vbmc_gp;   /* device-resident gp.post(1..S) (gplite_post.m:94-157)  */

/* ---- library / context ------------------------------------------------------------- */
int vbmc_abi_version(void);
/* The shapes the library accepts -- the numbers its own validation enforces (anything beyond is VBMC_ERR_UNSUPPORTED and falls
 * through to the reference), so that a binding asks instead of restating them: matlab/vbmc_hip_supported.m reads them through
 * vbmc_hip_mex('limits').  A pure host function: no device, no context.  Replaces nothing in the reference (it has no limits);
 * the fall-through edges are listed in INTEGRATION.md section 4. */
typedef struct vbmc_limits {
  uint32_t struct_size;      /* sizeof(vbmc_limits) of the caller */
  int32_t max_D;             /* dimensions (every entry point) */
  int32_t max_K;             /* mixture components (misc/negelcbo_vbmc.m, ent/entmc_vbmc.m) */
  int32_t max_N;             /* training points of the surrogate on the factor paths: gplite_post / _pred / _nlZ, the variance of the
                                expected log joint, the acquisition sweep (the plain expected log joint has no limit) */
  int32_t max_Na;            /* importance points of acqviqr / acqimiqr */
  int32_t max_T_vargrad;     /* variational parameters with the gradient of the variance (compute_var = 2) */
  int32_t delta_ok;          /* 1: vp.delta ~= 0 is accelerated */
  int32_t meanfun_mask;      /* bit i set: gplite mean function id i is accelerated (0, 1, 4) */
} vbmc_limits;
vbmc_status vbmc_get_limits(vbmc_limits* out);
/* stream: a hipStream_t to launch on (e.g. torch's current stream) or NULL for a private one.  Side effect of the FIRST call in a process (std::call_once;
 * later contexts do not touch the environment): setenv("GPU_MAX_HW_QUEUES", "8", no overwrite) -- the pipelined forms keep five
 * streams busy and the runtime's default of four hardware queues serialises two of them (VBMC_HW_QUEUES=0: leave it alone,
 * VBMC_HW_QUEUES=n: that many).  It takes effect only if no other HIP user (torch, say) initialised the runtime earlier; a host with
 * threads that read the environment concurrently should set the variable itself and pass VBMC_HW_QUEUES=0. */
vbmc_status vbmc_ctx_create(int device, void* stream, vbmc_ctx** out);
void vbmc_ctx_destroy(vbmc_ctx* ctx);
const char* vbmc_last_error(const vbmc_ctx* ctx);
vbmc_status vbmc_ctx_synchronize(vbmc_ctx* ctx);
/* When enabled, HIP events bracket the dominant kernel (entropy MC) of every elbo call on the
 * context's stream; vbmc_ctx_last_kernel_ms returns its duration (bench.py roofline leg).
 * enable = 1: the call as it normally runs (a blocking call forks the expected log joint onto
 * the context's second, low-priority stream, where it shares the chip with the dominant kernel
 * and stretches its duration); enable = 2: nothing is forked beside it -- the duration of the
 * kernel alone, the figure a roofline prices. */
vbmc_status vbmc_ctx_set_profiling(vbmc_ctx* ctx, int enable);
vbmc_status vbmc_ctx_last_kernel_ms(vbmc_ctx* ctx, double* ent_ms, double* logjoint_ms);

/* ---- GP surrogate state -------------------------------------------------------------- */
/*
 * Upload gp.X and gp.post(s).{hyp,alpha,L,sW,Lchol} once per vpoptimize_vbmc call
 * (misc/vpoptimize_vbmc.m:71 closes over a constant gp).  Replaces the reads at
 * misc/gplogjoint.m:97-160.
 *   X      N x D      training inputs
 *   hyp    Nhyp x S   [log ell(D); log sf; noise(Nnoise); mean(Nmean)]
 *   alpha  N x S
 *   L      N x N x S  upper Cholesky factor (Lchol=1) or -inv(K+sn2 I) (Lchol=0); may be NULL
 *                     when only value/gradient without variance will be requested
 *   sW1    S          gp.post(s).sW(1)   (sn2_eff = 1/sW1^2, gplogjoint.m:160)
 *   Lchol  S          uint8 flags
 *   meanfun           gplite mean-function id; only 0 (zero), 1 (const), 4 (negquad) are
 *                     accelerated -- others return VBMC_ERR_UNSUPPORTED
 */
vbmc_status vbmc_gp_upload(vbmc_ctx* ctx, int N, int D, int S, int Nhyp, int Ncov, int Nnoise,
                           int meanfun, const double* X, const double* hyp, const double* alpha,
                           const double* L, const double* sW1, const uint8_t* Lchol,
                           vbmc_gp** out);
/* Releases a surrogate.  Its device blocks belong to the creating context's pool: pass that context while it is alive
 * (after vbmc_ctx_destroy the blocks are already gone and ctx may be NULL). */
void vbmc_gp_free(vbmc_ctx* ctx, vbmc_gp* gp);
/* Noise model needed by vbmc_gp_pred: gp.noisefun (3 ids, gplite_noisefun.m:176-210) and
 * gp.post(s).sn2_mult (S). */
vbmc_status vbmc_gp_set_noise(vbmc_ctx* ctx, vbmc_gp* gp, const int32_t noisefun[3], const double* sn2_mult);

/*
 * gp = gplite_post(hyp, X, y, covfun=SE-ARD, meanfun, noisefun, s2)   (gplite/gplite_post.m:1,
 * gplite/private/gplite_core.m:1-102,278-291; full posterior, no rank-1): per hyper-sample the
 * ARD-SE kernel matrix via sq_dist, the jittered Cholesky with the reference's x10 noise
 * inflation retry (<= 10 tries), alpha, and L (upper factor, or -inv(K+sn2 I) when
 * min(sn2) < 1e-6).  Outputs (any may be NULL): alpha N x S, L N x N x S, sW N x S, sn2_mult S,
 * Lchol S; *gp_out (optional) receives the device-resident posterior for vbmc_elbo_batch /
 * vbmc_gp_pred without a second upload: it takes over the device blocks the factorisation worked in (no copy of the S
 * N x N factors) and is ready when the call returns -- one upload, one synchronisation per call.
 * This call and vbmc_gp_nlz end with a polling wait on the context's stream (at most 300 us of hipStreamQuery before the
 * blocking wait, none where the enqueued work is known to be large: their callers issue the next evaluation at once).
 */
vbmc_status vbmc_gp_post(vbmc_ctx* ctx, int N, int D, int S, int Nhyp, int meanfun, const int32_t noisefun[3],
                         const double* X, const double* y, const double* s2, const double* hyp,
                         double* alpha, double* L, double* sW, double* sn2_mult, uint8_t* Lchol,
                         vbmc_gp** gp_out);

/*
 * acq = acqwrapper_vbmc(Xs,vp,gp,optimState,0,acqFun,acqInfo)   (acq/acqwrapper_vbmc.m:11-46) for the
 * density-based acquisition functions, with vp.delta = 0 (vbmc_acq_eval_delta otherwise): gplite_pred for every hyper-sample (:17), fbar / vtot
 * (:21-29), p = max(vbmc_pdf(vp,Xs,0),realmin), then
 *   acq_id 0  acqf_vbmc     -vtot .* exp(fbar - ymax) .* p                       (acq/acqf_vbmc.m:9-10)
 *   acq_id 1  acqflog_vbmc  -(log(vtot) + fbar - ymax + log(p))                  (acq/acqflog_vbmc.m:17-18)
 *   acq_id 2  acqus_vbmc    -vtot .* p.^2                                        (acq/acqus_vbmc.m:9)
 *   acq_id 3  acqfsn2_vbmc  -vtot .* (1 - sn2./(vtot+sn2)) .* exp(fbar - ymax) .* p, sn2 = gp.sn2new at the nearest
 *             row of gp.X_rescaled to Xs ./ optimState.gplengthscale               (acq/acqfsn2_vbmc.m:9-17)
 * followed by the variance regularisation (:35-45, if var_regularized) and max(acq,-realmax) (:46).  NOT done
 * here: the integer mapping (:8) and the hard-bound test in the ORIGINAL parameter space (:49-51), which need the
 * caller's warpvars_vbmc; the caller sets acq(outside) = Inf.  Xs is Nstar x D column-major in transformed
 * coordinates; vp_mu D x K.  Optional outputs fbar, vtot (Nstar each, may be NULL).
 */
vbmc_status vbmc_acq_eval(vbmc_ctx* ctx, const vbmc_gp* gp, int Nstar, const double* Xs, int acq_id, int K,
                          const double* vp_mu, const double* vp_sigma, const double* vp_lambda, const double* vp_w,
                          double ymax, int var_regularized, double TolGPVar, const double* gplengthscale,
                          const double* X_rescaled, const double* sn2new, double* acq, double* fbar, double* vtot);
/*
 * The same sweep with vp.delta > 0 (acq/acqwrapper_vbmc.m:12-14): the mean and variance per hyper-sample come from
 * gplite_quad(gp,Xs,vp.delta',1) -- the quadrature pass of vbmc_gp_quad, left on the device -- instead of gplite_pred, and
 * everything from fbar / vtot on is unchanged.  delta: D values, non-negative.  acq_id 0-3; a delta that is all zero is
 * VBMC_ERR_INVALID (the reference takes the gplite_pred branch then: call vbmc_acq_eval).  The importance-sampled IQR
 * functions with delta > 0 are not accelerated.
 */
vbmc_status vbmc_acq_eval_delta(vbmc_ctx* ctx, const vbmc_gp* gp, int Nstar, const double* Xs, int acq_id, int K,
                                const double* vp_mu, const double* vp_sigma, const double* vp_lambda, const double* vp_w,
                                double ymax, int var_regularized, double TolGPVar, const double* gplengthscale,
                                const double* X_rescaled, const double* sn2new, double* acq, double* fbar, double* vtot,
                                const double* delta);

/*
 * Importance-sampled IQR acquisition functions: acqviqr_vbmc (acq/acqviqr_vbmc.m:36-109) and acqimiqr_vbmc
 * (acq/acqimiqr_vbmc.m:30-95) behind acqwrapper_vbmc (acq/acqwrapper_vbmc.m:11-46, log-valued).
 *
 * vbmc_acq_is_create uploads optimState.ActiveImportanceSampling for one gp: the Na importance points Xa
 * (Na x D, or Na x D x S if per_sample_inputs), lnw (S x Na; NULL = zeros, i.e. VIQR), fs2a (Na x S; NULL = computed
 * here with gplite_pred, shared inputs only) and Ctmp_mat (N x Na x S; NULL = computed here as in
 * private/activeimportancesampling_vbmc.m:248-276: (L\(L'\Kax'))/sn2_eff for Lchol samples, L*Kax' otherwise).
 * IMIQR's per-call solve (acqimiqr_vbmc.m:77-79) is the same matrix, so one state serves both functions.
 *
 * vbmc_acq_iqr_eval: per hyper-sample C = Ka -/+ Ks'*Ctmp (:84-90), tau2 = C.^2 ./ ys2 with ys2 = fs2 + sn2new at
 * the nearest row of X_rescaled (:42-45), s_pred = sqrt(max(fs2a' - tau2, 0)), log-sum-exp of
 * lnw + u*s_pred + log1p(-exp(-2*u*s_pred)) over the importance points (:97-102), log-mean-exp over hyper-samples
 * (:104-107), the wrapper's variance regulariser and clamp.  The integer mapping and hard-bound test stay with the
 * caller (see vbmc_acq_eval).  Xs: Nstar x D column-major, transformed coordinates.
 */
typedef struct vbmc_acq_is vbmc_acq_is;
vbmc_status vbmc_acq_is_create(vbmc_ctx* ctx, const vbmc_gp* gp, int Na, const double* Xa, int per_sample_inputs,
                               const double* lnw, const double* fs2a, const double* Ctmp, vbmc_acq_is** out);
void vbmc_acq_is_free(vbmc_ctx* ctx, vbmc_acq_is* is);
vbmc_status vbmc_acq_iqr_eval(vbmc_ctx* ctx, const vbmc_gp* gp, const vbmc_acq_is* is, int Nstar, const double* Xs,
                              const double* gplengthscale, const double* X_rescaled, const double* sn2new,
                              int var_regularized, double TolGPVar, double* acq, double* fbar, double* vtot);

/*
 * [nlZ,dnlZ] = gplite_nlZ(hyp,gp,[])   (gplite/gplite_nlZ.m:1-72 -> gplite/private/gplite_core.m:1-102,128-275)
 * for B hyper-parameter vectors at once (the walkers / restarts of gplite_train.m:181,251,292,330): negative
 * log marginal likelihood nlZ (B) and, if compute_grad, its gradient dnlZ (Nhyp x B, column-major).  SE-ARD
 * covariance, mean functions 0/1/4, noise models of gplite_noisefun.m:176-210, no integrated mean, no output
 * warping, no hyper-prior (gplite_hypprior is O(Nhyp) host work; see vbmc_amd/gplite.py).  A matrix that is
 * still not positive definite after the 10 noise-inflation retries yields NaN for that vector
 * (gplite_train.m:542-546), not an error.
 */
vbmc_status vbmc_gp_nlz(vbmc_ctx* ctx, int N, int D, int B, int Nhyp, int meanfun, const int32_t noisefun[3],
                        const double* X, const double* y, const double* s2, const double* hyp, int compute_grad,
                        double* nlZ, double* dnlZ);

/*
 * [samples,fvals,exitflag,output] = slicesamplebnd(@(hyp) gp_objfun(hyp(:),gp,hprior,0,1), hyp_start', Ns, widths, LB, UB, opts)
 * (ABI version 7; utils/slicesamplebnd.m:229-358 with StepOut = false, its default; call site gplite/gplite_train.m:318-330) with the
 * WHOLE chain on the device: the training set is uploaded once, candidates never leave the device, every evaluation of the target
 * -gplite_nlZ(hyp) + gplite_hypprior(hyp) runs on the batched kernels of vbmc_gp_nlz, and the host only polls a progress word.
 * Model: as vbmc_gp_nlz (SE-ARD, mean functions 0/1/4, the noise models of gplite_noisefun.m:176-210; anything else is
 * VBMC_ERR_UNSUPPORTED).  logpdfbound (:415-449): a proposal outside [LB, UB] is -Inf without an evaluation, a NaN target (a matrix
 * still not positive definite after the jitter retries, gplite_train.m:542-546) a rejected proposal that counts as an evaluation.
 *
 * SPECULATION.  Without step-out the k-th shrink proposal of a coordinate, GIVEN that proposals 1 .. k-1 were rejected, is a function
 * of the current point, the interval and the uniforms alone (:283-304), so W of them are evaluated in one batched pass and the first
 * accepted one is taken.  Candidates are consumed in order: samples, logp, widths and funccount are BIT-IDENTICAL for every W; only
 * `performed` changes.  W = 0 asks for the library's default, 1: the table of repeated runs that a wider default has to rest on has not
 * been measured yet (profiles/gp_slice_sample.md holds what has: one run per width); a caller who wants speculation passes W itself.
 *
 * `performed` counts every evaluation launched: the speculative ones, and -- once more -- the candidates of a round that had to be
 * repeated with the jitter retries because a consumed candidate's first factorisation failed.  At large N the library lowers W until
 * the W work matrices (W N^2 doubles) stay below 2 GiB; the results do not change, `performed` follows the W actually used.
 *
 * RANDOM NUMBERS, sweeps = Burnin + Ns + (Ns - 1) * (Thin - 1) (:205,229):
 *   perms     sweeps x Nhyp int32, row `sweep` = the 0-BASED permutation randperm(D) - 1 of that sweep (:239), stored sweep after sweep;
 *   uniforms  U[sweep][idd][slot], slot = 0 .. 1 + Kmax fastest, idd (the position in the sweep's permutation, fixed coordinates keep
 *             their unused rows) next: slot 0 is the slice level's rand (:245), slot 1 the interval placement's (:252), slot 2 + k the
 *             k-th shrink proposal's, k = 0, 1, ... (:286).  A coordinate that needs more than Kmax proposals ends the call with
 *             VBMC_ERR_INVALID ("uniform block exhausted").
 *   rng_mode 1 (parity): the caller supplies both.  rng_mode 0 (device): the library's counter-based generator (Philox4x32-10 keyed by
 *   seed, counter (sweep, idd, slot)), no limit on the shrink count; vbmc_slice_rng_dump writes exactly the perms and the uniform block
 *   (for a Kmax of the caller's choosing) that seed stands for -- a pure host function -- so that a replay in parity mode is bit-identical.
 *
 * widths: positive and finite (the caller resolves the reference's defaults, :173-174); basewidths: the user-supplied widths of :166
 * for the end-of-burn-in update (:350-356), NULL = none were supplied.  LB / UB may be infinite; LB == UB fixes a coordinate (:243).
 * prior_mu NULL: no hyper-prior; prior_df NULL: 7 for every coordinate (gplite_hypprior.m:26).
 * Outputs (any may be NULL): samples Ns x Nhyp (column-major), logp Ns (fvals), widths_out Nhyp (output.widths), funccount
 * (output.funccount: evaluations of the sequential algorithm), performed (evaluations launched), max_shrink (largest number of
 * proposals a coordinate took).  The reference's own failure -- the interval shrunk onto the current point with the proposal still
 * rejected (:298-301) -- returns VBMC_ERR_INVALID with the reference's message; the context stays usable after any error.
 */
typedef struct vbmc_slice_args {
  uint32_t struct_size;      /* = sizeof(vbmc_slice_args) */
  int32_t N, D, Nhyp, meanfun;
  int32_t noisefun[3];
  const double* X;           /* N x D */
  const double* y;           /* N */
  const double* s2;          /* N or NULL */
  const double* prior_mu;    /* Nhyp or NULL */
  const double* prior_sigma; /* Nhyp */
  const double* prior_df;    /* Nhyp or NULL */
  const double* LB;          /* Nhyp */
  const double* UB;          /* Nhyp */
  const double* hyp_start;   /* Nhyp, inside the bounds */
  const double* widths;      /* Nhyp */
  const double* basewidths;  /* Nhyp or NULL */
  int32_t Ns, Thin, Burnin, Adaptive;
  int32_t W;                 /* speculation width, 0 .. 16 (0: default) */
  int32_t rng_mode;          /* 0 device generator, 1 parity */
  uint64_t seed;             /* rng_mode 0 */
  int32_t Kmax;              /* rng_mode 1: shrink slots per coordinate in `uniforms` */
  const int32_t* perms;      /* rng_mode 1 */
  const double* uniforms;    /* rng_mode 1 */
  double* samples;
  double* logp;
  double* widths_out;
  int64_t* funccount;
  int64_t* performed;
  int32_t* max_shrink;
  int64_t* rounds;           /* 2 or NULL: rounds that did work, rounds enqueued (the difference ran behind the chain's end or a stall) */
} vbmc_slice_args;
vbmc_status vbmc_gp_slice_sample(vbmc_ctx* ctx, const vbmc_slice_args* args);
vbmc_status vbmc_slice_rng_dump(uint64_t seed, int sweeps, int Nhyp, int Kmax, int32_t* perms, double* uniforms);

/*
 * The optimisation half of gplite_train (ABI version 8; gplite/gplite_train.m:200-306, utils/fminfill.m:101-114) with the training
 * set uploaded once and only a progress word crossing the host link until the result:
 *   1. FILL (fminfill.m:101-114).  gp_objfun = gplite_nlZ - gplite_hypprior at the Ninit rows of `design` (Ninit x Nhyp, column-major;
 *      its first rows are the caller's hyp0, the rest the space-filling design of fminfill.m:42-101, which the caller builds), in
 *      chunks whose work matrices stay below 2 GiB.  A matrix that is still not positive definite after the ten noise-inflation
 *      retries gives NaN (gplite_train.m:542-546).  The values are sorted as MATLAB's sort does: ascending, stable, NaN last.
 *   2. STARTS.  The first Nopts sorted rows (:206); with a noise hyper-parameter, Nopts > 1 and Ninit > Nopts the second start is
 *      the best of the fifth of the remaining rows with the smallest first noise parameter (:210-221); all are moved into
 *      [LB + eps(LB), UB - eps(UB)] (:272, an infinite bound leaves the coordinate alone: MATLAB's min / max pass over the NaN of
 *      eps(Inf)) and a fixed coordinate (LB == UB) is put on its value.  widths_default = std(design) with the zero widths repaired
 *      (:207,258-267).  Ninit = 0 is the branch of :249-256: the N0 given columns are evaluated and sorted, they are the starts, and
 *      widths_default (PUB - PLB there) is left to the caller.
 *   3. OPTIMISER.  fmincon is toolbox code outside the reference tree, so its trajectory cannot be reproduced; this is the library's
 *      OWN bound-constrained quasi-Newton method, a projected BFGS with a dense inverse-Hessian approximation H per start:
 *        free set   F = { i : LB_i < UB_i and not (x_i <= LB_i, g_i > 0) and not (x_i >= UB_i, g_i < 0) }, recomputed every iteration;
 *        direction  d_F = -H_FF g_F, d = 0 elsewhere; if g'd is not negative H is reset to the identity (d_F = -g_F);
 *        line search  candidates clip(x + t0 2^-k d, LB, UB), k = 0, 1, ..., t0 = 1 (min(1, 1 / |g_F|_1) while H is the identity);
 *                   the first with a finite value and f_c <= f + 1e-4 g'(x_c - x) is taken, NaN is a rejection that counts as an
 *                   evaluation; a candidate equal to x ends the start with exit flag 3, thirty rejected candidates with -2;
 *        update     s = x_c - x, y = g_c - g (zero on fixed coordinates); skipped unless s'y > 1e-10 |s| |y|; the first update after a
 *                   reset starts from H = (s'y / y'y) I;  H <- H - rho (s (Hy)' + (Hy) s') + (rho^2 y'Hy + rho) s s', rho = 1 / s'y;
 *        stopping   |x - clip(x - g)|_inf <= TolFun (exit flag 1), |f - f_old| <= TolFun (1 + |f|) (2), MaxIter iterations or
 *                   MaxFunEvals evaluations (0); a start whose first value is not finite ends with -3.
 *      All Nopts starts advance in lock-step; one ROUND is one batched value + gradient pass over Nopts x W candidates, the W
 *      consecutive backtracking candidates of every start, consumed in order: hyp, nll, iterations, funccount and the history are
 *      BIT-IDENTICAL for every W, only `performed` changes.  W = 0 asks for the default, 1.  A consumed candidate whose first
 *      factorisation fails stalls the call until the host has repeated that round with the retries, as in vbmc_gp_slice_sample.
 *   4. CLOSING (:298-306).  best = argmin of nll ignoring NaN, hyp_start = that column inside the bounds, fixed coordinates at LB.
 * Model set and refusals as vbmc_gp_nlz; Nhyp <= 128, 1 <= Nopts <= 16, W <= 16, at most 16384 design rows, and Nopts N^2 doubles
 * below 2 GiB (the starts are not chunked; W is lowered until Nopts W N^2 doubles are), VBMC_ERR_UNSUPPORTED beyond.  TolFun: the caller passes TolOpt or TolOptMCMC
 * (:163-167).  MaxIter <= 0: 1000; MaxFunEvals <= 0: 3000.  prior_mu NULL: no hyper-prior; prior_df NULL: 7 (gplite_hypprior.m:26).
 * Outputs (any may be NULL): fill_fvals Ninit (sorted), fill_order Ninit (0-based rows of the design), widths_default Nhyp, hyp
 * Nhyp x Nopts (column-major), nll Nopts, best (0-based), hyp_start Nhyp, iterations / funccount / exitflag Nopts, performed
 * (evaluations launched by the optimiser, the speculative and the repeated ones included), and the history of the first hist_cap
 * iterations of every start: hist_x [start][iteration][Nhyp], hist_f and hist_k [start][iteration] (the accepted candidate's k).
 * The context stays usable after any error.
 */
typedef struct vbmc_gptrain_args {
  uint32_t struct_size;      /* = sizeof(vbmc_gptrain_args) */
  int32_t N, D, Nhyp, meanfun;
  int32_t noisefun[3];
  const double* X;           /* N x D */
  const double* y;           /* N */
  const double* s2;          /* N or NULL */
  const double* prior_mu;    /* Nhyp or NULL */
  const double* prior_sigma; /* Nhyp */
  const double* prior_df;    /* Nhyp or NULL */
  const double* LB;          /* Nhyp */
  const double* UB;          /* Nhyp */
  const double* design;      /* max(Ninit, N0) x Nhyp, column-major */
  int32_t Ninit;             /* rows of the design; 0: the N0 given rows only (:249-256) */
  int32_t N0;                /* rows of the design that are the caller's hyp0 (used when Ninit = 0) */
  int32_t Nopts;
  int32_t Ncov;              /* D + 1: the column of the first noise parameter (the low-noise pick) */
  double TolFun;
  int32_t MaxIter;
  int32_t MaxFunEvals;
  int32_t W;                 /* speculation width, 0 .. 16 (0: default) */
  int32_t hist_cap;          /* iterations per start the history blocks hold */
  double* fill_fvals;
  int32_t* fill_order;
  double* widths_default;
  double* hyp;
  double* nll;
  int32_t* best;
  double* hyp_start;
  int32_t* iterations;
  int64_t* funccount;
  int32_t* exitflag;
  int64_t* performed;
  double* hist_x;
  double* hist_f;
  int32_t* hist_k;
} vbmc_gptrain_args;
vbmc_status vbmc_gp_train_optimize(vbmc_ctx* ctx, const vbmc_gptrain_args* args);

/*
 * [ymu,ys2,fmu,fs2] = gplite_pred(gp, Xstar, ystar, s2star, ssflag)   (gplite/gplite_pred.m:1-165).
 * Xstar is Nstar x D.  ssflag = 0: outputs are Nstar vectors averaged over hyper-samples with
 * the between-sample variance added (:154-165); ssflag = 1: Nstar x S per-sample outputs.
 * ystar (Nstar, may be NULL = []) only enters the noise at the test points for output-dependent noise models
 * (gp.noisefun(3) = 1: sn2 += w^2 max(0, ythresh - ystar)^2, gplite_noisefun.m:198-207; skipped when ystar is empty, as in
 * the reference); fmu / fs2 never depend on it.
 */
vbmc_status vbmc_gp_pred(vbmc_ctx* ctx, const vbmc_gp* gp, int Nstar, const double* Xstar, const double* ystar,
                         const double* s2star, int ssflag, double* ymu, double* ys2, double* fmu, double* fs2);

/*
 * [F,varF] = gplite_quad(gp, mu, sigma, ssflag)   (gplite/gplite_quad.m:1-119): the Bayesian-quadrature integral of the GP
 * against N(mu_i, diag sigma^2) for every row mu_i of mu (Nstar x D, column-major), per hyper-sample
 *   z = exp(lnnf - 1/2 sum_d ((mu_id - X_nd) / tau_d)^2), tau = sqrt(sigma^2 + ell^2)      (:70-76)
 *   F = z alpha + m0 + nu                                                                    (:77-82)
 *   varF = max(eps, nf_kk - z inv(K) z')                                                     (:98-106)
 * with the same kernels, launch forms and limits as vbmc_gp_pred (needs L on the device and vbmc_gp_set_noise).
 * sigma is sigma_rows x D with sigma_rows = 1 (one row shared by all points: the only form a reference caller uses) or
 * sigma_rows = Nstar with all rows equal; distinct rows are VBMC_ERR_UNSUPPORTED (the distance is then no longer one scaled
 * product).  Mean functions 0, 1 and 4.  ssflag = 0: Nstar values averaged over the hyper-samples with the between-sample
 * variance added (:112-119); ssflag = 1: Nstar x S.  varF may be NULL.
 */
vbmc_status vbmc_gp_quad(vbmc_ctx* ctx, const vbmc_gp* gp, int Nstar, const double* mu, const double* sigma, int sigma_rows,
                         int ssflag, double* F, double* varF);

/*
 * The acquisition search of active sampling (private/activesample_vbmc.m:264-290 with SearchOptimizer = 'cmaes', VBMC's default) with
 * the WHOLE optimiser on the device: minimise acqwrapper_vbmc(x) -- exactly the function of vbmc_acq_eval, acq_id 0-3, vp.delta = 0 --
 * over the box [LB, UB] from x0.  The optimiser is the project's plain (mu/mu_w, lambda)-CMA-ES (vbmc_amd/optimize.py::cmaes_batched,
 * which stands in for the third-party cmaes_modded.m: same constants wts / mueff / cc / cs / c1 / cmu / damps / chiN, same hsig,
 * rank-one and rank-mu updates, step-size adaptation and the same four stopping rules over a history window of 10 + ceil(30 D / lambda)
 * values), in its CHOLESKY form (Krause, Arnold & Glasmachers 2016): Y = A Z with A the lower Cholesky factor of C, refreshed every
 * generation, and ps updated with A^-1 yw -- a factor that is unique, so that a trajectory is a function of Z and can be compared.
 * A C that has lost positive definiteness gets 1e-14 max diag added to its diagonal once; if it is still indefinite the search stops
 * with the stop code of MaxIter and the state so far.  Candidates are clamped into [LB, UB]; the clamped points are evaluated, ranked
 * (a value that is not finite ranks as +Inf, ties keep the index order) and fed to the update as y = (x_clamped - xmean) / sigma.
 * `evals` counts lambda per generation.  None of cmaes_modded's restarts, active-CMA or noise handling.
 *
 * One generation is one launch of the optimiser's kernel, the prediction of the lambda <= 16 points for every hyper-sample and the
 * acquisition kernel; generations are enqueued in chunks of `chunk` (0: the default, 16) with no host synchronisation inside a chunk,
 * and the host reads a progress word one chunk behind.  Results do not depend on `chunk`.
 *
 * popsize: lambda, 0 = 4 + floor(3 ln D), at most 16 (2 at the least).  MaxFunEvals <= 0: no limit.  MaxIter 0: 1e3 (D + 5)^2 / sqrt(lambda).
 * RANDOM NUMBERS.  rng_mode 0: Philox4x32-10 keyed by `seed`, counter (generation, point, d), through an inverse normal CDF made of
 * exactly rounded operations only; vbmc_acq_search_rng_dump -- a pure host function -- writes the D x lam x G block Z[d + D (j + lam g)]
 * that `seed` stands for.  rng_mode 1 (parity): the caller supplies that block for Gmax generations; a search that needs more ends with
 * VBMC_ERR_INVALID ("normal block exhausted").  A replay of a dump in parity mode is bit-identical.
 *
 * VBMC_ERR_UNSUPPORTED: the IQR acquisition functions (ids >= 10: vbmc_acq_search_iqr searches those) and any other id outside 0-3, vp_delta with a positive entry, and
 * whatever vbmc_acq_eval refuses.  VBMC_ERR_INVALID: LB / UB / x0 / insigma not finite, LB >= UB, x0 outside the box, insigma not
 * positive, popsize outside 2 .. 16 (0 aside).  The context stays usable after any error.
 * Outputs (any may be NULL): xmin / fmin the LAST generation's best point and value (what cmaes_modded returns first), xbest / fbest the
 * best ever seen (bestever; x0 and +Inf if no value was ever finite), the final xmean (D), sigma, C (D x D), evals, generations, stop
 * (VBMC_SEARCH_STOP_*), rounds[2] = {generations, launches of the optimiser's kernel that found the search finished}.  Trace (tests):
 * for the first trace_cap generations the rank order (lam int32 each, 0-based), the sorted values (lam), xmean (D) and sigma after the
 * update; all four pointers or none.
 */
#define VBMC_SEARCH_STOP_TOLX 1
#define VBMC_SEARCH_STOP_TOLFUN 2
#define VBMC_SEARCH_STOP_TOLHISTFUN 3
#define VBMC_SEARCH_STOP_MAXFUNEVALS 4
#define VBMC_SEARCH_STOP_MAXITER 5
typedef struct vbmc_acqsearch_args {
  uint32_t struct_size;      /* = sizeof(vbmc_acqsearch_args) */
  int32_t acq_id, K;
  const double* vp_mu;       /* D x K */
  const double* vp_sigma;    /* K */
  const double* vp_lambda;   /* D */
  const double* vp_w;        /* K */
  const double* vp_delta;    /* D or NULL; must be all zero */
  double ymax;
  int32_t var_regularized;
  double TolGPVar;
  const double* gplengthscale; /* acq_id 3, 10, 11 */
  const double* X_rescaled;    /* acq_id 3, 10, 11 */
  const double* sn2new;        /* acq_id 3, 10, 11 */
  const double* x0;          /* D, inside the box */
  const double* insigma;     /* D, positive */
  const double* LB;          /* D */
  const double* UB;          /* D */
  double TolX, TolFun, TolHistFun;
  int64_t MaxFunEvals;
  int32_t MaxIter, popsize;
  int32_t rng_mode;          /* 0 device generator, 1 parity */
  int32_t Gmax;              /* rng_mode 1: generations in Z */
  uint64_t seed;             /* rng_mode 0 */
  const double* Z;           /* rng_mode 1: D x lam x Gmax */
  int32_t chunk;             /* generations enqueued between two looks at the progress word (0: default) */
  int32_t trace_cap;
  double* xmin;
  double* fmin;
  double* xbest;
  double* fbest;
  double* xmean;
  double* sigma;
  double* C;
  int64_t* evals;
  int32_t* generations;
  int32_t* stop;
  int64_t* rounds;
  int32_t* tr_order;
  double* tr_F;
  double* tr_xmean;
  double* tr_sigma;
} vbmc_acqsearch_args;
vbmc_status vbmc_acq_search(vbmc_ctx* ctx, const vbmc_gp* gp, const vbmc_acqsearch_args* args);
vbmc_status vbmc_acq_search_rng_dump(uint64_t seed, int D, int lam, int G, double* Z);

/*
 * The same search on the importance-sampled IQR acquisition functions of noisy targets (misc/setupoptions_vbmc.m:144-159): the objective
 * is exactly the function of vbmc_acq_iqr_eval -- acqwrapper_vbmc with acqviqr_vbmc / acqimiqr_vbmc on the state `is`
 * (vbmc_acq_is_create), log-valued, with the wrapper's variance regulariser and clamp.  Same argument struct, optimiser, random-number
 * contract (vbmc_acq_search_rng_dump, parity replay), outputs, trace, stop codes, chunked driving and box / start / popsize validation as
 * vbmc_acq_search.  acq_id must be 10 or 11 (both mean the same computation; the state decides: no lnw is VIQR, lnw and / or
 * per-hyper-sample Xa is IMIQR), anything else is VBMC_ERR_UNSUPPORTED, as is vp_delta with a non-zero entry.  gplengthscale, X_rescaled
 * and sn2new are required (VBMC_ERR_INVALID without them); K, vp_mu, vp_sigma, vp_lambda, vp_w and ymax are not read.  A state created
 * for another GP is VBMC_ERR_INVALID.  One generation is the optimiser's kernel, the prediction of the one point tile (which leaves its
 * sW-scaled cross-kernel tile), the nearest-neighbour noise, the tile kernel -- one workgroup per 16 importance points and hyper-sample,
 * its waves splitting the sum over the training points -- and a closing kernel.  The prediction's sq_dist centring constant is the
 * training inputs' mean alone here, so that a point's value depends neither on its slot among the lambda points nor on the other points.
 */
vbmc_status vbmc_acq_search_iqr(vbmc_ctx* ctx, const vbmc_gp* gp, const vbmc_acq_is* is, const vbmc_acqsearch_args* args);

/*
 * The MCMC of the IMIQR importance sampler (private/activeimportancesampling_vbmc.m:153-235, Step 2) with the WHOLE sampler on the
 * device: for each of the S GP hyper-samples an ensemble of W walkers samples the log base density of acqimiqr_vbmc
 * (acq/acqimiqr_vbmc.m:22-25 with importance_sampling_vp = false; importance_sampling_vp = true is not offered),
 *     logp(x) = ymu + u ys + log1p(-exp(-2 u ys)),   ys = sqrt(max(ys2, realmin)),   u = 0.6745,
 * where [ymu, ys2] are the first two outputs of gplite_pred for hyper-sample s ALONE (:346 reads the noisy pair, not fmu / fs2) -- what
 * vbmc_gp_pred(..., ystar = NULL, s2star = NULL, ssflag = 1) returns in column s.  A value that is not finite is -Inf.  A point outside
 * [LB, UB] has density -Inf, costs no evaluation and is not counted.  A starting walker with -Inf density is VBMC_ERR_INVALID ("a
 * starting point has zero density"): the caller replaces such walkers before the call.
 *
 * THE ALGORITHM is the library's ensemble slice sampler (vbmc_amd/acq.py::ensemble_slice_sample, which stands in for the third-party
 * eissample_lite.m): the two halves of an ensemble move in turn; a walker of the moving half takes its direction x_other[b] - x_other[a]
 * from two distinct walkers of the complementary half as it stands when the half-move begins (sigma_factor = 1), places a unit interval
 * around itself, steps both ends out (at most max_steps unit steps each; an end stops at the first step below the slice level) and
 * shrinks (at most max_shrink proposals; the first one above the level is accepted).  A walker whose slice collapsed stays where it is.
 * After a half-move each of its H = W / 2 walkers counts as one move; after `burnin` moves every thin-th moved walker is recorded, until
 * Nm are.  All randomness comes from an INDEXED UNIFORM BLOCK  U[slot + 64 (j + H (e + S m))]  with m the half-move counted from 0 (half
 * m mod 2 moves), e the ensemble and j the walker's position inside the moving half:
 *     slot 0      a = floor(u H)
 *     slot 1      b = (a + 1 + floor(u (H - 1))) mod H        (H = 2: b = 1 - a; the slot is still reserved)
 *     slot 2      slice level y = logp(x) + log(u)
 *     slot 3      interval placement L = -u, R = L + 1
 *     slot 4 + q  the q-th shrink proposal t = L + u (R - L); a rejected t < 0 becomes L, otherwise R
 * The left end after k steps is L - k, the right end R + k, a candidate is x + t (x_other[b] - x_other[a]), every operation rounded on
 * its own.  rng_mode 0: slot (m, e H + j, slot) is generated with Philox4x32-10 keyed by `seed`, through the 52-bit uniform of
 * vbmc_gp_slice_sample, strictly inside (0, 1); vbmc_acq_is_sample_rng_dump -- a pure host function -- writes the 64 x H x S x M block
 * a seed stands for.  rng_mode 1 (parity): the caller supplies the block for Mmax half-moves; a chain that needs more ends with
 * VBMC_ERR_INVALID ("uniform block exhausted"), as does a block with a value outside the open interval (0, 1).  A replay of a dump in
 * parity mode is bit-identical.  The target's exponentials and logarithms are the library's own (the table exponential, the
 * logarithm of the search's generator, ln(1 - e) from it by exactly rounded operations), none the device library's.
 *
 * One ROUND is one launch each of the sampler's kernel (one workgroup per ensemble: it consumes the previous round's values in candidate
 * order, commits and records, and writes up to 2 spec candidates per walker while stepping out and spec while shrinking, with an in-bounds
 * mask, straight into the prediction's point buffer) and of the prediction, which evaluates every candidate under its own hyper-sample
 * only and closes with the target.  spec (1..4, 0: 3) changes the number of rounds, never a bit of the results.  Rounds are enqueued in
 * chunks of `chunk` (0: 16) and the progress words are read one chunk behind; results do not depend on `chunk`.  funccount counts the
 * in-bounds evaluations the one-at-a-time procedure (spec = 1) consumes, the W S starting walkers included; performed all in-bounds
 * evaluations launched.
 *
 * Inputs: x0 (W x D x S, column-major: the W starting walkers of each ensemble, inside the box), LB / UB (D, finite, LB < UB), W even
 * with 4 <= W <= 2 (D + 1), Nm (1 .. 256 recorded samples per ensemble), thin >= 1, burnin (-1: ceil(thin Nm / 2)), max_steps /
 * max_shrink (0: 20 and 60, which are also the caps).  Outputs (any may be NULL): Xa (Nm x D x S) the recorded walkers, logp (S x Nm) the
 * chain's own value at each, fs2a (Nm x S) the latent fs2 at the recorded points under their own hyper-sample from one closing
 * prediction, lnw (S x Nm) = fmu - logp (:218-230: islogf1 of IMIQR is fmu), funccount, performed, rounds[2] = {rounds that did work (the
 * slowest ensemble's), launches that found every chain finished}, and `state`: the importance-sampling state of those device buffers
 * with per_sample_inputs = 1, built without a host round trip (free it with vbmc_acq_is_free); it is what vbmc_acq_is_create makes of
 * the downloaded arrays.
 *
 * VBMC_ERR_UNSUPPORTED: whatever vbmc_gp_pred refuses, and a GP beyond the range in which the prediction keeps inv(L') resident (the
 * slab form of large N).  VBMC_ERR_INVALID: W odd or outside 4 .. 2 (D + 1), LB >= UB or not finite, a start outside the box or with zero
 * density, D / S that are not the GP's, Nm outside 1 .. 256, thin < 1, spec outside 0 .. 4, max_steps / max_shrink beyond their caps, an exhausted uniform block, a GP
 * without vbmc_gp_set_noise.  The context stays usable after any error.
 */
typedef struct vbmc_is_sample_args {
  uint32_t struct_size;      /* = sizeof(vbmc_is_sample_args) */
  int32_t W, Nm, thin, burnin, spec, max_steps, max_shrink;
  const double* x0;          /* W x D x S */
  const double* LB;          /* D */
  const double* UB;          /* D */
  int32_t rng_mode;          /* 0 device generator, 1 parity */
  int32_t Mmax;              /* rng_mode 1: half-moves in U */
  uint64_t seed;             /* rng_mode 0 */
  const double* U;           /* rng_mode 1: 64 x H x S x Mmax */
  int32_t chunk;             /* rounds enqueued between two looks at the progress words (0: default) */
  int32_t D, S;              /* the dimensions x0 and U are laid out for: they must be the GP's (VBMC_ERR_INVALID otherwise) */
  int32_t reserved_;
  double* Xa;                /* Nm x D x S */
  double* lnw;               /* S x Nm */
  double* fs2a;              /* Nm x S */
  double* logp;              /* S x Nm */
  int64_t* funccount;
  int64_t* performed;
  int64_t* rounds;           /* 2 */
  vbmc_acq_is** state;
} vbmc_is_sample_args;
vbmc_status vbmc_acq_is_sample(vbmc_ctx* ctx, const vbmc_gp* gp, const vbmc_is_sample_args* args);
vbmc_status vbmc_acq_is_sample_rng_dump(uint64_t seed, int S, int H, int M, double* U);

/*
 * vbmc_acq_is_setup: the whole set-up of the IMIQR importance sampler in one call, from (vp, gp) to the device-resident
 * importance-sampling state -- Step 1 (private/activeimportancesampling_vbmc.m:106-151), the resampling of the starting walkers
 * (:205-215), Step 2 as vbmc_acq_is_sample runs it, the closing prediction and Ctmp.  It serves acqimiqr_vbmc with
 * importance_sampling_vp = false and vp.delta = 0, the case vbmc_acq_is_sample serves.
 *
 * On the device: rect_delta = 2 std(X) and the box LB / UB = data range -/+ half the diameter (:27-31, :112); Nvp points of the
 * 4K-component smoothed mixture (:116-129, scales 0.05 / 0.2 / 1, weights renormalised) and Nbox points in boxes around training inputs
 * (:140-141); ONE prediction of the Na1 = Nvp + Nbox points under every hyper-sample; the proposal's log density -- a log-sum-exp over
 * the 4K components, the number of training inputs whose box holds the point, the two-term log-sum-exp of :335-337 --, lnw = fmu - lpdf
 * with non-finite values -Inf (:148; a point outside every box and beyond the mixture's range has lpdf = -Inf and weight zero) and the
 * resampling log weight lnw + u fs + log1p(-exp(-2 u fs)); per hyper-sample W draws without replacement by catrnd's rule
 * idx = #(cdf < u cdf(end)) + 1 (:208-214, :403-408; weights that ran out are reset to ones), each chosen point clipped into
 * [LB, UB].  The starting walkers' density comes from the sampler's own first prediction: if any is -Inf the call returns VBMC_OK with
 * n_bad > 0, the mask `bad` (W x S) and x0, the sampler's outputs untouched and no state -- the caller replaces those walkers and calls
 * vbmc_acq_is_sample.  Nm = 0 is Step 1 alone (the reference's Nmcmc_samples = 0 branch): no resampling, and `state` is the state of
 * the Na1 shared points with lnw1.
 *
 * All randomness of Step 1 and of the resampling is an INDEXED BLOCK  B  of (D + 1) Na1 + W S doubles:
 *     point i < Nvp          B[(D + 1) i] a uniform: the mixture component by catrnd;  B[1 + d + (D + 1) i] a standard normal z_d:
 *                            x_d = mu(d, c mod K) + (lambda_d sigma4_c) z_d
 *     point Nvp <= i < Na1   B[(D + 1) i] a uniform: the training input j = floor(u N);  B[1 + d + (D + 1) i] a uniform u_d:
 *                            x_d = X(j, d) + (2 u_d - 1) rect_delta_d
 *     draw i of ensemble s   B[(D + 1) Na1 + i + W s] a uniform
 * every operation rounded on its own.  rng_mode 0: the block is generated from `seed` with the Philox uniforms of vbmc_gp_slice_sample
 * and the normals of vbmc_acq_search, at counters Step 2 never reaches (Step 2 draws from the same seed exactly as vbmc_acq_is_sample
 * does); vbmc_acq_is_setup_rng_dump -- a pure host function -- writes the block a seed stands for.  rng_mode 1: the caller supplies B
 * (uniforms strictly inside (0, 1), normals finite; VBMC_ERR_INVALID otherwise) and, optionally, Step 2's block U with Mmax (without
 * it Step 2 uses `seed`).  A replay of the two dumps is bit-identical in every output.
 *
 * Inputs: the variational posterior (K, mu D x K, sigma K, lambda D, w K), Nvp, Nbox >= 0 with 1 <= Nvp + Nbox <= 256, and W, Nm, thin,
 * burnin, spec, chunk, max_steps, max_shrink as in vbmc_is_sample_args.  Outputs (any may be NULL): Xa1 (Na1 x D), lnw1 (S x Na1),
 * fs2a1 (Na1 x S), lpdf1 (Na1: the proposal's log density), rect_delta / LB / UB (D each), x0 (W x D x S), idx0 (W x S, 0-based indices
 * into Xa1), n_bad, bad (W x S), and everything vbmc_is_sample_args returns.  After a bad start funccount and performed count the W S
 * starting evaluations.
 *
 * Errors: those of vbmc_acq_is_sample, and VBMC_ERR_INVALID for Nvp + Nbox outside 1 .. 256, a negative count, a vp that is not finite
 * (sigma, lambda > 0, w >= 0 with a positive sum), a block value outside its range, fewer than two training inputs; VBMC_ERR_UNSUPPORTED
 * for K or D beyond the library's limits.  The context stays usable after any error.
 */
typedef struct vbmc_is_setup_args {
  uint32_t struct_size;      /* = sizeof(vbmc_is_setup_args) */
  int32_t D, S;              /* the dimensions the arrays are laid out for: they must be the GP's */
  int32_t K;
  const double* vp_mu;       /* D x K */
  const double* vp_sigma;    /* K */
  const double* vp_lambda;   /* D */
  const double* vp_w;        /* K */
  int32_t Nvp, Nbox;
  int32_t W, Nm, thin, burnin, spec, max_steps, max_shrink, chunk;
  int32_t rng_mode;          /* 0 device generator, 1 parity */
  int32_t Mmax;              /* rng_mode 1 with U: half-moves in U */
  uint64_t seed;
  const double* B;           /* rng_mode 1: (D + 1) Na1 + W S */
  const double* U;           /* rng_mode 1, optional: 64 x H x S x Mmax */
  double* Xa1;               /* Na1 x D */
  double* lnw1;              /* S x Na1 */
  double* fs2a1;             /* Na1 x S */
  double* lpdf1;             /* Na1 */
  double* rect_delta;        /* D */
  double* LB;                /* D */
  double* UB;                /* D */
  double* x0;                /* W x D x S */
  int32_t* idx0;             /* W x S */
  int32_t* n_bad;
  uint8_t* bad;              /* W x S */
  double* Xa;                /* Nm x D x S */
  double* lnw;               /* S x Nm */
  double* fs2a;              /* Nm x S */
  double* logp;              /* S x Nm */
  int64_t* funccount;
  int64_t* performed;
  int64_t* rounds;           /* 2 */
  vbmc_acq_is** state;
} vbmc_is_setup_args;
vbmc_status vbmc_acq_is_setup(vbmc_ctx* ctx, const vbmc_gp* gp, const vbmc_is_setup_args* args);
vbmc_status vbmc_acq_is_setup_rng_dump(uint64_t seed, int D, int S, int W, int Nvp, int Nbox, double* B);

/*
 * The O(N^2) pieces of gplite_post's rank-1 append of one training point x* (gplite/gplite_post.m:173-251),
 * for every hyper-sample: Ks = k(X, x*) (N x S); for Lchol samples v = L' \ Ks and x = L \ v, so that
 * alpha_update = x / sn2_eff (:227) and the new column of L is v / sn2_eff (:228); for low-noise samples
 * x = L * Ks (alpha_update = -x, :234).  The O(N) assembly of the enlarged posterior is the caller's.
 */
vbmc_status vbmc_gp_rank1_solves(vbmc_ctx* ctx, const vbmc_gp* gp, const double* xstar, double* Ks, double* v,
                                 double* x);

/* C = sq_dist(a, b)   (utils/sq_dist.m:14-50): a is D x n, b is D x m (NULL -> b = a), C is n x m.
 * The a'b contraction runs on v_mfma_f64_16x16x4_f64. */
/* gp = gplite_post(gp, xstar, ystar, [], [], [], [], 1): rank-one append of one observation, entirely on the device
 * (gplite/gplite_post.m:173-251).  X_new is the (N+1) x D training matrix with xstar as its last row; mstar, vstar (S each)
 * are [mstar, vstar] = gplite_pred(gp, xstar, ystar, [], 1) (:189) -- or both NULL, in which case they are computed here from
 * the solves of the append itself -- and sn2_eff (S) the noise at the new point times sn2_mult (:196-207), which the caller has.  *out is a NEW surrogate handle with N+1 points (the old one stays valid);
 * alpha_new ((N+1) x S) and L_new ((N+1) x (N+1) x S) are optional host copies of the new gp.post(s).alpha / .L. */
vbmc_status vbmc_gp_rank1_update(vbmc_ctx* ctx, const vbmc_gp* gp, const double* X_new, double ystar, const double* mstar,
                                 const double* vstar, const double* sn2_eff, double* alpha_new, double* L_new, vbmc_gp** out);
vbmc_status vbmc_sq_dist(vbmc_ctx* ctx, int D, int n, int m, const double* a, const double* b, double* C);

/* ---- the ELBO objective ---------------------------------------------------------------
 * One call evaluates R independent negelcbo_vbmc(theta_r, beta, vp, gp, Ns, compute_grad,
 * compute_var, ~, thetabnd) (misc/negelcbo_vbmc.m:1) -- R = 1 is the Adam-loop call
 * (misc/vpoptimize_vbmc.m:71, utils/fminadam.m:48), R > 1 is the sieve batch
 * (misc/vpsieve_vbmc.m:74-78).
 * gp == NULL evaluates the entropy term alone: H, dH (and F = -H + penalties) are then
 * [H,dH] = entmc_vbmc(vp,Ns,grad_flags,1) (ent/entmc_vbmc.m:1) for Ns > 0 and entlb_vbmc(vp,grad_flags,1)
 * (ent/entlb_vbmc.m:1) for Ns = 0, with grad_flags = optimize[]; G = 0, dG = 0; compute_var and
 * separate_K must be 0.  With Ns = 0 and a surrogate, G, dG, varG, varGss, I_sk, J_sjk are the outputs of
 * gplogjoint(vp,gp,grad_flags,1,1,compute_var,separate_K) (misc/gplogjoint.m:1) on its own; G_s / varG_s are its
 * avg_flag = 0 outputs.
 */
typedef struct vbmc_elbo_args {
  uint32_t struct_size;      /* = sizeof(vbmc_elbo_args), for ABI versioning                */
  int32_t D, K, R;
  int32_t optimize[4];       /* vp.optimize_{mu,sigma,lambda,weights}                       */
  const double* theta;       /* T x R, T = sum of optimised groups, negelcbo_vbmc.m:33-48   */
  /* current vp fields; used for every group that is NOT optimised (may be NULL otherwise)  */
  const double* vp_mu;       /* D x K */
  const double* vp_sigma;    /* K     */
  const double* vp_lambda;   /* D     */
  const double* vp_w;        /* K     */
  const double* vp_delta;    /* D or NULL (= 0), gplogjoint.m:85-89                         */
  int32_t Ns;                /* MC samples per component; forced even (entmc_vbmc.m:45);    */
                             /* 0 -> deterministic bound entlb_vbmc (negelcbo_vbmc.m:104-110) */
  int32_t eps_mode;          /* 0 device Philox RNG; 1 eps on host; 2 eps already on device */
  const double* eps;         /* D x Ns/2 x K (x R unless eps_shared): the K consecutive     */
                             /* randn(D,1,Ns/2) blocks of entmc_vbmc.m:53                   */
  int32_t eps_shared;        /* 1: one eps block reused for all R restarts                  */
  uint64_t seed;             /* eps_mode 0: Philox key; stream position = (r, j, sample)    */
  int32_t compute_grad;      /* negelcbo arg 6                                              */
  int32_t compute_var;       /* 0 none, 1 full K x K, 2 diagonal (gplogjoint.m:273-337)     */
  int32_t separate_K;        /* also return I_sk (and J_sjk when compute_var)               */
  double beta;               /* ELCBO weight (negelcbo arg 2)                               */
  /* soft bounds (misc/vpbounds.m, misc/vpbndloss.m); lb == NULL -> thetabnd = []           */
  const double* bnd_lb;      /* length of theta_ext: [mu(:); lnscale(:) (D x K); eta]       */
  const double* bnd_ub;
  double TolCon, WeightThreshold, WeightPenalty;
  double sparse_cutoff;      /* 0: dense (every sample x component term, as the reference).  c > 0: block-sparse -- a
                              * 16-component tile is skipped for a 16-sample tile when every one of its terms is
                              * provably < exp(-c) relative to q(x) (c = 100 changes results by < 1e-40 relative)   */
  /* outputs (any may be NULL) */
  double* F;                 /* R      negative EL(C)BO incl. penalties                     */
  double* dF;                /* T x R                                                       */
  double* G;                 /* R      expected log joint                                   */
  double* H;                 /* R      entropy                                              */
  double* dG;                /* T x R                                                       */
  double* dH;                /* T x R                                                       */
  double* varG;              /* R                                                           */
  double* varGss;            /* R                                                           */
  double* I_sk;              /* S x K x R                                                   */
  double* J_sjk;             /* S x K x K x R                                               */
  /* per-hyper-sample outputs of gplogjoint(vp,gp,0,0,...) (avg_flag = 0, misc/gplogjoint.m:399: no averaging) -- what
   * private/activesample_vbmc.m:155 ([~,~,varF] = gplogjoint(vp,gp,0,0,0,1)) and misc/vpoptimizeweights_vbmc.m:42 read */
  double* G_s;               /* S x R  F(s) = sum_k w_k I_sk  (:203)                        */
  double* varG_s;            /* S x R  varF(s), each max(.,eps) (:283,:329-332,:350); needs compute_var */
  int32_t chunk_world;       /* 0 / 1: the Monte-Carlo samples of a (restart, component) are split into as many chunks as fill
                              * THIS device once.  W > 1: as many as fill W devices -- the chunking vbmc_elbo_shard_* use for a
                              * world of W ranks, so that an unsharded evaluation with chunk_world = W is their bit-exact
                              * reference (the chunk count only moves the summation order of the entropy partials) */
  int32_t restart_offset;    /* eps_mode 0: the device stream of restart r (column r of theta) is keyed by                    */
  int32_t restart_stride;    /* restart_offset + r * restart_stride (stride 0 is read as 1).  0 / 1: the position in this      */
                             /* batch.  A batch dealt over G devices (vbmc_elbo_batch_multi: device g gets restarts g, g+G,   */
                             /* ...) passes g / G, so that every restart draws what it would draw in the undivided batch      */
  int32_t no_jacobian;       /* 1: gradients with respect to sigma, lambda and the weights w themselves -- the JACOBIAN_FLAG = 0  */
                             /* form of gplogjoint / entmc_vbmc / entlb_vbmc (misc/gplogjoint.m:352-373, ent/entmc_vbmc.m:110-125, */
                             /* ent/entlb_vbmc.m:132-143) -- instead of log sigma, log lambda, eta.  Stand-alone forms only: no soft  */
                             /* bounds (bnd_lb NULL); the variance gradient follows suit (round 5: misc/gplogjoint.m:375-396          */
                             /* skipped).  0 (default): the transformed gradients negelcbo uses                                     */
  double* dvarG;             /* T x R  gradient of the diagonal variance of the expected log joint, gplogjoint's 4th output     */
                             /* (compute_var = 2 with compute_grad; misc/gplogjoint.m:375-413), or NULL                          */
  double* dG_s;              /* T x S x R  gradient of the expected log joint PER hyper-sample: gplogjoint's dF with avg_flag = 0  */
                             /* (misc/gplogjoint.m:206-271 per s, Jacobians :352-373, the averaging of :411 skipped); needs      */
                             /* compute_grad; honours no_jacobian.  ABI version 4.  NULL: not wanted                               */
  /* ---- ABI version 5 ---- */
  double* dvarG_s;           /* T x S x R  gradient of the diagonal variance PER hyper-sample: gplogjoint's dvarF with avg_flag = 0   */
                             /* (misc/gplogjoint.m:286-304 per s, Jacobians :375-396, the averaging of :407-409 skipped); needs      */
                             /* compute_grad with compute_var = 2; honours no_jacobian.  NULL: not wanted                           */
  int32_t plan_restarts;     /* 0: launch shapes follow THIS call's R.  P > 0: this call is a share of a batch of P restarts (dealt   */
                             /* over devices: restart_offset / restart_stride): the sample chunking, the log-joint kernel and its     */
                             /* splits are chosen as for a batch of P, so that every restart's results are BIT-IDENTICAL to the ones   */
                             /* the undivided batch evaluated with plan_restarts = P computes (a blocking call with plan_restarts 0    */
                             /* may take the walking entropy launch of wide batches: same draws, another order of summation over a      */
                             /* component's partial records, 1e-13) -- the opt-in exact mode of                                         */
                             /* vbmc_elbo_batch_multi / vbmc_elbo_multi_submit, which pass the field through.  Costs throughput where   */
                             /* a share is much smaller than the batch (launch shapes of a full chip on an eighth of the work).        */
} vbmc_elbo_args;

vbmc_status vbmc_elbo_batch(vbmc_ctx* ctx, const vbmc_gp* gp, const vbmc_elbo_args* args);

/*
 * The same pass, pipelined, for a stream of INDEPENDENT batches -- the candidates of the sieve are evaluated one after the
 * other with no dependence between them (misc/vpsieve_vbmc.m:74-78), and so are the full-ELCBO re-evaluations of
 * misc/vpoptimize_vbmc.m:134-165:
 *   vbmc_elbo_submit   validates and stages the inputs of one batch in the slot's own pinned block, enqueues the H2D, the
 *                      kernels and the packed D2H on the context's stream and returns WITHOUT waiting;
 *   vbmc_elbo_collect  waits for that slot's pass and fills the outputs named in args (F, dF, G, H, dG, dH, varG, varGss).
 * Four slots (0 .. 3; round 4: slot s runs on slot stream s & 1 of two streams the context creates at the first submit, two passes
 * deep each -- the head and tail of one pass overlap the entropy kernel of another and a stream never runs dry while the host collects
 * and re-submits; slots 2 and 3 exist for passes without a variance term; the variance forms run on the context's own stream, slots 0
 * and 1).  The two slot streams are chosen among candidates that the runtime places on different hardware queues and dispatch pipes
 * (measured at creation; vbmc_ctx_create raises GPU_MAX_HW_QUEUES to 8 ahead of its own first HIP call so that there are queues to choose
 * from -- unless the environment holds a value, VBMC_HW_QUEUES=0 forbids it, or another HIP user initialised the runtime first: see
 * INTEGRATION.md), and a slot stream is ordered after whatever the context's own stream still holds at submit (a surrogate being
 * uploaded, draws being produced).  COST OF THE FIRST SUBMIT of a context: the placement is MEASURED -- up to six candidate streams
 * per slot stream, each timed with two probe launches beside every stream it has to share the device with (a 45 us low-occupancy
 * kernel and a one-wave kernel, twice, with a synchronisation each): 1-6 ms once per context, device otherwise idle, before the
 * first batch is enqueued; VBMC_PLACE=0 skips the measurement and takes the first candidate (VBMC_DEBUG_PLACE=1 prints the ratios).
 * Create the context, and submit a first (warm-up) batch, outside a timed region.  While the device works on one batch the host stages the next, so that the device never waits for
 * the host between batches.  Measured at the headline shape: 2.49 ms per blocking call of 64 restarts, 2.39-2.42 ms per pipelined batch;
 * 0.37 / 0.33 ms for 8 restarts, 102 / 65 us for one.  Passes of one slot stream execute in submission order; each
 * slot must be collected before it is submitted again.  Results are bit-identical to vbmc_elbo_batch with the same args.
 * Not offered here: separate_K / I_sk / J_sjk / G_s / varG_s outputs and host-resident draws (eps_mode 1) -- their copies
 * go through pageable memory; use vbmc_elbo_batch.  The surrogate handle and the arrays named in args must stay valid until the
 * slot is collected (the inputs are copied at submit, the outputs are written at collect).  Other entry points of the same context may be called between a submit and
 * its collect (they run on the context's own stream, beside the passes in flight) -- except those that change or free the surrogate
 * a pass in flight reads (vbmc_gp_set_noise, vbmc_gp_free): collect first.  (Round 5, ABI 5: those two now wait for the slot streams
 * that hold a pass before they touch the surrogate -- the pass completes on the old data and stays collectable -- so a forgotten
 * collect costs a synchronisation, not a read of recycled memory.)
 *   vbmc_elbo_abandon  gives a slot back WITHOUT its results: waits for the pass in flight, if any, and clears the slot (a caller that
 *                      will not collect: an exception between submit and collect, an abandoned generator).  VBMC_OK on an idle slot.
 */
vbmc_status vbmc_elbo_submit(vbmc_ctx* ctx, const vbmc_gp* gp, const vbmc_elbo_args* args, int slot);
vbmc_status vbmc_elbo_collect(vbmc_ctx* ctx, const vbmc_elbo_args* args, int slot);
vbmc_status vbmc_elbo_abandon(vbmc_ctx* ctx, int slot);

/*
 * ONE evaluation (or a batch with fewer restarts than GPUs) sharded over `world` ranks, one process per GPU, each with a
 * full replica of the surrogate: rank g evaluates the expected-log-joint records of its hyper-samples (the iterations of
 * misc/gplogjoint.m:98 are independent until the averaging at :399-413) and the Monte-Carlo entropy partials of its share
 * of the sample chunks (ent/entmc_vbmc.m:49-104: the samples are independent) into one contiguous device block;
 *   vbmc_elbo_shard_size    number of doubles of that block (equal on every rank);
 *   vbmc_elbo_shard_begin   fills d_send (device memory of the caller, e.g. a torch tensor) and synchronises;
 *   -- the caller all-gathers the blocks in rank order (RCCL ncclAllGather over xGMI: torch.distributed
 *      all_gather_into_tensor; ~0.3 MB per rank at the headline shape) --
 *   vbmc_elbo_shard_finish  scatters the gathered blocks into the unsharded record layouts, runs the unsharded
 *                           fixed-order reductions and k_finalize on every rank and returns the outputs of
 *                           vbmc_elbo_batch: BIT-IDENTICAL to the 1-GPU evaluation with args.chunk_world = world (the
 *                           samples are split into `world` times as many chunks as one device needs, so that every rank's
 *                           share still fills its device; same chunking, same summation order => same bits).
 * Covers value + gradient without variance (compute_var = 0, separate_K = 0), device RNG (eps_mode 0): the optimiser-loop
 * call of misc/vpoptimize_vbmc.m:71.  args must be identical on all ranks and in all three calls.
 */
vbmc_status vbmc_elbo_shard_size(vbmc_ctx* ctx, const vbmc_gp* gp, const vbmc_elbo_args* args, int world, size_t* n_doubles);
vbmc_status vbmc_elbo_shard_begin(vbmc_ctx* ctx, const vbmc_gp* gp, const vbmc_elbo_args* args, int rank, int world, double* d_send);
vbmc_status vbmc_elbo_shard_finish(vbmc_ctx* ctx, const vbmc_gp* gp, const vbmc_elbo_args* args, int world, const double* d_gathered);

/* ---- more than one GPU: the communicator inside the library -----------------------------------------------------------
 * The path shards over the independent restarts of the sieve / the optimiser (misc/vpsieve_vbmc.m:74-78,
 * misc/vpoptimize_vbmc.m:49): rank g of G evaluates restarts g, g + G, g + 2G, ... against its own replica of the surrogate, and
 * the ONE exchange is an all-gather of the restarts' ELCBO values (RCCL ncclAllGather, device to device over xGMI), after which
 * every rank holds the identical vector and performs the identical stable sort (:82) -- index-identical order with no broadcast.
 * RCCL is reached from inside the library (dlopen of librccl on first use), so that a host without a distributed runtime of its
 * own -- the MATLAB process behind matlab/vbmc_hip_mex.cpp -- can use every GPU of a node.
 *
 *   vbmc_comm_create_all    ONE process drives ndev devices (devices == NULL: 0 .. ndev-1): creates a context per device and an
 *                           RCCL rank per device (ncclCommInitAll).  vbmc_comm_ctx(c, i) is the context of local device i.
 *   vbmc_comm_unique_id /   one process PER device (python -m torch.distributed.run, mpirun): rank 0 obtains the 128-byte id and
 *   vbmc_comm_create_rank   hands it to the others by any means (a file, torch.distributed, MPI); every process then joins with its
 *                           own context (ncclCommInitRank).  The context stays the caller's.
 *   vbmc_allgather_f64      every local device contributes `count` doubles (d_send[i], device memory on local device i) and
 *                           receives size * count doubles in rank order (d_recv[i]); enqueued on the contexts' streams inside
 *                           ncclGroupStart / ncclGroupEnd, then synchronised.  All-gather, never all-reduce: the exchange moves
 *                           the values it is given without arithmetic, and every rank holds the identical vector afterwards
 *                           (whether the VALUES equal the one-GPU batch's bit for bit is vbmc_elbo_batch_multi's business: see
 *                           plan_restarts there).
 *   vbmc_allgather_host_f64 the same for host blocks (send: local * count doubles, recv: size * count), staged through the
 *                           communicator's own device blocks.
 *   vbmc_gp_upload_all      vbmc_gp_upload on every local device (gps[local]): the surrogate is replicated, not sharded (25.6 MB
 *                           at the headline shape against 288 GB of HBM per device).
 *   vbmc_elbo_batch_multi   vbmc_elbo_batch for R restarts dealt over the ranks.  args is the UNDIVIDED batch (theta T x R, outputs
 *                           sized for R), identical on every rank.  On return F and varG hold ALL R values on every rank (the
 *                           all-gathered vectors as device memory of local device 0 received them); the other outputs are filled
 *                           for the restarts this process evaluated (all of them for vbmc_comm_create_all) and left untouched
 *                           elsewhere.  The device stream of restart r is keyed by its index r in the undivided batch
 *                           (restart_offset / restart_stride): every rank evaluates exactly the Monte-Carlo estimator the one-device
 *                           batch evaluates, sample for sample.  The values agree with vbmc_elbo_batch of the whole batch on one
 *                           device to the order of summation (relative 1e-13): launch shapes -- the number of sample chunks per
 *                           component, which sets the order in which the entropy partials are added -- are chosen for the restarts a
 *                           device actually holds, which is what strong scaling needs (8 restarts per device want other chunks than
 *                           64).  Where the two launches coincide (small batches) the values are bit-identical.  EXACT MODE (round
 *                           5, opt-in): args.plan_restarts = R makes every device choose its launch shapes for the undivided batch
 *                           -- then every value is BIT-IDENTICAL to vbmc_elbo_batch of the whole batch on one device, whatever the
 *                           number of devices, and a sieve sorted on 1 GPU and on 8 orders even exact ties the same way
 *                           (tests/test_gpu_comm.py: shares of 2 / 3 / 8 at a shape where the two modes choose different chunkings).
 *                           All RANKS of one call always see the identical gathered vectors, hence the identical sieve order, in
 *                           either mode.  eps_mode 0, or one shared host block of draws (eps_mode 1 with eps_shared).
 * Errors of these calls are reported by vbmc_comm_last_error.
 */
typedef struct vbmc_comm vbmc_comm;
vbmc_status vbmc_comm_create_all(int ndev, const int* devices, vbmc_comm** out);
vbmc_status vbmc_comm_unique_id(void* id128);
vbmc_status vbmc_comm_create_rank(vbmc_ctx* ctx, int rank, int size, const void* id128, vbmc_comm** out);
void vbmc_comm_destroy(vbmc_comm* comm);
int vbmc_comm_size(const vbmc_comm* comm);    /* ranks of the communicator                         */
int vbmc_comm_local(const vbmc_comm* comm);   /* devices this process drives                        */
int vbmc_comm_rank(const vbmc_comm* comm);    /* rank of local device 0                             */
vbmc_ctx* vbmc_comm_ctx(vbmc_comm* comm, int local);
const char* vbmc_comm_last_error(const vbmc_comm* comm);
vbmc_status vbmc_allgather_f64(vbmc_comm* comm, const double* const* d_send, double* const* d_recv, size_t count);
vbmc_status vbmc_allgather_host_f64(vbmc_comm* comm, const double* send, double* recv, size_t count);
vbmc_status vbmc_gp_upload_all(vbmc_comm* comm, int N, int D, int S, int Nhyp, int Ncov, int Nnoise, int meanfun,
                               const double* X, const double* hyp, const double* alpha, const double* L, const double* sW1,
                               const uint8_t* Lchol, vbmc_gp** gps);
void vbmc_gp_free_all(vbmc_comm* comm, vbmc_gp** gps);
vbmc_status vbmc_elbo_batch_multi(vbmc_comm* comm, const vbmc_gp* const* gps, const vbmc_elbo_args* args);
/* The pipelined form of vbmc_elbo_batch_multi for streams of INDEPENDENT batches (the candidates of misc/vpsieve_vbmc.m:74-78), as
 * vbmc_elbo_submit / vbmc_elbo_collect are for one device: submit stages this process's restarts, enqueues the passes, the one
 * ncclAllGather and the copy of the gathered vectors to pinned host memory and returns; collect waits and fills the caller's arrays
 * (same contents as vbmc_elbo_batch_multi).  slot = 0 .. 3: up to four batches in flight, on two streams per device (the exchange itself
 * stays on each context's own stream, ordered after the pass).  Device RNG (eps_mode 0), no per-component or
 * per-hyper-sample outputs.  A steady-state call allocates nothing: the per-device argument structs, staging vectors, exchange
 * blocks and the pinned landing block live in the communicator's slot.  A failure local to one rank (resource error, missing
 * surrogate) is reported AFTER the rank has entered the collective with an all-NaN block, so that the other ranks are never left
 * waiting (vbmc_elbo_batch_multi does the same). */
vbmc_status vbmc_elbo_multi_submit(vbmc_comm* comm, const vbmc_gp* const* gps, const vbmc_elbo_args* args, int slot);
vbmc_status vbmc_elbo_multi_collect(vbmc_comm* comm, const vbmc_elbo_args* args, int slot);

/*
 * [x,f,xtab,ftab,iter] = fminadam(@(t) negelcbo_vbmc(t,beta,vp,gp,Ns,1,compute_var,~,thetabnd), x0, [], [],
 *                                 TolFun, MaxIter, master_stepsize)          (utils/fminadam.m:1-104,
 * call site misc/vpoptimize_vbmc.m:127) for R chains in lock-step, entirely on the device: per
 * iteration one batched ELBO+grad pass and the Adam update (:48-61), every 20 iterations the slope /
 * random-walk stopping test (:65-81); the host only polls R flags on those iterations.  args->theta
 * holds the R starting points x0 (T x R); args->seed + iter keys the MC draws of iteration iter
 * (eps_mode must be 0).  Outputs (any may be NULL): x T x R (mean of the last 20 iterates, :96),
 * f R (:97), iters R, xtab T x MaxIter x R and ftab MaxIter x R (first iters(r) entries filled), xmid T x R: per chain the
 * iterate with the smallest recorded objective, theta_lst(idx_mid,:) with [~,idx_mid] = min(fval_lst) of
 * misc/vpoptimize_vbmc.m:133 -- the one thing that caller reads from the tables, so that it need not ask for them (T x MaxIter x R
 * doubles with MaxIter = 1e4).
 */
vbmc_status vbmc_adam_batch(vbmc_ctx* ctx, const vbmc_gp* gp, const vbmc_elbo_args* args, double TolFun, int MaxIter,
                            double step_min, double step_max, double step_decay, double* x, double* f, int32_t* iters,
                            double* xtab, double* ftab, double* xmid);

/* Writes the exact standard-normal block eps (D x Ns/2 x K x R) that eps_mode 0 consumes for
 * `seed`, so that a host oracle can be fed the same draws (test hook; entmc_vbmc.m:53). */
vbmc_status vbmc_rng_dump(vbmc_ctx* ctx, int D, int K, int R, int Ns, uint64_t seed, double* eps_host);

/* Reporting hook: which instantiation of the Monte-Carlo entropy kernel (vbmc_amd/csrc/entropy_mfma.h) a D-dimensional,
 * K-component mixture runs on in dense mode: qs = ceil((D+2)/4), kt = 16-component k-tiles per wave, hv = waves per workgroup,
 * tail = values per lane of the component tail (0: none).  Returns 1; 2 when the shape is in the small class (K <= 16, D <= 12) and
 * runs on the lane-per-sample kernel (vbmc_amd/csrc/entropy_lane.h: qs = padded dimension DT, kt = padded component count KP,
 * hv = waves per workgroup); 0 when the plain VALU kernel serves it.  bench.py labels the kernel it measures with it. */
int vbmc_entropy_plan(int D, int K, int* qs, int* kt, int* hv, int* tail);

/* Test hook: y = exp(x) evaluated by the hot-loop device implementations (0: polynomial, 1 / 2: 256-entry table with the two- /
 * one-constant reduction, 3: the Monte-Carlo entropy kernel's exponential as built, 4 / 5: its cubic / quadratic form). */
vbmc_status vbmc_test_exp(vbmc_ctx* ctx, int n, int variant, const double* x, double* y);

/* Test hook (ABI version 6): which kernels the last ELBO pass enqueued on ctx (vbmc_elbo_batch, vbmc_elbo_submit, vbmc_adam_batch's
 * last iteration, a shard's vbmc_elbo_shard_begin) used for the entropy and for the expected log joint; 0 where none ran.  The
 * launch forms are chosen by shape and by the VBMC_*_KERNEL / VBMC_LJ_CO switches, and some requests fall back silently (a forced
 * matrix-core log joint whose moment exchange exceeds 64 KB runs the VALU kernel): tests that force a form check it here. */
enum {
  VBMC_ENTFORM_LB = 1,          /* k_entlb: the deterministic bound (Ns = 0)                                                     */
  VBMC_ENTFORM_VALU = 2,        /* k_entropy<DT>                                                                                  */
  VBMC_ENTFORM_MFMA = 3,        /* k_entropy_mfma                                                                                 */
  VBMC_ENTFORM_LANE = 4         /* k_entropy_lane                                                                                 */
};
enum {
  VBMC_LJFORM_VALU_WAVE = 1,    /* separate k_logjoint<DT>, one wave per cell                                                     */
  VBMC_LJFORM_VALU_SPLIT = 2,   /* separate k_logjoint<DT>, the training set split over four waves per cell                       */
  VBMC_LJFORM_MFMA_GRAD = 3,    /* k_logjoint_mfma<DT, true>                                                                      */
  VBMC_LJFORM_MFMA_VALUE = 4,   /* k_logjoint_mfma<DT, false> (value-only passes)                                                 */
  VBMC_LJFORM_ROLE_MFMA = 5,    /* a role inside the k_entropy_mfma launch                                                        */
  VBMC_LJFORM_ROLE_LANE = 6     /* a role inside the k_entropy_lane launch                                                        */
};
vbmc_status vbmc_ctx_last_launch(vbmc_ctx* ctx, int* ent_form, int* lj_form);

/* Reporting hook (an addition, backward compatible: VBMC_ABI_VERSION is unchanged): what the variance stage of the last ELBO pass with
 * compute_var != 0 enqueued on this context (vbmc_amd/csrc/elbo_pass.h: Pass::variance), recorded there from the expressions the
 * launches themselves use.  compute_var = 0: no such pass has run on this context yet.  Tests that mean to exercise a form of the
 * triangular step or a Gram kernel assert it here. */
enum {
  VBMC_VARSOLVE_TRSM2 = 1,      /* k_trsm2<solve_width>: a workgroup per 16 columns, solve_width = 4 or 8 row-block slots (N <= 512 / 1024) */
  VBMC_VARSOLVE_SLAB = 2        /* k_trsm_fwd<solve_width> / k_trsm_bwd<solve_width>: a wave per slab of solve_width = 16, 8, 4, 2, 1 columns */
};
enum {
  VBMC_VARGRAM_WAVE = 1,        /* k_var_gram: one wave per pair (the diagonal approximation)                                     */
  VBMC_VARGRAM_MFMA = 2         /* k_var_gram_mfma: 16 x 16 tiles of the upper triangle on the matrix cores (the full matrix)     */
};
typedef struct vbmc_var_launch_info {
  uint32_t struct_size;  /* sizeof(vbmc_var_launch_info) of the caller */
  int32_t compute_var;   /* of that pass: 1 full matrix, 2 diagonal approximation; 0: none yet */
  int32_t tri_gemm;      /* 1: V = inv(L') Z as a product with the explicit inverse (k_tri_gemm) for the Cholesky samples, no forward substitution */
  int32_t symm;          /* 1: k_symm ran (a low-noise sample is present) */
  int32_t fwd_solve;     /* VBMC_VARSOLVE_* of the forward substitution; 0 with tri_gemm */
  int32_t bwd_solve;     /* VBMC_VARSOLVE_* of the backward substitution (the variance gradient alone); 0 without */
  int32_t solve_width;   /* slots or slab columns of those substitutions; 0 where neither ran */
  int32_t gram;          /* VBMC_VARGRAM_* */
  int32_t vgrad;         /* 1: k_vargrad and k_var_sample ran */
  int32_t sample_lds;    /* dynamic LDS of k_var_sample in bytes; 0 where it did not run */
  int32_t final_lds;     /* dynamic LDS of k_var_final in bytes */
} vbmc_var_launch_info;
vbmc_status vbmc_ctx_last_variance(vbmc_ctx* ctx, vbmc_var_launch_info* out);

/* Reporting hook (an addition, backward compatible: VBMC_ABI_VERSION is unchanged): the launch form one call of vbmc_gp_pred /
 * vbmc_gp_quad (quad != 0) on Nstar points would take on this context's device, want_ks != 0 for the callers that read the cross-kernel
 * matrix themselves (the IQR acquisition functions).  It launches nothing and allocates nothing on the device: it evaluates the functions
 * the launch itself reads (vbmc_amd/csrc/gp_pred.h: pred_needs_slab, pred_row_groups, pred_forms), so what it reports is what runs.
 * The form depends on N, D, S, Nstar, on gp.post(s).Lchol, on the number of compute units and on the VBMC_PRED_FUSED switch; a sweep
 * beyond the chunk size (1 GiB of cross-kernel values) repeats the launch per chunk and is not described here.  Refuses what
 * vbmc_gp_pred / vbmc_gp_quad refuse.  Tests that mean to exercise a form assert it here. */
typedef struct vbmc_pred_plan_info {
  uint32_t struct_size;  /* sizeof(vbmc_pred_plan_info) of the caller */
  int32_t num_cu;        /* compute units of the device */
  int32_t slab;          /* 1: the variance comes from slab solves (k_pred_slab), N beyond the resident-tile range */
  int32_t cw;            /* columns per slab of the triangular solves at this N (16 in the resident-tile range) */
  int32_t fused;         /* 1: k_pred_fused / k_quad_fused; 0: k_pred_ks + k_gp_pred (or k_pred_slab) */
  int32_t QS;            /* ceil(D / 4): steps of the MFMA distance blocks */
  int32_t PT;            /* fused: resident 16-point tiles per workgroup (1..3); else 0 */
  int32_t RS;            /* fused: workgroups sharing the row tiles of one unit (1..4); else 1 */
  int32_t npass;         /* fused: passes of PT tiles over the points; else 0 */
  int32_t units;         /* fused: npass * S (hyper-sample, pass) units; a workgroup walks several when units * RS > grid; else 0 */
  int32_t grid;          /* workgroups of the variance kernel: k_pred_fused's x, k_gp_pred's x * y * z, k_pred_slab's x * y */
  int32_t PZ;            /* two-kernel form: slices of the point tiles over gridDim.z; else 1 */
  int32_t maxg;          /* row groups per hyper-sample, the largest over the samples (fused: RS; slab: 1) */
  int32_t nblk;          /* 16-row tiles of the training set, ceil(N / 16) */
  int32_t Rmax, Rmin;    /* resident row tiles of a group of the row-group table (what k_gp_pred holds in LDS), largest and
                            smallest over all groups and samples; 0 for the slab form */
} vbmc_pred_plan_info;
vbmc_status vbmc_pred_plan(vbmc_ctx* ctx, const vbmc_gp* gp, int Nstar, int want_ks, int quad, vbmc_pred_plan_info* out);

/* Device-memory helpers for callers without their own allocator (MEX). */
vbmc_status vbmc_device_alloc(vbmc_ctx* ctx, size_t bytes, void** dptr);
vbmc_status vbmc_device_free(vbmc_ctx* ctx, void* dptr);
vbmc_status vbmc_memcpy_h2d(vbmc_ctx* ctx, void* dst, const void* src, size_t bytes);
vbmc_status vbmc_memcpy_d2h(vbmc_ctx* ctx, void* dst, const void* src, size_t bytes);

/*
 * The variational posterior in the caller's own parameter space (additions, backward compatible: VBMC_ABI_VERSION is unchanged):
 * vbmc_pdf.m, vbmc_rnd.m, vbmc_moments.m:23-28 and vbmc_kldiv.m:70-88 with the variable transform of shared/warpvars_vbmc.m.
 *
 * vbmc_vp_desc: one posterior.  Caller-owned host data, column-major fp64; nothing is retained after return.  type == NULL is an
 * empty trinfo (the identity, warpvars_vbmc.m:47-58).  Per-variable types 0 (unbounded: (x - mu) / delta), 1 (lower bounded:
 * log(x - lb)), 2 (upper bounded: log(ub - x)) and 3 (logit of (x - lb) / (ub - lb), then (. - mu) / delta) are accelerated; types
 * 4 .. 13 answer VBMC_ERR_UNSUPPORTED.  scale (NULL or all ones: none) and R (NULL: none; D x D column-major, y = u R) are the
 * optional scale row and rotation of misc/warp_input_vbmc.m:72-73.  D <= 32, K <= 512, else VBMC_ERR_UNSUPPORTED.
 *
 * Randomness (the convention of vbmc_acq_is_setup): sample i owns the slots B[(D + 1) i ..]; slot 0 is a uniform in (0, 1) that
 * catrnd (vbmc_rnd.m:111-123) uses for an unbalanced draw or for a remainder draw of the balanced split, slots 1 + d are standard
 * normals.  With block == NULL they come from Philox counters keyed by seed; a non-null block of (D + 1) M doubles replays
 * vbmc_vp_rnd_rng_dump's, bit-identically in I and in the transformed-space samples.  The balanced split (vbmc_rnd.m:57-77): the
 * M = sum floor(w N) + ceil(sum w_extra) sample ids below sum floor(w N) take their component from the cumulative counts, the
 * others from catrnd(w_extra); randperm(numel(I), N) is a bijection pi of [0, M) keyed by seed, built from integer operations alone;
 * output row r is sample pi(r) (unbalanced: M = N and pi is the identity).  Every entry point below generates "row r -> sample pi(r)",
 * so that vbmc_vp_moments and vbmc_vp_kldiv equal vbmc_vp_rnd followed by the host's mean / cov resp. by vbmc_vp_pdf on the same seed.
 *
 *   vbmc_vp_pdf            y (N) and, where dy != NULL, dy (N x D) = vbmc_pdf(vp, X, origflag, logflag, transflag, df) at the rows of
 *                          X (N x D).  df = +-Inf or 0: the Gaussian mixture; df > 0 the multivariate t, df < 0 the product of
 *                          univariate t of |df| degrees of freedom.  Computed in the log domain: where the reference's sum of
 *                          densities underflows the result is -Inf resp. 0, as there; a value that the reference loses only in the
 *                          division by the Jacobian stays finite.  The gradient exists for the Gaussian mixture in the transformed
 *                          space (origflag = 0, or an empty trinfo); the forms the reference stops on (vbmc_pdf.m:82, :100, :117)
 *                          and the uncorrected plain-density gradient in the original space answer VBMC_ERR_UNSUPPORTED.
 *   vbmc_vp_rnd            X (N x D) and, where I != NULL, I (N, from 0) = vbmc_rnd(vp, N, origflag, balanceflag, df).  Gaussian
 *                          components only: a finite non-zero df and balanceflag = 2 (the reference's 'gp') answer
 *                          VBMC_ERR_UNSUPPORTED.  Original-space samples are clamped into [lb + eps(lb), ub - eps(ub)]
 *                          (warpvars_vbmc.m:456-459).
 *   vbmc_vp_moments        mubar (D) and, where Sigma != NULL, Sigma (D x D) of Ns >= 2 balanced draws in the original space
 *                          (vbmc_moments.m:23-28).  The samples never reach memory: shifted sums about the image of the mixture
 *                          mean, per-workgroup partials added in index order (no atomics), Sigma = (S2 - S1 S1' / Ns) / (Ns - 1).
 *   vbmc_vp_kldiv          kls[2] of vbmc_kldiv.m:70-88 (the non-Gaussian branch, the final max(., 0) included).  Direction 1 draws
 *                          from vp1 with (seed, block1), direction 2 from vp2 with (seed + 1, block2); xx1 / xx2 (Ns x D, NULL: not
 *                          wanted) are exactly vbmc_vp_rnd's rows for those.  Both densities are evaluated at the original-space
 *                          point through each posterior's own direct transform, as the reference does.  lb / ub of the two
 *                          posteriors must be equal, else VBMC_ERR_UNSUPPORTED.
 *   vbmc_vp_rnd_rng_dump   host function: the block a seed stands for.  B receives (D + 1) M doubles, M <= N + K (size it for
 *                          N + K samples); perm (N, NULL: not wanted) receives pi(r).  Either may be NULL.
 */
typedef struct vbmc_vp_desc {
  uint32_t struct_size;
  int32_t D, K;
  const double* mu;       /* D x K */
  const double* sigma;    /* K */
  const double* lambda;   /* D */
  const double* w;        /* K */
  const int32_t* type;    /* D, or NULL: empty trinfo */
  const double* lb;       /* D: trinfo.lb_orig */
  const double* ub;       /* D: trinfo.ub_orig */
  const double* tmu;      /* D: trinfo.mu */
  const double* tdelta;   /* D: trinfo.delta */
  const double* scale;    /* D, or NULL */
  const double* R;        /* D x D column-major, or NULL: trinfo.R_mat */
} vbmc_vp_desc;
vbmc_status vbmc_vp_pdf(vbmc_ctx* ctx, const vbmc_vp_desc* vp, int64_t N, const double* X, int origflag, int logflag, int transflag, double df, double* y, double* dy);
vbmc_status vbmc_vp_rnd(vbmc_ctx* ctx, const vbmc_vp_desc* vp, int64_t N, int origflag, int balanceflag, double df, uint64_t seed, const double* block, double* X, int32_t* I);
vbmc_status vbmc_vp_moments(vbmc_ctx* ctx, const vbmc_vp_desc* vp, int64_t Ns, uint64_t seed, const double* block, double* mubar, double* Sigma);
vbmc_status vbmc_vp_kldiv(vbmc_ctx* ctx, const vbmc_vp_desc* vp1, const vbmc_vp_desc* vp2, int64_t Ns, uint64_t seed, const double* block1, const double* block2, double* kls, double* xx1, double* xx2);
vbmc_status vbmc_vp_rnd_rng_dump(uint64_t seed, int64_t N, int D, int K, int balanceflag, const double* w, double* B, int64_t* perm);

/*
 * vbmc_vp_mtv: the marginal total variation distances of vbmc_mtv.m between two posteriors (an addition, backward compatible:
 * VBMC_ABI_VERSION is unchanged).  Ns balanced draws of each posterior in the original space -- vp1 with (seed, block1), vp2 with
 * (seed + 1, block2), exactly vbmc_vp_rnd's rows, held on the device (more than 1 GiB per posterior: VBMC_ERR_UNSUPPORTED) --; per
 * posterior and dimension the mesh bounds of vbmc_mtv.m:55-63 (lb / ub of the two posteriors may differ), shared/kde1d.m on nkde mesh
 * points (binning, cosine transform, the root of fixed_point inside the bracket of root(), inverse transform) and the normalisation of
 * vbmc_mtv.m:68; per dimension 0.5 qtrapz |s1 - s2| over nquad points of each of the three segments between the four sorted mesh
 * ends, s1 / s2 the not-a-knot cubic splines through the two densities (0 outside their own mesh).  The unique count of kde1d.m:46
 * is Ns - max(0, c_lo - 1) - max(0, c_hi - 1), c_lo / c_hi the draws that sit on the column's clamp ends lb + eps(lb), ub - eps(ub).
 * A column of the draws whose range is zero or not finite gives NaN in that dimension alone.  A column that reaches the reference's
 * fminbnd branch (no bracket below 0.1, kde1d.m:136-138) answers VBMC_ERR_UNSUPPORTED, as does whatever vbmc_vp_rnd refuses; sample
 * matrices in place of a posterior (vbmc_mtv.m:35-38) are not part of the ABI.  Column c = p D + d is posterior p (0, 1), dimension d.
 * Every output pointer may be NULL.  Results are identical from run to run.
 */
typedef struct vbmc_mtv_args {
  uint32_t struct_size;
  int32_t nkde;           /* 0: 8192; else a power of two in 256 .. 16384 (vbmc_mtv.m:51) */
  int32_t nquad;          /* 0: 100000; else 2 .. 2^20 (vbmc_mtv.m:76) */
  int64_t Ns;             /* >= 2 */
  uint64_t seed;
  const double* block1;   /* NULL, or vbmc_vp_rnd_rng_dump's block for (seed, vp1) */
  const double* block2;   /* NULL, or the block for (seed + 1, vp2) */
  double* mtv;            /* D */
  double* xx1;            /* Ns x D column-major */
  double* xx2;            /* Ns x D column-major */
  double* mesh;           /* 2 x D x 2: MIN, MAX of column c at [2 c], [2 c + 1] */
  int32_t* counts;        /* 2 x D x nkde: column c at [c nkde ..] */
  int64_t* nuniq;         /* 2 x D */
  double* tstar;          /* 2 x D: the root t* of kde1d.m:53 */
  double* density;        /* 2 x D x nkde: the normalised densities of vbmc_mtv.m:68, :71 */
} vbmc_mtv_args;
vbmc_status vbmc_vp_mtv(vbmc_ctx* ctx, const vbmc_vp_desc* vp1, const vbmc_vp_desc* vp2, const vbmc_mtv_args* args);

/*
 * vbmc_vp_corner: the data of a corner plot -- what vbmc_plot.m:12-15 and private/vbmc_iterplot.m:21, :47 hand to utils/cornerplot.m --
 * in one call (an addition, backward compatible: VBMC_ABI_VERSION is unchanged).
 *
 * THE SAMPLES.  With a posterior: the Ns rows of vbmc_vp_rnd(vp, Ns, origflag, balanceflag, Inf, seed, block), exactly (vbmc_plot
 * draws with balanceflag 0, vbmc_iterplot with 1).  With vp == NULL: the caller's matrix X_in (Ns x D column-major) and D, what
 * cornerplot(Xs, ...) of vbmc_examples.m takes; an entry that is not finite answers VBMC_ERR_INVALID.  2 <= Ns <= 2^28 and
 * Ns x D doubles <= 1 GiB (else VBMC_ERR_UNSUPPORTED); D <= 32, K <= 512, transform types 0 .. 3 through the posterior; D = 1 has no
 * pairs.
 *
 * THE BOUNDS.  bounds == NULL: each column's min and max (cornerplot.m:93-96, :116).  Given bounds (2 x D, finite, lo < hi, else
 * VBMC_ERR_INVALID) are vbmc_iterplot's case: a sample outside them is dropped from every count and is still counted in N (kde2d.m:79,
 * :193).  bounds_out receives the ones used.
 *
 * hist      nbins x D counts on nbins equal bins between the column's bounds: bin k is the largest k with lo + k (hi - lo) / nbins <= x,
 *           a sample on hi goes to the last bin, a sample outside the bounds is not counted; the probability is count / Ns.  A
 *           DEPARTURE: cornerplot.m:129 calls histogram(x, 40), whose "nice" bin edges are toolbox code outside the reference tree.
 * quant     nq x D: utils/quantile1.m:37-72 of every column over all Ns rows at the probabilities p (at most 16, in [0, 1]): the
 *           median's own branch (:40-45) for p = {0.5}, the caps of :53-54 and the "exact" and "same" copies of :59-70.  The device
 *           selects exact order statistics (no sort of the matrix); the ranks and the interpolation of :57 are the host's.
 * Per pair pp of dimensions d1 < d2 in cornerplot.m:154-155's order (d1 = 0 .. D-2 outer, d2 = d1+1 .. D-1 inner), P = D (D - 1) / 2,
 * kde2d.m:74-212 on res x res (Botev's diffusion estimator: ndhist on 0:1/res:1 of the rescaled samples, dct2d, the root of
 * t - evolve(t) with N = Ns inside the bracket of root(), t_x / t_y, idct2d):
 *   density    res x res x P column-major, row the d2 mesh, column the d1 mesh, as kde2d.m:103 returns it (idct2d has one
 *              transpose); negative values are eps (:104).  The mesh MIN : scaling / (res - 1) : MAX (:105) is the caller's to build
 *              from bounds_out.
 *   bandwidth  2 x P (:107).
 *   tstar      P: the root; counts2 res x res x P int32: ndhist's counts, row the d1 bin, column the d2 bin.
 * The cosine transforms are the direct sums dct2d / idct2d stand for (the reference goes through fft), the root comes from a
 * bisection-safeguarded secant iteration down to a few ulps (the reference's fzero stops at its own tolerance).
 *
 * DEGENERATE AND REFUSED.  A column of zero range without given bounds: its histogram is zero, every pair that contains it is NaN in
 * density, bandwidth and tstar, the other outputs are unaffected.  A pair whose equation has no bracket below 0.1 is the fminbnd
 * branch of kde2d.m:208-210: VBMC_ERR_UNSUPPORTED, the message names the pair.  res: 0 is 64 (cornerplot.m:104), else 16, 32 or 64;
 * anything else VBMC_ERR_UNSUPPORTED (kde2d's own default of 256 does not fit one workgroup's LDS tile).  nbins: 0 is 40 (:102), else
 * 1 .. 1024.  Refused in this order: a NULL context, a wrong struct_size, the arguments, the posterior.  Every output pointer may be
 * NULL.  Results are identical from run to run.
 */
typedef struct vbmc_corner_args {
  uint32_t struct_size;
  int32_t D;              /* with X_in; ignored with a posterior */
  int32_t res;            /* 0: 64; else 16, 32 or 64 */
  int32_t nbins;          /* 0: 40; else 1 .. 1024 */
  int32_t nq;             /* 0 .. 16 */
  int32_t origflag;       /* the draws' space (vbmc_plot: 1) */
  int32_t balanceflag;    /* 0 or 1 */
  int32_t reserved_;
  int64_t Ns;             /* >= 2 */
  uint64_t seed;
  const double* block;    /* NULL, or vbmc_vp_rnd_rng_dump's block for (seed, vp) */
  const double* X_in;     /* Ns x D column-major with vp == NULL, else NULL */
  const double* bounds;   /* NULL, or 2 x D: lo, hi of dimension d at [2 d], [2 d + 1] */
  const double* p;        /* nq */
  double* xx;             /* Ns x D column-major: the samples used */
  double* bounds_out;     /* 2 x D */
  int32_t* hist;          /* nbins x D */
  double* quant;          /* nq x D */
  double* density;        /* res x res x P */
  double* bandwidth;      /* 2 x P */
  double* tstar;          /* P */
  int32_t* counts2;       /* res x res x P */
} vbmc_corner_args;
vbmc_status vbmc_vp_corner(vbmc_ctx* ctx, const vbmc_vp_desc* vp, const vbmc_corner_args* args);

/*
 * vbmc_vp_diagnostics: the pair loop of vbmc_diagnostics.m:116-127 over R runs in one call (an addition, backward compatible:
 * VBMC_ABI_VERSION is unchanged).  Run i draws ONCE: the rows of vbmc_vp_rnd(vps[i], Ns, 1, 1, seed + i).  (The reference draws afresh
 * for every pair; here every pair's estimate is the reference's estimator on Ns balanced draws of each posterior, and only the
 * estimates of different pairs are correlated.)
 *   kl_mat[i + R j]      KL(run i || run j) of vbmc_kldiv.m:72-77, :88 on run i's draws, both densities through each posterior's own
 *                        direct transform: what vbmc_vp_kldiv(vps[i], vps[j], Ns, seed + i) returns in kls[0] (to the bit, unless a
 *                        density comes within e^40 of the smallest normal double: there it is formed as vbmc_pdf.m:56-60 forms it,
 *                        exponentials that have lost their bits included, where vbmc_vp_kldiv keeps full precision).  Zero diagonal.  The
 *                        runs' bounds may differ: a draw outside run j's support has a density that is not a number there, which
 *                        the rule of :76 replaces by realmin.
 *   mtv[d + D (i + R j)] vbmc_mtv.m on the two runs' sample matrices: the mesh bounds of :55-63 with lb = -Inf, ub = +Inf (:35-38,
 *                        :44-47), so that a run's mesh, counts, bandwidth and density depend on that run's draws alone; the unique
 *                        count by the clamp-end rule of vbmc_vp_mtv with the run's own clamp ends; kde1d, the normalisation and the
 *                        integral as in vbmc_vp_mtv.  Symmetric in (i, j), zero for i = j.  A run's degenerate column gives NaN in
 *                        that dimension of every pair the run takes part in.
 *   maxmtv_mat[i + R j]  the maximum of mtv over the dimensions that are not NaN (MATLAB's max, vbmc_diagnostics.m:124); NaN if all are.
 * Stage outputs per run, column c = i D + d, as vbmc_mtv_args has them per posterior.  Every output pointer may be NULL.
 * 2 <= R <= 32; all runs the same D (else VBMC_ERR_INVALID); posteriors, transforms, Ns, nkde and nquad as vbmc_vp_mtv takes them.  A
 * column that reaches kde1d's fminbnd branch answers VBMC_ERR_UNSUPPORTED and the message names the run and the dimension.  A NULL
 * context, a wrong struct_size and R < 2 are refused before anything else is read.  Results are identical from call to call, and a
 * run's stage outputs and draws are identical whichever other runs are in the call.
 */
typedef struct vbmc_diag_args {
  uint32_t struct_size;
  int32_t nkde;           /* 0: 8192; else a power of two in 256 .. 16384 */
  int32_t nquad;          /* 0: 100000; else 2 .. 2^20 */
  int64_t Ns;             /* >= 2 */
  uint64_t seed;
  double* kl_mat;         /* R x R column-major */
  double* mtv;            /* D x R x R */
  double* maxmtv_mat;     /* R x R */
  double* mesh;           /* R x D x 2: MIN, MAX of column c at [2 c], [2 c + 1] */
  int32_t* counts;        /* R x D x nkde: column c at [c nkde ..] */
  int64_t* nuniq;         /* R x D */
  double* tstar;          /* R x D */
  double* density;        /* R x D x nkde */
  double* xx;             /* Ns x D x R: run i's draws, column-major, at [Ns D i ..] */
} vbmc_diag_args;
vbmc_status vbmc_vp_diagnostics(vbmc_ctx* ctx, int32_t R, const vbmc_vp_desc* const* vps, const vbmc_diag_args* args);

/*
 * vbmc_vp_mode: the mode of the variational posterior, vbmc_mode.m, in one call (an addition, backward compatible: VBMC_ABI_VERSION is
 * unchanged).  One launch optimises from every start; the optimiser is the library's own, not fmincon.
 *
 * THE OBJECTIVE.  origflag = 0: log q(u), the mixture in the transformed space.  origflag != 0: the log density in the original space,
 * log q(T(x)) - logJ, which the library maximises over u as g(u) = log q(u) - logprob(u), logprob what warpvars_vbmc(u, 'logprob',
 * trinfo) returns (vbmc_pdf.m:115): T is a bijection, so the maximiser over x is the inverse transform of the maximiser over u.  The
 * objective stays in the log domain: a start whose density underflows still has a finite objective and a gradient, and is optimised
 * (the reference hands fmincon -Inf there).
 *
 * THE STARTS are the means of S = min(nmax, K) components.  nmax >= K: all of them in index order.  nmax < K: the objective is
 * evaluated at all K means and the first nmax of a stable ascending sort of its negative are kept (vbmc_mode.m:23-28).  With origflag
 * the reference ranks by the original-space density evaluated AT the transformed-space means (vbmc_mode.m:24); the library ranks by
 * the objective at the starts themselves.
 *
 * THE OPTIMISER, per start: BFGS on an inverse-Hessian approximation that starts from diag((sigma_c lambda_d)^2) of the start's own
 * component c, direction d = -H grad F for F = -g, backtracking candidates u + 2^-k d, k = 0 .. 31, the first with
 * F(u + t d) <= F(u) + 1e-4 t grad F' d taken; the update is skipped unless y's > 1e-10 |y| |s|.  It stops with
 *   VBMC_MODE_STOP_GRAD     max_d |grad_d| <= tol_grad (tested before every iteration, the start included),
 *   VBMC_MODE_STOP_STEP     no candidate was acceptable,
 *   VBMC_MODE_STOP_MAXITER  max_iter iterations were made (0: 200; at most 1000).
 * The objective never decreases along an optimisation: fs[s] >= f0[s].
 *
 * THE ANSWER is the start with the largest fs, the first of equal ones: idx, fval = fs[idx], and x (D) = xs(idx, :).  us is the
 * maximiser in the transformed space; xs is us for origflag = 0 and otherwise its inverse transform with vbmc_vp_rnd's clamp to
 * [lb + eps(lb), ub - eps(ub)] (the reference keeps sqrt(eps) from the bounds).  Per start s < S (the arrays are S long, us and xs
 * S x D column-major; each may be NULL): start_comp the component (from 0), f0 the objective at the start, iters, nfev the objective
 * evaluations (the line search evaluates four candidates at a time) and stop.  S_out receives S.
 *
 * Posteriors and transforms as vbmc_vp_pdf takes them (D <= 32, K <= 512, types 0 .. 3, scale, rotation, no trinfo); types 4 .. 13:
 * VBMC_ERR_UNSUPPORTED.  A NULL context, a wrong struct_size, tol_grad that is not positive, max_iter outside 0 .. 1000, a missing x,
 * fval or idx and a posterior that is not finite are refused, in this order, with VBMC_ERR_INVALID before anything runs.  Results are
 * identical from call to call.
 */
#define VBMC_MODE_STOP_GRAD 1
#define VBMC_MODE_STOP_STEP 2
#define VBMC_MODE_STOP_MAXITER 3
typedef struct vbmc_mode_args {
  uint32_t struct_size;
  int32_t nmax;           /* <= 0: 20 */
  int32_t origflag;
  int32_t max_iter;       /* 0: 200; else 1 .. 1000 */
  double tol_grad;        /* > 0; the shims pass 1e-6 */
  double* x;              /* D */
  double* fval;           /* 1 */
  int32_t* idx;           /* 1: the start that won, from 0 */
  int32_t* S_out;         /* 1 */
  int32_t* start_comp;    /* S */
  double* f0;             /* S */
  double* us;             /* S x D column-major */
  double* xs;             /* S x D column-major */
  double* fs;             /* S */
  int32_t* iters;         /* S */
  int32_t* nfev;          /* S */
  int32_t* stop;          /* S: VBMC_MODE_STOP_* */
} vbmc_mode_args;
vbmc_status vbmc_vp_mode(vbmc_ctx* ctx, const vbmc_vp_desc* vp, const vbmc_mode_args* args);

/* Test hook: one cosine transform of kde1d (forward: dct1d with a2 = (a_k / 2)^2, a2 may be NULL; inverse: idct1d) of C columns of n
 * values (n a power of two in 256 .. 16384, column c at [c n ..]) by the kernel of vbmc_vp_mtv (kernel 0) or of vbmc_vp_diagnostics
 * (kernel 1), launched reps times; out / a2 are the last launch's, ms[reps] (may be NULL) each launch's HIP-event duration. */
vbmc_status vbmc_test_dct(vbmc_ctx* ctx, int n, int C, int inverse, int kernel, int reps, const double* in, double* out, double* a2, double* ms);

/*
 * vbmc_gp_surrogate_sample: samples of the GP surrogate itself (misc/gpsample_vbmc.m -> gplite/gplite_sample.m with method 'parallel';
 * an addition, backward compatible: VBMC_ABI_VERSION is unchanged).  The whole chain runs on the device.
 *
 * THE TARGET is log_gpfun (gplite_sample.m:109-117) on the first two outputs of gplite_pred -- the noisy pair [ymu, ys2] -- averaged
 * over ALL S hyper-samples as gplite_pred.m:154-164 does: S > 1: ybar = sum ymu_s / S, vy = sum (ymu_s - ybar)^2 / (S - 1),
 * ys2 = sum ys2_s / S + vy (sums over s in index order); S = 1: that sample's pair.  (VarThresh == 0 or not finite) and beta == 0:
 * y = ybar.  Otherwise y = ybar - (ys2 - VarThresh) where ys2 >= VarThresh, and everywhere y -= beta sqrt(ys2).  A value that is not
 * finite is -Inf.
 *
 * THE SAMPLER is the ensemble slice sampler of vbmc_acq_is_sample with its indexed uniform block, E INDEPENDENT ensembles of W walkers
 * (E has nothing to do with S; the block is 64 x H x E x M, vbmc_gp_surrogate_sample_rng_dump writes the one a seed stands for).  Each
 * ensemble discards `burnin` walker moves (-1: ceil(Ns / 5), the reference's, whatever E is) and records every thin-th move after them
 * until it has Nm = ceil(Ns / E).  Row r = e + E i of X is record i of ensemble e; rows >= Ns are dropped.  A round is three launches:
 * the sampler's step, the prediction of every candidate of every ensemble under every hyper-sample, the combination into the target.
 * spec and chunk change the number of rounds, never a bit of the results.
 *
 * THE START: x0 (W x D x E), or, with x0 == NULL, the W E unbalanced transformed-space draws of vbmc_vp_rnd(vp, W E, 0, 0, seed), draw
 * w + W e being walker w of ensemble e (gpsample_vbmc.m:41).  Either is clipped into [LB, UB] (gplite_sample.m:102).
 *
 * THE NOISE ESTIMATE (gpsample_vbmc.m:30-38), with sn2new != NULL: Nnn (0: 20000) draws vbmc_vp_rnd(vp, Nnn, 0, 0, seed + 1) kept on
 * the device, per draw the nearest row of X_rescaled in units of gplengthscale (first minimum wins), sn2_avg the mean of sn2new there
 * (a fixed-order reduction) and VarThresh = max(1, sn2_avg), which replaces the argument.  gplengthscale (D), X_rescaled (N x D) and
 * sn2new (N, the mean over hyper-samples of the training noise) are the caller's O(N D S) set-up, as for vbmc_acq_eval.
 *
 * origflag: X is warpvars_vbmc(X, 'inv', vp.trinfo) with its clamp, as vbmc_vp_rnd returns original-space draws; 0: the transformed
 * space.  vp may be NULL where nothing needs it (x0 given, no noise estimate, origflag = 0).
 *
 * Inputs: D, S (the GP's), Ns >= 1, 1 <= E <= 64, W even with 4 <= W <= 2 (D + 1) (0: 2 (D + 1)), thin >= 1, burnin, LB / UB (D,
 * finite, LB < UB), beta, VarThresh (Inf: none); spec, chunk, max_steps, max_shrink, rng_mode, seed, U, Mmax as in vbmc_is_sample_args.
 * Outputs (any may be NULL): X (Ns x D), Xt (Nm x D x E, the transformed-space records), logp (E x Nm), x0_out (W x D x E, the clipped
 * start), varthresh_out, sn2_avg_out (0 without the estimate), sn2_nn (Nnn: sn2new at each draw's nearest row), funccount, performed,
 * rounds[2].
 *
 * VBMC_ERR_UNSUPPORTED: whatever vbmc_gp_pred refuses, N beyond the range in which the prediction keeps inv(L') resident (N <= 1136),
 * E Nm D doubles above 1 GiB, a vp the vp tools refuse.  VBMC_ERR_INVALID: what vbmc_acq_is_sample answers so (W, the box, thin, spec,
 * the caps, the uniform block, D / S that are not the GP's, a GP without vbmc_gp_set_noise), Ns < 1, E outside 1 .. 64, vp == NULL
 * where it is needed, a noise estimate without X_rescaled or gplengthscale, a start of zero density ("a starting point has zero
 * density").  The context stays usable after any error.
 */
typedef struct vbmc_gs_args {
  uint32_t struct_size;      /* = sizeof(vbmc_gs_args) */
  int32_t D, S;              /* the GP's */
  int32_t E, W, thin, burnin, spec, max_steps, max_shrink, chunk;
  int32_t rng_mode;          /* 0 device generator, 1 parity */
  int32_t Mmax;              /* rng_mode 1: half-moves in U */
  int32_t origflag;
  int32_t Nnn;               /* draws of the noise estimate (0: 20000) */
  int32_t reserved_;
  int64_t Ns;
  uint64_t seed;
  const double* U;           /* rng_mode 1: 64 x H x E x Mmax */
  const double* LB;          /* D */
  const double* UB;          /* D */
  const double* x0;          /* W x D x E, or NULL */
  double beta;
  double VarThresh;
  const double* X_rescaled;  /* N x D */
  const double* gplengthscale; /* D */
  const double* sn2new;      /* N, or NULL: no noise estimate */
  double* X;                 /* Ns x D */
  double* Xt;                /* Nm x D x E */
  double* logp;              /* E x Nm */
  double* x0_out;            /* W x D x E */
  double* varthresh_out;
  double* sn2_avg_out;
  double* sn2_nn;            /* Nnn */
  int64_t* funccount;
  int64_t* performed;
  int64_t* rounds;           /* 2 */
} vbmc_gs_args;
vbmc_status vbmc_gp_surrogate_sample(vbmc_ctx* ctx, const vbmc_gp* gp, const vbmc_vp_desc* vp, const vbmc_gs_args* args);
vbmc_status vbmc_gp_surrogate_sample_rng_dump(uint64_t seed, int E, int H, int M, double* U);

#ifdef __cplusplus
}
#endif
#endif /* VBMC_HIP_H */

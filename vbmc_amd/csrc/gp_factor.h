// Host side of the GP factorisation (gplite_core.m:33-102), shared by the entry points that factorise: vbmc_gp_post and vbmc_gp_nlz
// (abi_gp.hip: hyper-parameters uploaded by the call, gp_factorize) and the two device-resident halves of gplite_train
// (abi_gp_train.hip: hyper-parameters written by a kernel, GpObjWork).  It owns the host noise model, the check of the GP model, the
// workspace of the factorisation, the launches of the value and gradient paths of gplite_nlZ, gp_factorize with its options, the
// optimistic-then-checked retry, and the scope guard of a handle under construction.
#pragma once
#include <algorithm>
#include <cmath>
#include <functional>
#include <limits>

#include "dev_layout.h"
#include "elbo_pass.h"   // copy_f64_small
#include "gp_factor_kernels.h"
#include "gp_nlz_kernels.h"

namespace {

// ------------------------------------------------------------------------------------------
// the noise model on the host, O(N)
// ------------------------------------------------------------------------------------------
// gplite_noisefun.m:176-210: returns per-point sn2 (length N)
void noise_vector(const int32_t nf[3], const double* hn, int N, const double* y, const double* s2, std::vector<double>& sn2) {
  int idx = 0;
  double base;
  if (nf[0] == 0) base = 2.220446049250313e-16;
  else { base = std::exp(2.0 * hn[idx]); idx++; }
  sn2.assign(N, base);
  if (nf[1] == 1 && s2) { for (int n = 0; n < N; ++n) sn2[n] += s2[n]; }
  else if (nf[1] == 2 && s2) { double c = std::exp(hn[idx]); for (int n = 0; n < N; ++n) sn2[n] += c * s2[n]; idx++; }
  else if (nf[1] == 2) idx++;
  if (nf[2] == 1) {
    if (y) {
      double ythr = hn[idx], w2 = std::exp(2.0 * hn[idx + 1]);
      for (int n = 0; n < N; ++n) { double zz = std::max(0.0, ythr - y[n]); sn2[n] += w2 * zz * zz; }
    }
  }
}

int noise_nhyp(const int32_t nf[3]) { return (nf[0] == 1) + (nf[1] == 2) + 2 * (nf[2] == 1); }

// gplite_noisefun.m:164-210, gradient part: dsn2 as Nnoise x N (constant models replicated over n)
void noise_grad(const int32_t nf[3], const double* hn, int N, const double* y, const double* s2, int Nnoise, double* dsn2) {
  std::fill(dsn2, dsn2 + (size_t)Nnoise * N, 0.0);
  int idx = 0;
  if (nf[0] == 1) { const double v = 2.0 * std::exp(2.0 * hn[idx]); for (int n = 0; n < N; ++n) dsn2[(size_t)idx * N + n] = v; idx++; }
  if (nf[1] == 2) { const double c = std::exp(hn[idx]); for (int n = 0; n < N; ++n) dsn2[(size_t)idx * N + n] = s2 ? c * s2[n] : 0.0; idx++; }
  if (nf[2] == 1 && y) {
    const double ythr = hn[idx], w2 = std::exp(2.0 * hn[idx + 1]);
    for (int n = 0; n < N; ++n) {
      const double zz = std::max(0.0, ythr - y[n]);
      dsn2[(size_t)idx * N + n] = zz > 0 ? 2.0 * w2 * (ythr - y[n]) : 0.0;
      dsn2[(size_t)(idx + 1) * N + n] = 2.0 * w2 * zz * zz;
    }
  }
}

// ------------------------------------------------------------------------------------------
// the GP models the factorisation accelerates
// ------------------------------------------------------------------------------------------
struct GpModel { int Ncov = 0, Nnoise = 0, Nmean = 0; };
// who: the gplite function in whose name a mismatch of Nhyp is reported (gplite_post, gplite_nlZ).  given_ncov: the caller's own
// count of covariance hyper-parameters if it states one (0: it does not), held against the model's with the identity.
vbmc_status gp_model_check(vbmc_ctx* ctx, const char* who, int N, int D, int Nhyp, int meanfun, const int32_t noisefun[3], int given_ncov, GpModel& m) {
  if (D > VBMC_LIM_D) return set_err(ctx, VBMC_ERR_UNSUPPORTED, "D = %d > %d not accelerated", D, VBMC_LIM_D);
  if (!(meanfun == 0 || meanfun == 1 || meanfun == 4))
    return set_err(ctx, VBMC_ERR_UNSUPPORTED, "gplite mean function %d not accelerated (0,1,4 are)", meanfun);
  m.Ncov = D + 1; m.Nnoise = noise_nhyp(noisefun); m.Nmean = meanfun == 0 ? 0 : (meanfun == 1 ? 1 : 2 * D + 1);
  if (Nhyp != m.Ncov + m.Nnoise + m.Nmean || (given_ncov != 0 && given_ncov != m.Ncov))
    return set_err(ctx, VBMC_ERR_INVALID, "%s:dimmismatch Number of hyperparameters mismatched with GP model specification.", who);
  // right-hand-side slabs of the triangular solves live in LDS: 16 columns wide up to N = 1136, narrower beyond (trsm_cw_for);
  // the Cholesky panel moves to a global scratch block when it no longer fits
  if (trsm_cw_for(N) == 0) return set_err(ctx, VBMC_ERR_UNSUPPORTED, "N = %d > %d not accelerated", N, trsm_max_n());
  return VBMC_OK;
}
// the noise functions whose hyper-parameters a kernel lays out (the gplite_train entry points, in front of gp_model_check)
vbmc_status gp_noise_range_check(vbmc_ctx* ctx, const int32_t noisefun[3]) {
  for (int i = 0; i < 3; ++i)
    if (noisefun[i] < 0 || noisefun[i] > (i == 1 ? 2 : 1))
      return set_err(ctx, VBMC_ERR_UNSUPPORTED, "gplite noise function [%d %d %d] not accelerated", noisefun[0], noisefun[1], noisefun[2]);
  return VBMC_OK;
}

// ------------------------------------------------------------------------------------------
// the workspace and the launches
// ------------------------------------------------------------------------------------------
// The device blocks of B factorisations at (N, D): scaled inputs and their row norms, the matrices (kernel matrix, then its factor),
// the Cholesky's failure indices, the residual y - m, z = R' \ r, alpha with the failure indices as doubles behind it (pfd), the
// inverses of the factor's diagonal blocks and, where the 16 x N panel of the Cholesky no longer fits the LDS (N > 1120, chol_mfma.h),
// its global scratch block.
struct GpWork {
  TmpBuf dXc, daa, dA, dpf, dr, dz, dal, dfinv, dPg;
  double* pfd = nullptr;
  vbmc_status alloc(vbmc_ctx* ctx, int N, int D, int B) {
    HIP_TRY(ctx, dXc.alloc(ctx, (size_t)B * N * D * 8));
    HIP_TRY(ctx, daa.alloc(ctx, (size_t)B * N * 8));
    HIP_TRY(ctx, dA.alloc(ctx, (size_t)B * N * N * 8));
    HIP_TRY(ctx, dpf.alloc(ctx, (size_t)B * sizeof(int)));
    HIP_TRY(ctx, dr.alloc(ctx, (size_t)B * N * 8));
    HIP_TRY(ctx, dz.alloc(ctx, (size_t)B * N * 8));
    HIP_TRY(ctx, dal.alloc(ctx, ((size_t)B * N + B) * 8));
    HIP_TRY(ctx, dfinv.alloc(ctx, (size_t)B * TRSM_NBLK(N) * 256 * 8));
    if (chol2_needs_gpanel(N, true)) HIP_TRY(ctx, dPg.alloc(ctx, (size_t)B * 16 * (size_t)(((N + 15) >> 4) << 4) * 8));
    pfd = dal.as<double>() + (size_t)B * N;
    return VBMC_OK;
  }
};

// The launches of the factorisation path: every argument is a device pointer.
inline void gp_launch_scale(hipStream_t st, int N, int D, int S, int Nhyp, int moff, int meanfun, const double* X, const double* hyp,
                            double* Xc, double* aa, const double* y, double* r) {
  hipLaunchKernelGGL(k_gp_scale, dim3(4, S), dim3(256), 0, st, N, D, Nhyp, X, hyp, Xc, aa, moff, meanfun, y, r);
}
// one try of the jittered Cholesky: kernel matrices of the active vectors, factorisation, block inverses, z = R' \ r
inline hipError_t gp_launch_try(hipStream_t st, int N, int D, int S, int Nhyp, const double* hyp, const double* sn2, const double* scal,
                                const unsigned char* act, GpWork& w) {
  DISPATCH_GPDT(D, hipLaunchKernelGGL((k_gp_build<DT>), dim3((N + GPB_T - 1) / GPB_T, (N + GPB_T - 1) / GPB_T, S), dim3(256), 0, st, N, D,
                                      Nhyp, hyp, w.dXc.as<double>(), w.daa.as<double>(), sn2, scal, act, w.dA.as<double>()));
  return chol2_launch(N, S, w.dA.as<double>(), w.dpf.as<int>(), act, w.dPg.p ? w.dPg.as<double>() : nullptr, st, w.dfinv.as<double>(), w.pfd,
                      w.dr.as<double>(), w.dz.as<double>());
}
// alpha = R \ z / sl: the backward half of the two-sided solve
inline void gp_launch_alpha(hipStream_t sa, int N, int S, const double* A, const double* finv, const unsigned char* on, const double* z,
                            double* al, const double* scal) {
  if (N <= ASOLVE1_THREADS)
    hipLaunchKernelGGL(k_alpha_solve1, dim3(S), dim3(ASOLVE1_THREADS), 0, sa, N, A, finv, on, z, al, 1, scal);
  else
    hipLaunchKernelGGL(k_alpha_solve, dim3(S), dim3(ASOLVE_THREADS), (size_t)((TRSM_NBLK(N) << 4) + 16) * sizeof(double), sa, N, A, finv, on, z,
                       al, 1, scal);
}
// The gradient leg of gplite_nlZ for B factors: Kinv*sl = L\(L'\eye(N)) (:240) as T'T with T = inv(L') -- one triangular solve of the
// identity into TT (k_tri_inverse2 / k_tri_inverse, from the column block's own rows down) and a rank-k update on the matrix cores
// into Ki (k_syrk_tt, tile form syrk_form; only the upper triangle is formed: the part k_nlz_grad reads) -- then the partial sums of
// k_nlz_grad over the noise-model derivatives dsn2.  Neither the inverse nor the product needs alpha.  combined (few matrices of
// moderate order): alpha's backward solve, not yet enqueued, runs as one more workgroup of the inverse's launch.  join: alpha is
// being computed on another stream; k_nlz_grad waits for that event.
inline vbmc_status gp_launch_grad(vbmc_ctx* ctx, hipStream_t st, int N, int D, int B, int Nhyp, int Nnoise, const double* hyp, const double* scal,
                                  const unsigned char* on, const double* dsn2, GpWork& w, double* TT, double* Ki, double* part, bool combined,
                                  int syrk_form, hipEvent_t join) {
  if (combined) {
    const int nblk = TRSM_NBLK(N);
    if (nblk <= TRI2_W * 4)
      hipLaunchKernelGGL((k_tri_inverse2_alpha<4>), dim3(nblk + 1, B), dim3(64 * TRI2_W), 0, st, N, w.dA.as<double>(), w.dfinv.as<double>(), on, TT,
                         w.dz.as<double>(), w.dal.as<double>(), scal);
    else
      hipLaunchKernelGGL((k_tri_inverse2_alpha<8>), dim3(nblk + 1, B), dim3(64 * TRI2_W), 0, st, N, w.dA.as<double>(), w.dfinv.as<double>(), on, TT,
                         w.dz.as<double>(), w.dal.as<double>(), scal);
  } else {
    HIP_TRY(ctx, tri_inverse_launch(st, N, B, w.dA.as<double>(), w.dfinv.as<double>(), on, TT, 1));
  }
  syrk_tt_launch(st, N, B, TT, on, Ki, false, syrk_form);
  if (join) HIP_TRY(ctx, hipStreamWaitEvent(st, join, 0));
  const int nt1 = (N + NLZ_T - 1) / NLZ_T;
  DISPATCH_GPDT(D, hipLaunchKernelGGL((k_nlz_grad<DT>), dim3(nt1, nt1, B), dim3(256), 0, st, N, D, Nhyp, Nnoise, hyp, w.dXc.as<double>(),
                                      w.daa.as<double>(), Ki, w.dal.as<double>(), scal, dsn2, part));
  return VBMC_OK;
}
// the closing kernel of gplite_nlZ: out = [nlZ B | failure indices B | dnlZ B x Nhyp]
inline void gp_launch_nlz_final(hipStream_t st, int N, int D, int B, int Nhyp, int Nnoise, int Nmean, int meanfun, int ntile, int grad,
                                const double* X, const double* y, const double* hyp, const double* A, const double* al, const double* scal,
                                const double* part, const double* pfd, double* out) {
  DISPATCH_GPDT(D, hipLaunchKernelGGL((k_nlz_final<DT>), dim3(B), dim3(256), 0, st, N, D, Nhyp, Nnoise, Nmean, meanfun, ntile, grad, X, y, hyp, A, al,
                                      scal, part, pfd, out));
}

// ------------------------------------------------------------------------------------------
// gp_factorize: kernel matrices, jittered Cholesky and alpha for S hyper-parameter vectors of the call, left on the device
// ------------------------------------------------------------------------------------------
struct GpFactorOpts {
  const char* who = "";
  // true (vbmc_gp_post): a matrix that is still not positive definite after the retries is refused; false (vbmc_gp_nlz): that
  // hyper-parameter vector is marked as failed (NaN result, gplite_train.m:542-546) and the call goes on
  bool fail_is_error = false;
  // The first try's failure indices are NOT waited for.  Almost every factorisation succeeds at the first try (the retries exist for
  // hyper-parameter vectors at the edge of the prior): everything downstream is enqueued as if it had, the indices travel with the
  // caller's results (GpWork::pfd -> GpFactor::h_pfd) and the caller looks at them at its own final synchronisation (gp_factor_ok); if
  // one is set it repeats the call with the retry loop -- one host round trip (25 us of an otherwise idle device) and one copy less per call
  bool optimistic = false;
  // alpha's backward solve runs on the context's second stream while the caller inverts the factor on the first (vbmc_gp_nlz with a
  // gradient, few matrices) -- two latency-bound kernels that do not depend on each other; the caller waits for ctx->ev_join
  // (GpFactor::alpha_event) before it reads alpha
  bool alpha_aside = false;
  bool defer_alpha = false;     // the caller launches alpha's backward solve itself (gp_launch_grad's combined form)
  size_t pin_out = 0;           // doubles of the pinned block, behind the inputs, that the caller's results come back through (GpFactor::pin_out)
  // the caller's extra inputs riding in the packed upload: extra_in doubles, filled by fill_extra (GpFactor::dExtra on the device)
  size_t extra_in = 0;
  std::function<void(double*)> fill_extra;
};

struct GpFactor {
  GpModel m;
  int cw = 16;                                      // slab width of the triangular solves at this N (trsm_cw_for)
  std::vector<double> sn2all, scal, sn2min;         // host copies: S x N noise, S x 4 {sn2div, mult, lchol, sl}
  std::vector<unsigned char> lch, failed;           // Lchol flag; 1 = Cholesky still failing after 10 retries
  bool any_inv = false;
  size_t tlds = 0;
  double* pin_out = nullptr;
  const double* h_pfd = nullptr;   // optimistic: where the caller has copied the failure indices (w.pfd) to, with its own results
  bool unchecked = false;
  bool alpha_event = false;        // alpha is being computed on the second stream: wait for ctx->ev_join before reading it
  GpWork w;
  TmpBuf dIn, dX, dy, dhyp, dsn2, dscal, dact, dones, dninv, dlch, dExtra;   // dIn: the packed inputs (the others are its windows)
};

// The packed upload, one pinned block and one copy: [X | y | hyp | sn2 | scal | flags | caller's extras].  flags: four arrays of S
// bytes, ones | needinv | active | lchol, rounded up together to whole doubles.  total: the block in doubles.
struct GpPackLayout {
  DevLayout L;
  DevWin<double> X, y, hyp, sn2, scal, extra;
  DevWin<unsigned char> ones, needinv, active, lchol;
  size_t total;
  GpPackLayout(int N, int D, int S, int Nhyp, size_t extra_in) {
    X = L.add<double>((size_t)N * D); y = L.add<double>(N); hyp = L.add<double>((size_t)Nhyp * S); sn2 = L.add<double>((size_t)S * N);
    scal = L.add<double>((size_t)S * 4);
    ones = L.add<unsigned char>(S); needinv = L.add<unsigned char>(S); active = L.add<unsigned char>(S); lchol = L.add<unsigned char>(S);
    L.round_up(sizeof(double));
    extra = L.add<double>(extra_in);
    total = L.count();
  }
};

// vbmc_gp_post's extras in that block, what a device-resident posterior needs beyond the factorisation:  gpc (nG) | sn2_eff (S) | meanX (D) | mult (S)
struct GpPostExtra {
  DevLayout L;
  DevWin<double> gpc, sn2_eff, meanX, mult;
  GpPostExtra(int D, int S, size_t nG) { gpc = L.add<double>(nG); sn2_eff = L.add<double>(S); meanX = L.add<double>(D); mult = L.add<double>(S); }
};

// gplite_nlZ's block of results, what k_nlz_final writes:  nlZ (B) | failure indices (B) | dnlZ (B x Nhyp, with a gradient only)
struct GpNlzOut {
  DevLayout L;
  DevWin<double> nlZ, pfd, dnlZ;
  GpNlzOut(int B, int Nhyp, bool grad) { nlZ = L.add<double>(B); pfd = L.add<double>(B); dnlZ = L.add_if<double>(grad, (size_t)B * Nhyp); }
};
// The small blocks of the surrogate a rank-one update makes, windows of one pooled block:
//   X_new (N1 x D) | meanX (D) | hyp | gpc (nG) | sn2_eff | mult (S each) | lchol (S bytes, rounded up to whole doubles)
// X_new and meanX come up from the host (upload: their doubles); the rest is copied from the surrogate it extends.
struct GpRank1Block {
  DevLayout L;
  DevWin<double> X, meanX, hyp, gpc, sn2_eff, mult;
  DevWin<unsigned char> lchol;
  size_t upload;
  GpRank1Block(int N1, int D, int S, int Nhyp, size_t nG) {
    X = L.add<double>((size_t)N1 * D); meanX = L.add<double>(D);
    upload = L.count();
    hyp = L.add<double>((size_t)Nhyp * S); gpc = L.add<double>(nG); sn2_eff = L.add<double>(S); mult = L.add<double>(S);
    lchol = L.add<unsigned char>(S);
    L.round_up(sizeof(double));
  }
  void bind(vbmc_gp& g, void* b) const {
    g.X = X.at(b); g.d_meanX = meanX.at(b); g.hyp = hyp.at(b); g.gpc = gpc.at(b); g.d_sn2 = sn2_eff.at(b); g.d_mult = mult.at(b); g.d_lchol = lchol.at(b);
  }
};

// host: noise vectors, Lchol flags, the constants of the first try (gplite_core.m:33-40,67)
void gp_host_noise(int N, int S, int Nhyp, const int32_t noisefun[3], const double* y, const double* s2, const double* hyp, GpFactor& f,
                   std::vector<unsigned char>& needinv) {
  f.sn2all.assign((size_t)S * N, 0.0); f.scal.assign((size_t)S * 4, 0.0); f.sn2min.assign(S, 0.0);
  f.lch.assign(S, 0); f.failed.assign(S, 0);
  needinv.assign(S, 0);
  std::vector<double> tmp;
  for (int s = 0; s < S; ++s) {
    noise_vector(noisefun, hyp + (size_t)s * Nhyp + f.m.Ncov, N, y, s2, tmp);
    std::copy(tmp.begin(), tmp.end(), f.sn2all.begin() + (size_t)s * N);
    const double mn = *std::min_element(tmp.begin(), tmp.end());
    f.sn2min[s] = mn;
    f.lch[s] = mn >= 1e-6 ? 1 : 0;
    needinv[s] = f.lch[s] ? 0 : 1;
    f.any_inv |= !f.lch[s];
    f.scal[s * 4 + 0] = f.lch[s] ? mn : 1.0;  // sn2div
    f.scal[s * 4 + 1] = 1.0;                  // sn2_mult
    f.scal[s * 4 + 2] = f.lch[s];
    f.scal[s * 4 + 3] = f.lch[s] ? f.scal[s * 4 + 0] : 1.0;   // sl = sn2div * sn2_mult (:82,:96); rewritten if a retry inflates the noise
  }
}

inline hipError_t gp_factor_try(hipStream_t st, int N, int D, int S, int Nhyp, GpFactor& f) {
  return gp_launch_try(st, N, D, S, Nhyp, f.dhyp.as<double>(), f.dsn2.as<double>(), f.dscal.as<double>(), f.dact.as<unsigned char>(), f.w);
}

// The jittered Cholesky with its flags waited for: up to 10 tries, noise multiplier x10 per failure (gplite_core.m:77-80,91-94).  On
// return f.scal holds the multipliers and sl, on the device too; f.failed marks what still fails (fail_is_error: refused instead).
vbmc_status gp_factor_checked(vbmc_ctx* ctx, hipStream_t st, int N, int D, int S, int Nhyp, bool fail_is_error, GpFactor& f) {
  std::vector<double>& scal = f.scal;
  std::vector<unsigned char> active(S, 1);
  std::vector<int> pf(S);
  bool pending = true, retried = false;
  for (int iter = 0; iter < 10 && pending; ++iter) {
    if (iter > 0) {   // (the first try's copies are part of the packed block)
      HIP_TRY(ctx, hipMemcpyAsync(f.dscal.p, scal.data(), (size_t)S * 4 * 8, hipMemcpyHostToDevice, st));
      HIP_TRY(ctx, hipMemcpyAsync(f.dact.p, active.data(), S, hipMemcpyHostToDevice, st));
    }
    HIP_TRY(ctx, gp_factor_try(st, N, D, S, Nhyp, f));
    HIP_TRY(ctx, hipMemcpyAsync(pf.data(), f.w.dpf.p, (size_t)S * sizeof(int), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    pending = false;
    for (int s = 0; s < S; ++s) {
      if (!active[s]) continue;
      if (pf[s] > 0) { scal[s * 4 + 1] *= 10.0; pending = true; retried = true; }  // sn2_mult = sn2_mult*10
      else active[s] = 0;
    }
  }
  if (pending) {
    // MATLAB leaves the loop with the last multiplier even when chol still fails; we refuse instead.
    if (fail_is_error)
      return set_err(ctx, VBMC_ERR_NOT_POSDEF, "gplite_core: Cholesky failed after 10 noise-inflation retries");
    for (int s = 0; s < S; ++s) f.failed[s] = active[s];
  }
  if (retried) {   // (without a retry the packed block already carries sl)
    for (int s = 0; s < S; ++s) scal[s * 4 + 3] = f.lch[s] ? scal[s * 4 + 0] * scal[s * 4 + 1] : 1.0;  // sl (:82,:96)
    HIP_TRY(ctx, hipMemcpyAsync(f.dscal.p, scal.data(), (size_t)S * 4 * 8, hipMemcpyHostToDevice, st));
  }
  return VBMC_OK;
}

// Device schedule: ONE upload of the packed inputs; k_gp_scale (scaled inputs, row norms AND the residual y - m); k_gp_build; k_chol2,
// which also leaves the inverses of the diagonal blocks (the triangular solves' Finv) and the forward solve z = R' \ (y - m) behind;
// the backward half of alpha's solve with the 1 / sl scaling folded in.
vbmc_status gp_factorize(vbmc_ctx* ctx, int N, int D, int S, int Nhyp, int meanfun, const int32_t noisefun[3], const double* X,
                         const double* y, const double* s2, const double* hyp, const GpFactorOpts& o, GpFactor& f) {
  if (N <= 0 || D <= 0 || S <= 0 || !X || !y || !hyp || !noisefun)
    return set_err(ctx, VBMC_ERR_INVALID, "%s: bad arguments", o.who);
  VB_TRY(gp_model_check(ctx, o.fail_is_error ? "gplite_post" : "gplite_nlZ", N, D, Nhyp, meanfun, noisefun, 0, f.m));
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  std::vector<unsigned char> needinv, ones(S, 1);
  gp_host_noise(N, S, Nhyp, noisefun, y, s2, hyp, f, needinv);

  // Inputs: ONE pinned block, one asynchronous copy (eight hipMemcpyAsync from pageable memory were each staged and waited for by
  // the runtime, ~100 us of host time in a call whose kernels take 0.36 ms); the caller's results come back through the same block
  const GpPackLayout lay(N, D, S, Nhyp, o.extra_in);
  VB_TRY(ensure_pin(ctx, (lay.total + o.pin_out) * 8 + 8));
  double* hin = (double*)ctx->pin;
  f.pin_out = hin + lay.total;
  lay.X.put(hin, X); lay.y.put(hin, y); lay.hyp.put(hin, hyp); lay.sn2.put(hin, f.sn2all.data()); lay.scal.put(hin, f.scal.data());
  lay.ones.put(hin, ones.data()); lay.needinv.put(hin, needinv.data());
  lay.active.put(hin, ones.data()); lay.lchol.put(hin, f.lch.data());                        // every vector starts active
  if (o.extra_in && o.fill_extra) o.fill_extra(lay.extra.at(hin));
  HIP_TRY(ctx, f.dIn.alloc(ctx, lay.L.bytes()));
  double* din = f.dIn.as<double>();
  f.dX.view(lay.X.at(din)); f.dy.view(lay.y.at(din)); f.dhyp.view(lay.hyp.at(din)); f.dsn2.view(lay.sn2.at(din)); f.dscal.view(lay.scal.at(din));
  f.dones.view(lay.ones.at(din)); f.dninv.view(lay.needinv.at(din)); f.dact.view(lay.active.at(din)); f.dlch.view(lay.lchol.at(din));
  f.dExtra.view(lay.extra.at(din));
  VB_TRY(f.w.alloc(ctx, N, D, S));
  // (small blocks by a kernel that reads the pinned block over the host link instead of the copy engine: the hand-over from a DMA
  // copy to the first kernel of the stream is 8-9 us on top of the copy's 6.5 -- elbo_pass.h: copy_by_kernel)
  HIP_TRY(ctx, copy_f64_small(ctx, st, din, hin, lay.total, hipMemcpyHostToDevice));
  gp_launch_scale(st, N, D, S, Nhyp, f.m.Ncov + f.m.Nnoise, meanfun, f.dX.as<double>(), f.dhyp.as<double>(), f.w.dXc.as<double>(),
                  f.w.daa.as<double>(), f.dy.as<double>(), f.w.dr.as<double>());

  if (o.optimistic) {
    HIP_TRY(ctx, gp_factor_try(st, N, D, S, Nhyp, f));
    f.unchecked = true;
  } else {
    VB_TRY(gp_factor_checked(ctx, st, N, D, S, Nhyp, o.fail_is_error, f));
  }

  // alpha = L\(L'\(y-m)) / sl  (:102): the forward half came out of the factorisation (w.dz)
  f.cw = trsm_cw_for(N);
  f.tlds = TRSM_LDS_BYTES_CW(N, f.cw);
  hipStream_t sa = st;
  f.alpha_event = false;
  if (o.defer_alpha) { HIP_TRY(ctx, hipGetLastError()); return VBMC_OK; }
  if (o.alpha_aside && ctx->ev_fork && ctx->ev_join && ctx_aux(ctx)) {
    HIP_TRY(ctx, hipEventRecord(ctx->ev_fork, st));
    HIP_TRY(ctx, hipStreamWaitEvent(ctx->aux, ctx->ev_fork, 0));
    sa = ctx->aux;
    f.alpha_event = true;
  }
  gp_launch_alpha(sa, N, S, f.w.dA.as<double>(), f.w.dfinv.as<double>(), f.dones.as<unsigned char>(), f.w.dz.as<double>(), f.w.dal.as<double>(),
                  f.dscal.as<double>());
  if (f.alpha_event) HIP_TRY(ctx, hipEventRecord(ctx->ev_join, sa));
  HIP_TRY(ctx, hipGetLastError());
  return VBMC_OK;
}

// after the caller's synchronisation: did the optimistic first try succeed for every matrix?
bool gp_factor_ok(const GpFactor& f, int S) {
  if (!f.unchecked) return true;
  if (!f.h_pfd) return false;            // nobody brought the flags back: take the checked path
  for (int s = 0; s < S; ++s)
    if (f.h_pfd[s] > 0.0) return false;
  return true;
}

// impl(optimistic, &ok) enqueues its call over an optimistic factorisation, synchronises and sets ok = gp_factor_ok; where a first
// try had failed it returns at once, and the call is made again with the noise-inflation loop.
template <class Impl>
vbmc_status gp_optimistic_then_checked(Impl impl) {
  bool ok = true;
  const vbmc_status st = impl(true, &ok);
  return ok ? st : impl(false, &ok);
}

// ------------------------------------------------------------------------------------------
// A handle under construction: freed with its device blocks on every path that does not release it
// ------------------------------------------------------------------------------------------
template <class T, void (*Free)(vbmc_ctx*, T*)>
struct HandleGuard {
  vbmc_ctx* ctx;
  T* h;
  HandleGuard(vbmc_ctx* c, T* p) : ctx(c), h(p) {}
  HandleGuard(const HandleGuard&) = delete;
  ~HandleGuard() { if (h) Free(ctx, h); }
  T* operator->() const { return h; }
  T* release() { T* q = h; h = nullptr; return q; }
};
using GpGuard = HandleGuard<vbmc_gp, vbmc_gp_free>;

}  // namespace

// C-ABI entry points for the gplite GP surrogate: vbmc_sq_dist, vbmc_gp_post, vbmc_gp_nlz, vbmc_gp_set_noise, vbmc_gp_pred,
// vbmc_gp_quad and the rank-1 append (include/vbmc_hip.h).  The factorisation with its jitter-retry loop (gplite_core.m:77-80,91-94)
// is gp_factor.h, the prediction gp_pred.h; here: the calls' own launches, the posterior's assembly and the copies back.
#include <algorithm>
#include <cmath>
#include <limits>

#include "ctx_core.h"    // gp_constants, gp_upload_impl
#include "gp_factor.h"
#include "gp_pred.h"

// ------------------------------------------------------------------------------------------
extern "C" vbmc_status vbmc_sq_dist(vbmc_ctx* ctx, int D, int n, int m, const double* a, const double* b, double* C) {
  if (!ctx) return VBMC_ERR_INVALID;
  if (D <= 0 || n <= 0 || !a || !C) return set_err(ctx, VBMC_ERR_INVALID, "sq_dist: Wrong number of arguments.");
  const bool self = (b == nullptr);
  if (self) { b = a; m = n; }
  if (m <= 0) return set_err(ctx, VBMC_ERR_INVALID, "sq_dist: empty b");
  // mean used for stabilisation (sq_dist.m:26,36), computed in MATLAB's order on the host: O(D(n+m))
  std::vector<double> mu(D);
  for (int d = 0; d < D; ++d) {
    double sa = 0.0, sb = 0.0;
    for (int i = 0; i < n; ++i) sa += a[d + (size_t)D * i];
    if (self) mu[d] = sa / n;
    else {
      for (int j = 0; j < m; ++j) sb += b[d + (size_t)D * j];
      mu[d] = ((double)m / (n + m)) * (sb / m) + ((double)n / (n + m)) * (sa / n);
    }
  }
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  TmpBuf da, db, dmu, dC;
  HIP_TRY(ctx, da.alloc(ctx, (size_t)D * n * 8));
  HIP_TRY(ctx, dmu.alloc(ctx, (size_t)D * 8));
  HIP_TRY(ctx, dC.alloc(ctx, (size_t)n * m * 8));
  hipStream_t st = ctx->stream;
  HIP_TRY(ctx, hipMemcpyAsync(da.p, a, (size_t)D * n * 8, hipMemcpyHostToDevice, st));
  const double* dbp = da.as<double>();
  if (!self) {
    HIP_TRY(ctx, db.alloc(ctx, (size_t)D * m * 8));
    HIP_TRY(ctx, hipMemcpyAsync(db.p, b, (size_t)D * m * 8, hipMemcpyHostToDevice, st));
    dbp = db.as<double>();
  }
  HIP_TRY(ctx, hipMemcpyAsync(dmu.p, mu.data(), (size_t)D * 8, hipMemcpyHostToDevice, st));
  dim3 grid(((n + 15) / 16 + 3) / 4, (m + 15) / 16);
  hipLaunchKernelGGL(k_sq_dist_mfma, grid, dim3(256), 0, st, D, n, m, da.as<double>(), dbp, dmu.as<double>(), dC.as<double>());
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(C, dC.p, (size_t)n * m * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return VBMC_OK;
}

// ------------------------------------------------------------------------------------------
// gplite_post: the factorisation (gp_factor.h), gp.post(s).L of the low-noise samples, the posterior to the host and / or into a
// device-resident surrogate.  ok: gp_optimistic_then_checked's.
static vbmc_status gp_post_impl(vbmc_ctx* ctx, int N, int D, int S, int Nhyp, int meanfun, const int32_t noisefun[3],
                                const double* X, const double* y, const double* s2, const double* hyp,
                                double* alpha, double* L, double* sW, double* sn2_mult, uint8_t* Lchol,
                                vbmc_gp** gp_out, bool optimistic, bool* ok) {
  if (!ctx) return VBMC_ERR_INVALID;
  if (gp_out) *gp_out = nullptr;
  GpFactor f;
  GpFactorOpts o;
  o.who = "vbmc_gp_post"; o.fail_is_error = true; o.optimistic = optimistic;
  o.pin_out = (size_t)S * N + S;
  // Device-resident posterior, first (optimistic) try: what a vbmc_gp needs beyond the factorisation's own buffers -- the
  // per-sample constants of the log joint, sn2_eff, the column means of X, the noise multipliers -- rides in the packed upload
  // (they depend on the inputs only, the multipliers being 1 unless a retry inflates the noise), and the surrogate ADOPTS the
  // device blocks of the factorisation: no second round of uploads, no copy of the S N x N factors, one synchronisation per call.
  const bool resident = gp_out != nullptr && optimistic && D <= 32 && D > 0 && S > 0 && N > 0;
  const size_t nG = resident ? (size_t)S * GPC_STRIDE(D) : 0;
  std::vector<double> sW1(S > 0 ? S : 0), mult(S > 0 ? S : 0, 1.0);
  const GpPostExtra xl(resident ? D : 0, resident ? S : 0, nG);
  if (resident) {
    o.extra_in = xl.L.count();
    o.fill_extra = [&](double* e) {
      gp_constants(D, S, Nhyp, D + 1, noise_nhyp(noisefun), meanfun, hyp, xl.gpc.at(e));
      for (int s = 0; s < S; ++s) {
        const double w = 1.0 / std::sqrt(f.sn2min[s]);               // post.sW(1) with sn2_mult = 1  (:281)
        xl.sn2_eff.at(e)[s] = 1.0 / (w * w);                         // gplogjoint.m:160
        xl.mult.at(e)[s] = 1.0;
      }
      for (int d = 0; d < D; ++d) {
        double acc = 0.0;
        for (int n = 0; n < N; ++n) acc += X[n + (size_t)N * d];
        xl.meanX.at(e)[d] = acc / N;
      }
    };
  }
  VB_TRY(gp_factorize(ctx, N, D, S, Nhyp, meanfun, noisefun, X, y, s2, hyp, o, f));
  hipStream_t st = ctx->stream;
  const int Ncov = f.m.Ncov, Nnoise = f.m.Nnoise;
  const bool any_inv = f.any_inv;
  std::vector<double>&scal = f.scal, &sn2min = f.sn2min;
  std::vector<unsigned char>& lch = f.lch;
  TmpBuf &dA = f.w.dA, &dal = f.w.dal, &dfinv = f.w.dfinv, &dninv = f.dninv, dXi;

  double* alh = f.pin_out;   // pinned: the copy is asynchronous, one synchronisation below; the failure indices ride behind alpha
  HIP_TRY(ctx, copy_f64_small(ctx, st, alh, dal.as<double>(), (size_t)S * N + S, hipMemcpyDeviceToHost));
  f.h_pfd = alh + (size_t)S * N;
  const bool wantL = L != nullptr || gp_out != nullptr;
  // Low-noise samples (:84-99): gp.post(s).L = -inv(K + sn2 I) = -T'T with T = inv(R').  N <= 1024: the workgroup-per-slab
  // inverse of the factor and the rank-k product on the matrix cores (k_tri_inverse2 + k_syrk_tt, as in the marginal-likelihood
  // gradient), the product written NEGATED and in full over the factor it came from -- the factorisation's block then holds
  // gp.post(s).L for every sample, whichever branch it took (k_spd_inverse, 270 us at N = 400, wrote the inverse elsewhere and left the
  // sign and one copy per sample to the assembly).  alpha's solve (gp_factorize) read the factor before this point of the stream.
  const bool inv_in_place = wantL && any_inv && tri_inverse2_fits(N) && trsm2_wanted(N);
  TmpBuf dTTi;
  if (inv_in_place) {
    HIP_TRY(ctx, dTTi.alloc(ctx, (size_t)S * N * N * 8));
    HIP_TRY(ctx, tri_inverse_launch(st, N, S, dA.as<double>(), dfinv.as<double>(), dninv.as<unsigned char>(), dTTi.as<double>(), 1));
    syrk_tt_launch(st, N, S, dTTi.as<double>(), dninv.as<unsigned char>(), dA.as<double>(), true);
    HIP_TRY(ctx, hipGetLastError());
  } else if (wantL && any_inv) {
    // pL = -L\(L'\eye(N)) for low-noise samples (:98); the sign is applied where the matrix is consumed
    HIP_TRY(ctx, dXi.alloc(ctx, (size_t)S * N * N * 8));
    SPD_INVERSE_LAUNCH(ctx, N, S, st, dA.as<double>(), dfinv.as<double>(), dninv.as<unsigned char>(), dXi.as<double>());
    HIP_TRY(ctx, hipGetLastError());
  }
  if (L) {
    // the caller's copy of gp.post(s).L (D2H only when asked for)
    if (!any_inv || inv_in_place) {   // one contiguous block: every sample on the Cholesky branch, or the inverses already in their places
      VB_TRY(d2h_bounced(ctx, L, dA.as<double>(), (size_t)S * N * N * 8));
    } else {
      for (int s = 0; s < S; ++s) {
        const double* src = lch[s] ? dA.as<double>() + (size_t)s * N * N : dXi.as<double>() + (size_t)s * N * N;
        VB_TRY(d2h_bounced(ctx, L + (size_t)s * N * N, src, (size_t)N * N * 8));
      }
    }
  }
  HIP_TRY(ctx, stream_wait_latency(st, N > 1024));
  if (!(*ok = gp_factor_ok(f, S))) return VBMC_OK;     // a first try failed: once more with the noise-inflation loop
  if (L && any_inv && !inv_in_place)
    for (int s = 0; s < S; ++s)
      if (!lch[s]) for (size_t i = 0; i < (size_t)N * N; ++i) L[(size_t)s * N * N + i] = -L[(size_t)s * N * N + i];

  for (int s = 0; s < S; ++s) {
    mult[s] = scal[s * 4 + 1];
    sW1[s] = 1.0 / std::sqrt(sn2min[s] * mult[s]);  // post.sW = ones(N,1)./sqrt(min(sn2)*sn2_mult)  (:281)
  }
  if (alpha) memcpy(alpha, alh, (size_t)S * N * 8);
  if (sW) for (int s = 0; s < S; ++s) for (int n = 0; n < N; ++n) sW[(size_t)s * N + n] = sW1[s];
  if (sn2_mult) memcpy(sn2_mult, mult.data(), S * 8);
  if (Lchol) memcpy(Lchol, lch.data(), S);
  if (gp_out && resident && (!any_inv || inv_in_place)) {
    // adopt: the surrogate's device blocks ARE the factorisation's (d_lchol = the per-sample branch flags of the packed upload)
    GpGuard gp(ctx, new vbmc_gp());
    gp->N = N; gp->D = D; gp->S = S; gp->Nhyp = Nhyp; gp->Ncov = Ncov; gp->Nnoise = Nnoise; gp->meanfun = meanfun;
    gp->hyp_host.assign(hyp, hyp + (size_t)Nhyp * S);
    gp->sn2_eff.resize(S); gp->Lchol.assign(lch.begin(), lch.end());
    for (int s = 0; s < S; ++s) gp->sn2_eff[s] = 1.0 / (sW1[s] * sW1[s]);
    gp->pooled = true; gp->in_views = true; gp->hasL = true;
    gp->blk_in = f.dIn.release();
    gp->X = f.dX.as<double>(); gp->hyp = f.dhyp.as<double>(); gp->d_lchol = f.dlch.as<unsigned char>();
    double* e = f.dExtra.as<double>();
    gp->gpc = xl.gpc.at(e); gp->d_sn2 = xl.sn2_eff.at(e); gp->d_meanX = xl.meanX.at(e); gp->d_mult = xl.mult.at(e);
    gp->alpha = (double*)dal.release();
    gp->L = (double*)dA.release();
    gp->d_finv = (double*)dfinv.release();
    for (int i = 0; i < 3; ++i) gp->noisefun[i] = noisefun[i];
    gp->has_noise = true;
    *gp_out = gp.release();
  } else if (gp_out) {
    // the device-resident posterior is assembled from the device buffers (no round trip of the S N x N matrices)
    vbmc_status st2 = gp_upload_impl(ctx, N, D, S, Nhyp, Ncov, Nnoise, meanfun, X, hyp, alh, nullptr, dA.as<double>(),
                                     any_inv ? dXi.as<double>() : nullptr, sW1.data(), lch.data(), gp_out);
    if (st2 != VBMC_OK) return st2;
    st2 = vbmc_gp_set_noise(ctx, *gp_out, noisefun, mult.data());
    if (st2 != VBMC_OK) return st2;
  }
  return VBMC_OK;
}

extern "C" vbmc_status vbmc_gp_post(vbmc_ctx* ctx, int N, int D, int S, int Nhyp, int meanfun, const int32_t noisefun[3],
                                    const double* X, const double* y, const double* s2, const double* hyp,
                                    double* alpha, double* L, double* sW, double* sn2_mult, uint8_t* Lchol,
                                    vbmc_gp** gp_out) {
  return gp_optimistic_then_checked([&](bool optimistic, bool* ok) {
    return gp_post_impl(ctx, N, D, S, Nhyp, meanfun, noisefun, X, y, s2, hyp, alpha, L, sW, sn2_mult, Lchol, gp_out, optimistic, ok);
  });
}

// ------------------------------------------------------------------------------------------
// gplite_nlZ for B hyper-parameter vectors: the factorisation, the gradient leg, the closing kernel
static vbmc_status gp_nlz_impl(vbmc_ctx* ctx, int N, int D, int B, int Nhyp, int meanfun, const int32_t noisefun[3], const double* X,
                               const double* y, const double* s2, const double* hyp, int compute_grad, double* nlZ, double* dnlZ,
                               bool optimistic, bool* ok) {
  if (!ctx) return VBMC_ERR_INVALID;
  if (!nlZ || (compute_grad && !dnlZ)) return set_err(ctx, VBMC_ERR_INVALID, "vbmc_gp_nlz: null output");
  {
    // three B x N x N work matrices: keep each below 2 GiB by cutting the batch
    const size_t per = (size_t)N * N * 8;
    const int CHB = (int)std::max<size_t>(1, ((size_t)2 << 30) / std::max<size_t>(per, 1));
    if (N > 0 && B > CHB && hyp) {
      for (int b0 = 0; b0 < B; b0 += CHB) {
        const int nb = std::min(CHB, B - b0);
        vbmc_status st_ = vbmc_gp_nlz(ctx, N, D, nb, Nhyp, meanfun, noisefun, X, y, s2, hyp + (size_t)b0 * Nhyp, compute_grad, nlZ + b0,
                                      compute_grad ? dnlZ + (size_t)b0 * Nhyp : nullptr);
        if (st_ != VBMC_OK) return st_;
      }
      return VBMC_OK;
    }
  }
  GpFactor f;
  GpFactorOpts o;
  o.who = "vbmc_gp_nlz"; o.optimistic = optimistic;
  const int NnoiseH = noise_nhyp(noisefun);
  // the noise-model derivatives (host, O(B Nnoise N)) ride in the packed upload
  const size_t nds = compute_grad ? (size_t)B * std::max(NnoiseH, 1) * N : 0;
  if (compute_grad && N > 0 && B > 0 && hyp && y) {
    o.extra_in = nds;
    o.fill_extra = [&](double* e) {
      for (int b = 0; b < B; ++b)
        noise_grad(noisefun, hyp + (size_t)b * Nhyp + D + 1, N, y, s2, NnoiseH, e + (size_t)b * NnoiseH * N);
    };
  }
  const GpNlzOut ol(B > 0 ? B : 0, Nhyp, compute_grad != 0);   // the results: one block on the device, one copy back
  const size_t nout = ol.L.count();
  o.pin_out = nout;
  // few matrices of moderate order with a gradient: the factor's inverse and alpha's backward solve share one launch (gp_launch_grad);
  // otherwise, for few matrices, alpha's solve runs on the second stream beside the inverse and the streams join in front of k_nlz_grad
  const bool combined = compute_grad && N > 0 && N <= ASOLVE1_THREADS && (size_t)B * TRSM_NBLK(N) <= 1024 && tri_inverse2_fits(N);
  o.defer_alpha = combined;
  o.alpha_aside = compute_grad && B <= 16;
  VB_TRY(gp_factorize(ctx, N, D, B, Nhyp, meanfun, noisefun, X, y, s2, hyp, o, f));
  hipStream_t st = ctx->stream;
  const int Nnoise = f.m.Nnoise, Nmean = f.m.Nmean;
  TmpBuf dout, dKi, dpart, dTT;
  // the closing kernel writes the (small) block of results straight into the pinned block over the host link: no copy behind it
  const bool out_direct = copy_by_kernel(nout * 8);
  if (!out_direct) HIP_TRY(ctx, dout.alloc(ctx, nout * 8));
  double* dnlz = out_direct ? f.pin_out : dout.as<double>();
  const int nt1 = (N + NLZ_T - 1) / NLZ_T, ntile = nt1 * nt1, P = D + 1 + Nnoise;
  if (compute_grad) {
    HIP_TRY(ctx, dKi.alloc(ctx, (size_t)B * N * N * 8));
    HIP_TRY(ctx, dTT.alloc(ctx, (size_t)B * N * N * 8));
    HIP_TRY(ctx, dpart.alloc(ctx, (size_t)B * ntile * P * 8));
    VB_TRY(gp_launch_grad(ctx, st, N, D, B, Nhyp, Nnoise, f.dhyp.as<double>(), f.dscal.as<double>(), f.dones.as<unsigned char>(), f.dExtra.as<double>(),
                          f.w, dTT.as<double>(), dKi.as<double>(), dpart.as<double>(), combined, 0, f.alpha_event ? ctx->ev_join : nullptr));
  }
  gp_launch_nlz_final(st, N, D, B, Nhyp, Nnoise, Nmean, meanfun, ntile, compute_grad ? 1 : 0, f.dX.as<double>(), f.dy.as<double>(), f.dhyp.as<double>(),
                      f.w.dA.as<double>(), f.w.dal.as<double>(), f.dscal.as<double>(), compute_grad ? dpart.as<double>() : (const double*)nullptr,
                      (const double*)f.w.pfd, dnlz);
  HIP_TRY(ctx, hipGetLastError());
  if (!out_direct) HIP_TRY(ctx, hipMemcpyAsync(f.pin_out, dnlz, nout * 8, hipMemcpyDeviceToHost, st));   // pinned: asynchronous
  f.h_pfd = ol.pfd.at(f.pin_out);
  HIP_TRY(ctx, stream_wait_latency(st, N > 1024));
  if (!(*ok = gp_factor_ok(f, B))) return VBMC_OK;
  memcpy(nlZ, ol.nlZ.at(f.pin_out), ol.nlZ.size());
  if (compute_grad) memcpy(dnlZ, ol.dnlZ.at(f.pin_out), ol.dnlZ.size());
  // a matrix still not positive definite after the retries: MATLAB errors downstream and the caller maps it to NaN
  // (gplite_train.m:542-546)
  const double qnan = std::numeric_limits<double>::quiet_NaN();
  for (int b = 0; b < B; ++b)
    if (f.failed[b]) {
      nlZ[b] = qnan;
      if (compute_grad) for (int i = 0; i < Nhyp; ++i) dnlZ[(size_t)b * Nhyp + i] = qnan;
    }
  return VBMC_OK;
}

extern "C" vbmc_status vbmc_gp_nlz(vbmc_ctx* ctx, int N, int D, int B, int Nhyp, int meanfun, const int32_t noisefun[3],
                                   const double* X, const double* y, const double* s2, const double* hyp, int compute_grad,
                                   double* nlZ, double* dnlZ) {
  return gp_optimistic_then_checked([&](bool optimistic, bool* ok) {
    return gp_nlz_impl(ctx, N, D, B, Nhyp, meanfun, noisefun, X, y, s2, hyp, compute_grad, nlZ, dnlZ, optimistic, ok);
  });
}

extern "C" vbmc_status vbmc_gp_set_noise(vbmc_ctx* ctx, vbmc_gp* gp, const int32_t noisefun[3], const double* sn2_mult) {
  if (!ctx || !gp || !noisefun || !sn2_mult) return VBMC_ERR_INVALID;
  if (gp->d_mult) ctx_drain_slots(ctx);    // a pass in flight on a slot stream may be reading the multipliers about to be overwritten
  for (int i = 0; i < 3; ++i) gp->noisefun[i] = noisefun[i];
  if (!gp->d_mult) HIP_TRY(ctx, gp->pooled ? pool_get(ctx, (size_t)gp->S * 8, (void**)&gp->d_mult) : hipMalloc((void**)&gp->d_mult, (size_t)gp->S * 8));
  HIP_TRY(ctx, hipMemcpy(gp->d_mult, sn2_mult, (size_t)gp->S * 8, hipMemcpyHostToDevice));
  gp->has_noise = true;
  return VBMC_OK;
}

// ------------------------------------------------------------------------------------------
extern "C" vbmc_status vbmc_gp_pred(vbmc_ctx* ctx, const vbmc_gp* gp, int Nstar, const double* Xstar, const double* ystar,
                                    const double* s2star, int ssflag, double* ymu, double* ys2, double* fmu, double* fs2) {
  if (!ctx) return VBMC_ERR_INVALID;
  if (gp && Xstar && Nstar > pred_chunk_points(gp, Nstar)) {
    const int nc = (ssflag && gp->S > 1) ? gp->S : 1;
    return sweep_chunked(gp, Nstar, {{Xstar, nullptr, gp->D}, {ystar, nullptr, 1}, {s2star, nullptr, 1}, {nullptr, ymu, nc}, {nullptr, ys2, nc},
                                     {nullptr, fmu, nc}, {nullptr, fs2, nc}}, [&](int n, const double* const* in, double* const* out) {
      return vbmc_gp_pred(ctx, gp, n, in[0], in[1], in[2], ssflag, out[3], out[4], out[5], out[6]);
    });
  }
  PredBufs pb;
  VB_TRY(pred_on_device(ctx, "vbmc_gp_pred", gp, Nstar, Xstar, ystar, s2star, pb));
  return pred_read_columns(ctx, pb, Nstar, gp->S, ssflag, false, {ymu, ys2, fmu, fs2});
}

// reporting hook: the launch form of one prediction / quadrature call, from the functions pred_plan and pred_launch read (no launch)
extern "C" vbmc_status vbmc_pred_plan(vbmc_ctx* ctx, const vbmc_gp* gp, int Nstar, int want_ks, int quad, vbmc_pred_plan_info* out) {
  if (!ctx) return VBMC_ERR_INVALID;
  if (!out || out->struct_size != sizeof(vbmc_pred_plan_info)) return set_err(ctx, VBMC_ERR_INVALID, "vbmc_pred_plan: bad arguments");
  VB_TRY(pred_check(ctx, "vbmc_pred_plan", gp, Nstar, quad != 0));
  const bool slab = pred_needs_slab(gp->N);
  PredGroups grp = pred_row_groups(gp, slab);
  const PredForms f = pred_forms(ctx, gp->N, gp->D, gp->S, Nstar, want_ks != 0, grp.maxg);
  out->num_cu = ctx->num_cu; out->slab = f.slab_pred; out->cw = trsm_cw_for(gp->N); out->fused = f.fused; out->QS = f.QS;
  out->PT = f.fused ? f.fused_pt : 0; out->RS = f.fused_rs; out->npass = f.npass; out->units = f.units; out->grid = f.grid;
  out->PZ = (f.fused || f.slab_pred) ? 1 : f.PZ; out->maxg = f.fused ? f.fused_rs : grp.maxg; out->nblk = f.nblk;
  int rmax = 0, rmin = 0;
  for (int s = 0; s < gp->S && !slab; ++s)
    for (int g = 0; g < grp.count(s); ++g) {
      const int R = grp.edge(s, g, 1) - grp.edge(s, g, 0);
      rmax = std::max(rmax, R);
      rmin = rmin ? std::min(rmin, R) : R;
    }
  out->Rmax = rmax; out->Rmin = rmin;
  return VBMC_OK;
}

// ------------------------------------------------------------------------------------------
// gplite_quad (gplite/gplite_quad.m:1-119) with one sigma row shared by all points
namespace {
// the shared row of an Nstar x D (or 1 x D) column-major sigma; false when the rows differ
bool quad_shared_sigma(const double* sigma, int sigma_rows, int D, std::vector<double>& row) {
  row.resize(D);
  for (int d = 0; d < D; ++d) {
    row[d] = sigma[(size_t)sigma_rows * d];
    for (int i = 1; i < sigma_rows; ++i)
      if (sigma[i + (size_t)sigma_rows * d] != row[d]) return false;
  }
  return true;
}
}  // namespace

extern "C" vbmc_status vbmc_gp_quad(vbmc_ctx* ctx, const vbmc_gp* gp, int Nstar, const double* mu, const double* sigma, int sigma_rows,
                                    int ssflag, double* F, double* varF) {
  if (!ctx) return VBMC_ERR_INVALID;
  if (!gp || Nstar <= 0 || !mu || !sigma || !F || (sigma_rows != 1 && sigma_rows != Nstar))
    return set_err(ctx, VBMC_ERR_INVALID, "vbmc_gp_quad: bad arguments");
  const int D = gp->D, S = gp->S;
  std::vector<double> sg;
  if (!quad_shared_sigma(sigma, sigma_rows, D, sg))
    return set_err(ctx, VBMC_ERR_UNSUPPORTED, "vbmc_gp_quad: a sigma row per point is not accelerated (one shared row only)");
  for (int d = 0; d < D; ++d)
    if (!(sg[d] >= 0.0) || !std::isfinite(sg[d])) return set_err(ctx, VBMC_ERR_INVALID, "vbmc_gp_quad: sigma must be finite and non-negative");
  const int nc = (ssflag && S > 1) ? S : 1;
  if (Nstar > pred_chunk_points(gp, Nstar))
    return sweep_chunked(gp, Nstar, {{mu, nullptr, D}, {nullptr, F, nc}, {nullptr, varF, nc}}, [&](int n, const double* const* in, double* const* out) {
      return vbmc_gp_quad(ctx, gp, n, in[0], sg.data(), 1, ssflag, out[1], out[2]);
    });
  PredBufs pb;
  VB_TRY(pred_on_device(ctx, "vbmc_gp_quad", gp, Nstar, mu, nullptr, nullptr, pb, false, sg.data()));
  return pred_read_columns(ctx, pb, Nstar, S, ssflag, true, {nullptr, nullptr, F, varF});
}

// ------------------------------------------------------------------------------------------
// The O(N^2) pieces of the rank-1 append (gplite_post.m:210-237) for every hyper-sample:
//   Ks = k(X, x*);  Lchol: v = L' \ Ks, x = L \ v  (alpha_update = x / sn2_eff, new column = v / sn2_eff)
//                   else : x = L * Ks               (alpha_update = -x)
// The O(N) assembly of the new alpha / L / sW stays with the caller (vbmc_amd/gplite.py, the MEX shim).
namespace {
// Ks = k(X, xstar), v = L' \ Ks, x = L \ v per hyper-sample on the device (gplite_post.m:226-237); for the samples that store
// -inv(K + sn2 I) instead of a factor, x = L Ks (k_symm) and v is unused.
// up to six small device-to-device copies in one launch (the per-sample constants a surrogate inherits from the one it extends)
struct CopySegs { const double* src[6]; double* dst[6]; int n[6]; };
__global__ void k_copy_segs(CopySegs c) {
  const int g = blockIdx.x;
  for (int i = threadIdx.x; i < c.n[g]; i += blockDim.x) c.dst[g][i] = c.src[g][i];
}

vbmc_status rank1_solves_dev(vbmc_ctx* ctx, const vbmc_gp* gp, const double* xstar, TmpBuf& dKs, TmpBuf& dV, TmpBuf& dXo) {
  const int N = gp->N, D = gp->D, S = gp->S;
  if (trsm_cw_for(N) == 0) return set_err(ctx, VBMC_ERR_UNSUPPORTED, "N = %d too large", N);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  TmpBuf dxs;
  HIP_TRY(ctx, dxs.alloc(ctx, (size_t)D * 8));
  HIP_TRY(ctx, dKs.alloc(ctx, (size_t)S * N * 8));
  HIP_TRY(ctx, dV.alloc(ctx, (size_t)S * N * 8));
  HIP_TRY(ctx, dXo.alloc(ctx, (size_t)S * N * 8));
  HIP_TRY(ctx, hipMemcpyAsync(dxs.p, xstar, (size_t)D * 8, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_gp_ks, dim3(4, S), dim3(256), 0, st, N, D, gp->Nhyp, gp->X, dxs.as<double>(), gp->hyp, gp->d_meanX, dKs.as<double>());
  HIP_TRY(ctx, hipMemcpyAsync(dV.p, dKs.p, (size_t)S * N * 8, hipMemcpyDeviceToDevice, st));
  // Lchol samples: triangular solves; the others (flag 0) are skipped by the kernels and handled by k_symm
  hipLaunchKernelGGL(k_symm, dim3(8, S, 1), dim3(256), 0, st, N, 1, S, gp->L, gp->d_lchol, dKs.as<double>(), dXo.as<double>());
  HIP_TRY(ctx, trsm_fwd_launch(st, N, 1, S, 1, gp->L, gp->d_finv, gp->d_lchol, dV.as<double>()));
  HIP_TRY(ctx, trsm_bwd_launch(st, N, 1, S, 1, gp->L, gp->d_finv, gp->d_lchol, dV.as<double>(), dXo.as<double>()));
  HIP_TRY(ctx, hipGetLastError());
  return VBMC_OK;
}
}  // namespace

extern "C" vbmc_status vbmc_gp_rank1_solves(vbmc_ctx* ctx, const vbmc_gp* gp, const double* xstar, double* Ks,
                                            double* v, double* x) {
  if (!ctx) return VBMC_ERR_INVALID;
  if (!gp || !xstar || !Ks || !v || !x) return set_err(ctx, VBMC_ERR_INVALID, "vbmc_gp_rank1_solves: null argument");
  if (!gp->hasL) return set_err(ctx, VBMC_ERR_INVALID, "vbmc_gp_rank1_solves needs gp.post(s).L on the device");
  const int N = gp->N, S = gp->S;
  TmpBuf dKs, dV, dXo;
  VB_TRY(rank1_solves_dev(ctx, gp, xstar, dKs, dV, dXo));
  hipStream_t st = ctx->stream;
  HIP_TRY(ctx, hipMemcpyAsync(Ks, dKs.p, (size_t)S * N * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipMemcpyAsync(v, dV.p, (size_t)S * N * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipMemcpyAsync(x, dXo.p, (size_t)S * N * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return VBMC_OK;
}

extern "C" vbmc_status vbmc_gp_rank1_update(vbmc_ctx* ctx, const vbmc_gp* gp, const double* X_new, double ystar, const double* mstar,
                                            const double* vstar, const double* sn2_eff, double* alpha_new, double* L_new,
                                            vbmc_gp** out) {
  if (!ctx) return VBMC_ERR_INVALID;
  if (!gp || !X_new || !sn2_eff || !out || ((mstar == nullptr) != (vstar == nullptr)))
    return set_err(ctx, VBMC_ERR_INVALID, "vbmc_gp_rank1_update: null argument (mstar and vstar go together)");
  *out = nullptr;
  if (!gp->hasL) return set_err(ctx, VBMC_ERR_INVALID, "vbmc_gp_rank1_update needs gp.post(s).L on the device");
  const int N = gp->N, D = gp->D, S = gp->S, N1 = N + 1;
  if (trsm_cw_for(N1) == 0) return set_err(ctx, VBMC_ERR_UNSUPPORTED, "N = %d too large", N1);
  std::vector<double> xs(D);
  for (int d = 0; d < D; ++d) xs[d] = X_new[(size_t)N + (size_t)N1 * d];   // the appended row of the (N+1) x D matrix
  TmpBuf dKs, dV, dXo, dsc, dLn, dan;
  VB_TRY(rank1_solves_dev(ctx, gp, xs.data(), dKs, dV, dXo));
  hipStream_t st = ctx->stream;
  // per-sample scalars: sn2_eff (:207), Kss = sf2 (:213), (mstar - ystar)/vstar (:245), vstar
  std::vector<double> sc((size_t)S * 4);
  for (int s = 0; s < S; ++s) {
    sc[s * 4 + 0] = sn2_eff[s];
    sc[s * 4 + 1] = std::exp(2.0 * gp->hyp_host[(size_t)s * gp->Nhyp + D]);
    sc[s * 4 + 2] = mstar ? (mstar[s] - ystar) / vstar[s] : 0.0;
    sc[s * 4 + 3] = mstar ? vstar[s] : 0.0;
  }
  HIP_TRY(ctx, dsc.alloc(ctx, sc.size() * 8));
  HIP_TRY(ctx, hipMemcpyAsync(dsc.p, sc.data(), sc.size() * 8, hipMemcpyHostToDevice, st));
  if (!mstar) {   // the prediction at the new point from the solves at hand (no separate gplite_pred pass)
    TmpBuf dx1;
    HIP_TRY(ctx, dx1.alloc(ctx, (size_t)D * 8));
    HIP_TRY(ctx, hipMemcpyAsync(dx1.p, xs.data(), (size_t)D * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_rank1_stats, dim3(S), dim3(256), 0, st, N, D, gp->Nhyp, gp->Ncov + gp->Nnoise, gp->meanfun, gp->hyp, dx1.as<double>(),
                       gp->alpha, gp->d_lchol, dKs.as<double>(), dV.as<double>(), dXo.as<double>(), ystar, dsc.as<double>());
  }
  HIP_TRY(ctx, dLn.alloc(ctx, (size_t)S * N1 * N1 * 8));
  HIP_TRY(ctx, dan.alloc(ctx, (size_t)S * N1 * 8));
  hipLaunchKernelGGL(k_rank1_assemble, dim3(N1, S), dim3(256), 0, st, N, gp->L, gp->alpha, gp->d_lchol, dV.as<double>(), dXo.as<double>(),
                     dsc.as<double>(), dLn.as<double>(), dan.as<double>());
  HIP_TRY(ctx, hipGetLastError());
  // The new surrogate ADOPTS the assembled factors and alpha (round 5; before: alpha to the host, a second round of six pageable
  // uploads, a device-to-device copy of the S factors, two more synchronisations).  Its small blocks are windows of ONE pooled
  // block [X_new | meanX | hyp | gpc | sn2_eff | mult | lchol]: X_new and its column means come up through the pinned block, the
  // per-sample constants -- unchanged by an append -- are copied from the surrogate it extends in one launch.
  const int Nhyp = gp->Nhyp;
  const size_t nG = (size_t)S * GPC_STRIDE(D), nH = (size_t)Nhyp * S;
  const GpRank1Block bl(N1, D, S, Nhyp, nG);
  VB_TRY(ensure_pin(ctx, (bl.upload + (size_t)S * N1) * 8 + 8));
  double* hin = (double*)ctx->pin;
  bl.X.put(hin, X_new);
  for (int d = 0; d < D; ++d) {
    double acc = 0.0;
    for (int n = 0; n < N1; ++n) acc += X_new[n + (size_t)N1 * d];
    bl.meanX.at(hin)[d] = acc / N1;
  }
  double* ah = hin + bl.upload;            // alpha comes back here
  GpGuard ng(ctx, new vbmc_gp());
  ng->N = N1; ng->D = D; ng->S = S; ng->Nhyp = Nhyp; ng->Ncov = gp->Ncov; ng->Nnoise = gp->Nnoise; ng->meanfun = gp->meanfun;
  ng->hyp_host = gp->hyp_host; ng->sn2_eff = gp->sn2_eff; ng->Lchol = gp->Lchol;     // post.sW(1) is unchanged by the append (:239)
  ng->pooled = true; ng->in_views = true; ng->hasL = true;
  HIP_TRY(ctx, pool_get(ctx, bl.L.bytes(), &ng->blk_in));
  HIP_TRY(ctx, pool_get(ctx, (size_t)S * TRSM_NBLK(N1) * 256 * sizeof(double), (void**)&ng->d_finv));
  double* blk = (double*)ng->blk_in;
  bl.bind(*ng.h, blk);
  ng->L = (double*)dLn.release();
  ng->alpha = (double*)dan.release();
  HIP_TRY(ctx, copy_f64_small(ctx, st, blk, hin, bl.upload, hipMemcpyHostToDevice));
  {
    CopySegs cs{};
    cs.src[0] = gp->hyp; cs.dst[0] = ng->hyp; cs.n[0] = (int)nH;
    cs.src[1] = gp->gpc; cs.dst[1] = ng->gpc; cs.n[1] = (int)nG;
    cs.src[2] = gp->d_sn2; cs.dst[2] = ng->d_sn2; cs.n[2] = S;
    cs.src[3] = gp->has_noise ? gp->d_mult : gp->d_sn2; cs.dst[3] = ng->d_mult; cs.n[3] = S;     // (without a noise model the slot is just initialised)
    cs.src[4] = (const double*)gp->d_lchol; cs.dst[4] = (double*)ng->d_lchol; cs.n[4] = 0;
    hipLaunchKernelGGL(k_copy_segs, dim3(4), dim3(256), 0, st, cs);
    HIP_TRY(ctx, hipMemcpyAsync(ng->d_lchol, gp->d_lchol, (size_t)S, hipMemcpyDeviceToDevice, st));     // bytes: not a whole number of doubles
  }
  hipLaunchKernelGGL(k_diag_inv, dim3(TRSM_NBLK(N1), S), dim3(64), 0, st, N1, ng->L, ng->d_lchol, ng->d_finv);
  HIP_TRY(ctx, copy_f64_small(ctx, st, ah, ng->alpha, (size_t)S * N1, hipMemcpyDeviceToHost));
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, stream_wait_latency(st, N1 > 1024));
  if (gp->has_noise) {
    for (int i = 0; i < 3; ++i) ng->noisefun[i] = gp->noisefun[i];
    ng->has_noise = true;
  }
  if (alpha_new) memcpy(alpha_new, ah, (size_t)S * N1 * 8);
  if (L_new) VB_TRY(d2h_bounced(ctx, L_new, ng->L, (size_t)S * N1 * N1 * 8));
  *out = ng.release();
  return VBMC_OK;
}

// C-ABI entry points of the acquisition functions: vbmc_acq_eval, vbmc_acq_eval_delta, the importance-sampling state of the IQR
// functions (vbmc_acq_is_create, vbmc_acq_is_free) and vbmc_acq_iqr_eval (include/vbmc_hip.h).  The prediction underneath, the chunked
// sweep, the constants of k_acq and the read-back are gp_pred.h.
#include <algorithm>
#include <cmath>

#include "gp_pred.h"

// ------------------------------------------------------------------------------------------
// vbmc_acq_eval and vbmc_acq_eval_delta: delta (D values) switches the per-hyper-sample mean and variance from gplite_pred to
// gplite_quad(gp,Xs,vp.delta',1) (acqwrapper_vbmc.m:12-17); everything from fbar / vtot on is the same k_acq
namespace {
vbmc_status acq_eval_impl(vbmc_ctx* ctx, const char* who, const vbmc_gp* gp, int Nstar, const double* Xs, int acq_id, int K,
                          const double* vp_mu, const double* vp_sigma, const double* vp_lambda, const double* vp_w,
                          double ymax, int var_regularized, double TolGPVar, const double* gplengthscale,
                          const double* X_rescaled, const double* sn2new, const double* delta, double* acq, double* fbar, double* vtot) {
  if (!acq || K <= 0 || !vp_mu || !vp_sigma || !vp_lambda || !vp_w) return set_err(ctx, VBMC_ERR_INVALID, "%s: bad arguments", who);
  if (acq_id < 0 || acq_id > 3) return set_err(ctx, VBMC_ERR_UNSUPPORTED, "acquisition function id %d not accelerated (0 acqf, 1 acqflog, 2 acqus, 3 acqfsn2)", acq_id);
  if (acq_id == 3 && (!gplengthscale || !X_rescaled || !sn2new))
    return set_err(ctx, VBMC_ERR_INVALID, "%s: acqfsn2 needs gplengthscale, X_rescaled and sn2new", who);
  if (gp && Xs && Nstar > pred_chunk_points(gp, Nstar))
    return sweep_chunked(gp, Nstar, {{Xs, nullptr, gp->D}, {nullptr, acq, 1}, {nullptr, fbar, 1}, {nullptr, vtot, 1}},
                         [&](int n, const double* const* in, double* const* out) {
      return acq_eval_impl(ctx, who, gp, n, in[0], acq_id, K, vp_mu, vp_sigma, vp_lambda, vp_w, ymax, var_regularized, TolGPVar,
                           gplengthscale, X_rescaled, sn2new, delta, out[1], out[2], out[3]);
    });
  PredBufs pb;
  VB_TRY(pred_on_device(ctx, who, gp, Nstar, Xs, nullptr, nullptr, pb, false, delta));
  hipStream_t st = ctx->stream;
  AcqConsts ac;
  TmpBuf dres;
  const AcqInputs in{acq_id, K, vp_mu, vp_sigma, vp_lambda, vp_w, ymax, var_regularized, TolGPVar, gplengthscale, X_rescaled, sn2new};
  VB_TRY(ac.upload(ctx, who, gp, Nstar, in));
  HIP_TRY(ctx, dres.alloc(ctx, (size_t)3 * Nstar * 8));
  ac.a.Xs = pb.dXs.as<double>(); ac.a.fmu = pb.fmu; ac.a.fs2 = pb.fs2;
  ac.a.acq = dres.as<double>(); ac.a.fbar = ac.a.acq + Nstar; ac.a.vtot = ac.a.fbar + Nstar;
  ac.launch(st);
  return acq_read_triple(ctx, dres.as<double>(), Nstar, acq, fbar, vtot);
}
}  // namespace
extern "C" vbmc_status vbmc_acq_eval(vbmc_ctx* ctx, const vbmc_gp* gp, int Nstar, const double* Xs, int acq_id, int K,
                                     const double* vp_mu, const double* vp_sigma, const double* vp_lambda, const double* vp_w,
                                     double ymax, int var_regularized, double TolGPVar, const double* gplengthscale,
                                     const double* X_rescaled, const double* sn2new, double* acq, double* fbar, double* vtot) {
  if (!ctx) return VBMC_ERR_INVALID;
  return acq_eval_impl(ctx, "vbmc_acq_eval", gp, Nstar, Xs, acq_id, K, vp_mu, vp_sigma, vp_lambda, vp_w, ymax, var_regularized, TolGPVar,
                       gplengthscale, X_rescaled, sn2new, nullptr, acq, fbar, vtot);
}

extern "C" vbmc_status vbmc_acq_eval_delta(vbmc_ctx* ctx, const vbmc_gp* gp, int Nstar, const double* Xs, int acq_id, int K,
                                           const double* vp_mu, const double* vp_sigma, const double* vp_lambda, const double* vp_w,
                                           double ymax, int var_regularized, double TolGPVar, const double* gplengthscale,
                                           const double* X_rescaled, const double* sn2new, double* acq, double* fbar, double* vtot,
                                           const double* delta) {
  if (!ctx) return VBMC_ERR_INVALID;
  if (!gp || !delta) return set_err(ctx, VBMC_ERR_INVALID, "vbmc_acq_eval_delta: bad arguments");
  bool any = false;
  for (int d = 0; d < gp->D; ++d) {
    if (!(delta[d] >= 0.0) || !std::isfinite(delta[d])) return set_err(ctx, VBMC_ERR_INVALID, "vbmc_acq_eval_delta: delta must be finite and non-negative");
    any = any || delta[d] > 0.0;
  }
  if (!any) return set_err(ctx, VBMC_ERR_INVALID, "vbmc_acq_eval_delta: delta is all zero (acqwrapper_vbmc.m:12 takes gplite_pred then: call vbmc_acq_eval)");
  return acq_eval_impl(ctx, "vbmc_acq_eval_delta", gp, Nstar, Xs, acq_id, K, vp_mu, vp_sigma, vp_lambda, vp_w, ymax, var_regularized, TolGPVar,
                       gplengthscale, X_rescaled, sn2new, delta, acq, fbar, vtot);
}

extern "C" void vbmc_acq_is_free(vbmc_ctx* ctx, vbmc_acq_is* h) {
  if (!h) return;
  if (ctx) (void)hipSetDevice(ctx->device);
  for (double* p : {h->Xa, h->CT, h->fs2a, h->lnw})
    if (p) (void)hipFree(p);
  delete h;
}

namespace {
// The state's device blocks (Xa, CT, fs2a and, with has_lnw, lnw), empty.  The caller fills Xa (Na x D [x S]), fs2a and lnw (S x Nap rows,
// 0 / -inf in the padding) where they are, on the device, and closes with acq_is_ctmp_resident.
vbmc_status acq_is_new(vbmc_ctx* ctx, const vbmc_gp* gp, int Na, int per_sample_inputs, bool has_lnw, vbmc_acq_is** out) {
  const int N = gp->N, D = gp->D, S = gp->S;
  const int Nap = ((Na + 15) / 16) * 16;
  if (Nap > VBMC_LIM_NA) return set_err(ctx, VBMC_ERR_UNSUPPORTED, "Na = %d > %d importance points not accelerated", Na, VBMC_LIM_NA);
  if (trsm_cw_for(N) == 0) return set_err(ctx, VBMC_ERR_UNSUPPORTED, "N = %d too large", N);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  AcqIsGuard h(ctx, new vbmc_acq_is());
  h->Na = Na; h->Nap = Nap; h->per_s = per_sample_inputs ? 1 : 0; h->S = S; h->N = N; h->D = D;
  const size_t nxa = (size_t)Na * D * (per_sample_inputs ? S : 1);
  HIP_TRY(ctx, hipMalloc((void**)&h->Xa, nxa * 8));
  HIP_TRY(ctx, hipMalloc((void**)&h->CT, (size_t)S * N * Nap * 8));
  HIP_TRY(ctx, hipMalloc((void**)&h->fs2a, (size_t)S * Nap * 8));
  if (has_lnw) {
    h->has_lnw = true;
    HIP_TRY(ctx, hipMalloc((void**)&h->lnw, (size_t)S * Nap * 8));
  }
  *out = h.release();
  return VBMC_OK;
}

// Ctmp = (L\(L'\Kax'))/sn2_eff | L*Kax' (activeimportancesampling_vbmc.m:255-275) from the importance points h->Xa already on the
// device, packed into h->CT.  On failure the state stays the caller's.
vbmc_status acq_is_ctmp_resident(vbmc_ctx* ctx, const vbmc_gp* gp, vbmc_acq_is* h) {
  const int N = gp->N, D = gp->D, S = gp->S, Na = h->Na, Nap = h->Nap;
  hipStream_t st = ctx->stream;
  TmpBuf dZ, dU;
  HIP_TRY(ctx, dZ.alloc(ctx, (size_t)S * N * Na * 8));
  HIP_TRY(ctx, dU.alloc(ctx, (size_t)S * N * Na * 8));
  hipLaunchKernelGGL(k_cross_kernel, dim3(64, S), dim3(256), 0, st, N, D, gp->Nhyp, Na, h->per_s, gp->X, h->Xa, gp->hyp, dZ.as<double>());
  hipLaunchKernelGGL(k_symm, dim3(64, S, 1), dim3(256), 0, st, N, Na, S, gp->L, gp->d_lchol, dZ.as<double>(), dU.as<double>());
  HIP_TRY(ctx, trsm_fwd_launch(st, N, Na, S, 1, gp->L, gp->d_finv, gp->d_lchol, dZ.as<double>()));
  HIP_TRY(ctx, trsm_bwd_launch(st, N, Na, S, 1, gp->L, gp->d_finv, gp->d_lchol, dZ.as<double>(), dU.as<double>()));
  hipLaunchKernelGGL(k_ctmp_pack, dim3(64, S), dim3(256), 0, st, N, Na, Nap, dU.as<double>(), gp->d_sn2, gp->d_lchol, h->CT);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return VBMC_OK;
}

// A state with lnw made of device buffers in the state's own layouts (Xa: Na x D [x S]; lnw, fs2a: S x Nap rows), behind whatever wrote
// them in the context's stream.
vbmc_status acq_is_from_device(vbmc_ctx* ctx, const vbmc_gp* gp, const char* who, int Na, int per_sample_inputs, const double* Xa,
                               const double* lnw, const double* fs2a, vbmc_acq_is** out) {
  vbmc_acq_is* made = nullptr;
  VB_TRY(acq_is_new(ctx, gp, Na, per_sample_inputs, true, &made));
  AcqIsGuard h(ctx, made);
  const size_t nxa = (size_t)Na * gp->D * (per_sample_inputs ? gp->S : 1), np = (size_t)gp->S * h->Nap;
  hipError_t e1 = hipMemcpyAsync(h->Xa, Xa, nxa * 8, hipMemcpyDeviceToDevice, ctx->stream);
  hipError_t e2 = hipMemcpyAsync(h->lnw, lnw, np * 8, hipMemcpyDeviceToDevice, ctx->stream);
  hipError_t e3 = hipMemcpyAsync(h->fs2a, fs2a, np * 8, hipMemcpyDeviceToDevice, ctx->stream);
  if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) return set_err(ctx, VBMC_ERR_HIP, "%s: device copy into the state failed", who);
  VB_TRY(acq_is_ctmp_resident(ctx, gp, h.h));
  *out = h.release();
  return VBMC_OK;
}
}  // namespace

// the host-pointer entry: its uploads, then the device-resident routine (the way pred_on_device / pred_on_device_resident are split)
extern "C" vbmc_status vbmc_acq_is_create(vbmc_ctx* ctx, const vbmc_gp* gp, int Na, const double* Xa, int per_sample_inputs,
                                          const double* lnw, const double* fs2a, const double* Ctmp, vbmc_acq_is** out) {
  if (!ctx) return VBMC_ERR_INVALID;
  if (out) *out = nullptr;
  if (!gp || !out || Na <= 0 || !Xa) return set_err(ctx, VBMC_ERR_INVALID, "vbmc_acq_is_create: bad arguments");
  if (!gp->hasL) return set_err(ctx, VBMC_ERR_INVALID, "vbmc_acq_is_create needs gp.post(s).L on the device");
  if (per_sample_inputs && !fs2a)
    return set_err(ctx, VBMC_ERR_INVALID, "vbmc_acq_is_create: per-hyper-sample importance points need fs2a from the caller");
  const int N = gp->N, D = gp->D, S = gp->S;
  vbmc_acq_is* made = nullptr;
  VB_TRY(acq_is_new(ctx, gp, Na, per_sample_inputs, lnw != nullptr, &made));
  AcqIsGuard h(ctx, made);
  hipStream_t st = ctx->stream;
  const int Nap = h->Nap;
  const size_t nxa = (size_t)Na * D * (per_sample_inputs ? S : 1);
  HIP_TRY(ctx, hipMemcpyAsync(h->Xa, Xa, nxa * 8, hipMemcpyHostToDevice, st));
  // lnw (S x Na, column-major as in MATLAB) -> S x Nap rows, -inf in the padding
  std::vector<double> hb((size_t)S * Nap);
  if (lnw) {
    for (int s = 0; s < S; ++s)
      for (int a = 0; a < Nap; ++a) hb[(size_t)s * Nap + a] = a < Na ? lnw[s + (size_t)S * a] : -INFINITY;
    HIP_TRY(ctx, hipMemcpyAsync(h->lnw, hb.data(), hb.size() * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
  }
  // fs2a (Na x S): given, or gplite_pred at the (shared) importance points
  std::vector<double> f2((size_t)S * Nap, 0.0);
  if (fs2a) {
    for (int s = 0; s < S; ++s)
      for (int a = 0; a < Na; ++a) f2[(size_t)s * Nap + a] = fs2a[a + (size_t)Na * s];
  } else {
    std::vector<double> tmp((size_t)Na * S);
    VB_TRY(vbmc_gp_pred(ctx, gp, Na, Xa, nullptr, nullptr, 1, nullptr, nullptr, nullptr, tmp.data()));
    for (int s = 0; s < S; ++s)
      for (int a = 0; a < Na; ++a) f2[(size_t)s * Nap + a] = tmp[a + (size_t)Na * s];
  }
  HIP_TRY(ctx, hipMemcpyAsync(h->fs2a, f2.data(), f2.size() * 8, hipMemcpyHostToDevice, st));
  if (Ctmp) {
    // Ctmp (N x Na x S) given, already scaled: pack with unit scale (flag array of zeros -> sc = 1)
    TmpBuf dU, dzero;
    HIP_TRY(ctx, dU.alloc(ctx, (size_t)S * N * Na * 8));
    HIP_TRY(ctx, hipMemcpyAsync(dU.p, Ctmp, (size_t)S * N * Na * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, dzero.alloc(ctx, S));
    HIP_TRY(ctx, hipMemsetAsync(dzero.p, 0, S, st));
    hipLaunchKernelGGL(k_ctmp_pack, dim3(64, S), dim3(256), 0, st, N, Na, Nap, dU.as<double>(), gp->d_sn2, dzero.as<unsigned char>(), h->CT);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(st));
  } else {
    VB_TRY(acq_is_ctmp_resident(ctx, gp, h.h));   // (f2 stays alive until its copy has been waited for in there)
  }
  *out = h.release();
  return VBMC_OK;
}

extern "C" vbmc_status vbmc_acq_iqr_eval(vbmc_ctx* ctx, const vbmc_gp* gp, const vbmc_acq_is* is, int Nstar, const double* Xs,
                                         const double* gplengthscale, const double* X_rescaled, const double* sn2new,
                                         int var_regularized, double TolGPVar, double* acq, double* fbar, double* vtot) {
  if (!ctx) return VBMC_ERR_INVALID;
  if (!is || !acq || !gplengthscale || !X_rescaled || !sn2new) return set_err(ctx, VBMC_ERR_INVALID, "vbmc_acq_iqr_eval: bad arguments");
  if (gp && (is->N != gp->N || is->S != gp->S || is->D != gp->D))
    return set_err(ctx, VBMC_ERR_INVALID, "vbmc_acq_iqr_eval: importance-sampling state belongs to a different GP");
  if (gp && Xs && Nstar > pred_chunk_points(gp, Nstar))
    return sweep_chunked(gp, Nstar, {{Xs, nullptr, gp->D}, {nullptr, acq, 1}, {nullptr, fbar, 1}, {nullptr, vtot, 1}},
                         [&](int n, const double* const* in, double* const* out) {
      return vbmc_acq_iqr_eval(ctx, gp, is, n, in[0], gplengthscale, X_rescaled, sn2new, var_regularized, TolGPVar, out[1], out[2], out[3]);
    });
  PredBufs pb;
  VB_TRY(pred_on_device(ctx, "vbmc_acq_iqr_eval", gp, Nstar, Xs, nullptr, nullptr, pb, true));
  hipStream_t st = ctx->stream;
  const int N = gp->N, D = gp->D, S = gp->S;
  NnNoise nn;
  TmpBuf dsx, dacqs, dres;
  VB_TRY(nn.upload(ctx, gp, gplengthscale, X_rescaled, sn2new));
  HIP_TRY(ctx, dsx.alloc(ctx, (size_t)Nstar * 8));
  HIP_TRY(ctx, dacqs.alloc(ctx, (size_t)Nstar * S * 8));
  HIP_TRY(ctx, dres.alloc(ctx, (size_t)3 * Nstar * 8));
  nn.launch(st, Nstar, pb.dXs.as<double>(), dsx.as<double>());
  IqrArgs a{};
  a.N = N; a.D = D; a.S = S; a.Nhyp = gp->Nhyp; a.Nstar = Nstar; a.Na = is->Na; a.Nap = is->Nap; a.per_s = is->per_s;
  a.Xs = pb.dXs.as<double>(); a.Xa = is->Xa; a.hyp = gp->hyp; a.Xc = pb.dXc.as<double>(); a.muv = pb.dmuv.as<double>();
  a.CT = is->CT; a.fs2a = is->fs2a; a.lnw = is->has_lnw ? is->lnw : nullptr; a.fs2 = pb.fs2; a.sn2x = dsx.as<double>();
  a.lchol = gp->d_lchol; a.acqs = dacqs.as<double>(); a.KsW = pb.dKs.as<double>(); a.sn2_eff = gp->d_sn2;
  dim3 grid((Nstar + IQR_PTS - 1) / IQR_PTS, S);
  switch (is->Nap / 16) {
#define IQR_CASE(NT)                                                                                                                   \
  case NT:                                                                                                                             \
    if (IQR_LDS_BYTES(NT) > 64 * 1024)                                                                                                 \
      HIP_TRY(ctx, hipFuncSetAttribute((const void*)k_acq_iqr<NT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)IQR_LDS_BYTES(NT))); \
    hipLaunchKernelGGL((k_acq_iqr<NT>), grid, dim3(IQR_THREADS), IQR_LDS_BYTES(NT), st, a);                                                     \
    break;
    IQR_CASE(1) IQR_CASE(2) IQR_CASE(3) IQR_CASE(4) IQR_CASE(5) IQR_CASE(6) IQR_CASE(7) IQR_CASE(8)
    IQR_CASE(9) IQR_CASE(10) IQR_CASE(11) IQR_CASE(12) IQR_CASE(13) IQR_CASE(14) IQR_CASE(15) IQR_CASE(16)
#undef IQR_CASE
    default: return set_err(ctx, VBMC_ERR_UNSUPPORTED, "Na = %d not accelerated", is->Na);
  }
  double* r = dres.as<double>();
  hipLaunchKernelGGL(k_iqr_final, dim3((Nstar + 255) / 256), dim3(256), 0, st, Nstar, S, var_regularized ? 1 : 0, TolGPVar,
                     dacqs.as<double>(), pb.fmu, pb.fs2, r, r + Nstar, r + 2 * (size_t)Nstar);
  return acq_read_triple(ctx, r, Nstar, acq, fbar, vtot);
}

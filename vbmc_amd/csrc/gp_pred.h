// Host side of the GP prediction (gplite_pred, gplite_quad) with its results left on the device, and what rides on it: the chunked
// sweep over many points, the read-backs, the constants of the acquisition functions and the importance-sampling state.  Shared by
// vbmc_gp_pred / vbmc_gp_quad (abi_gp.hip), the acquisition entry points (abi_acq.hip), the acquisition search
// (abi_acq_search.hip), the ensemble sampler's core (is_core.h) and the surrogate sampler (abi_gp_surrogate.hip).
#pragma once
#include <algorithm>
#include <cmath>

#include "elbo_pass.h"   // ensure_tinv
#include "gp_acq_kernels.h"
#include "gp_factor.h"   // HandleGuard
#include "gp_pred_kernels.h"

// D -> QS = ceil(D / 4) steps of the MFMA distance blocks, the way DISPATCH_GPDT (gp_factor_kernels.h) pads D; nothing runs for D > 32
#define DISPATCH_QS_CASE(QSV, ...) case QSV: { constexpr int QS = QSV; __VA_ARGS__; } break;
#define DISPATCH_QS(D_, ...)                                                                                          \
  switch (((D_) + 3) / 4) {                                                                                           \
    DISPATCH_QS_CASE(1, __VA_ARGS__) DISPATCH_QS_CASE(2, __VA_ARGS__) DISPATCH_QS_CASE(3, __VA_ARGS__)                \
    DISPATCH_QS_CASE(4, __VA_ARGS__) DISPATCH_QS_CASE(5, __VA_ARGS__) DISPATCH_QS_CASE(6, __VA_ARGS__)                \
    DISPATCH_QS_CASE(7, __VA_ARGS__) DISPATCH_QS_CASE(8, __VA_ARGS__)                                                 \
    default: break;                                                                                                   \
  }

// Importance-sampling state of the IQR acquisition functions (optimState.ActiveImportanceSampling); abi_acq.hip makes and frees it
struct vbmc_acq_is {
  int Na = 0, Nap = 0, per_s = 0, S = 0, N = 0, D = 0;
  bool has_lnw = false;
  double *Xa = nullptr, *CT = nullptr, *fs2a = nullptr, *lnw = nullptr;
};

namespace {
using AcqIsGuard = HandleGuard<vbmc_acq_is, vbmc_acq_is_free>;
// A state with lnw made of device buffers in the state's own layouts (Xa: Na x D [x S]; lnw, fs2a: S x Nap rows), behind whatever wrote
// them in the context's stream (abi_acq.hip).
vbmc_status acq_is_from_device(vbmc_ctx* ctx, const vbmc_gp* gp, const char* who, int Na, int per_sample_inputs, const double* Xa,
                               const double* lnw, const double* fs2a, vbmc_acq_is** out);

// ------------------------------------------------------------------------------------------
// the prediction
// ------------------------------------------------------------------------------------------
struct PredBufs {
  TmpBuf dXs, ds2, dys, dmb, dout, dXc, daa, dmuv, dgrp, dpV, dpF, dKs, dqs, dqn;
  double *fmu = nullptr, *fs2 = nullptr, *ys2 = nullptr;   // Nstar x S each, inside dout
};

// gplite_pred for every hyper-sample, results left on the device (shared by vbmc_gp_pred and vbmc_acq_eval)
// want_ks: the caller reads the sW-scaled cross-kernel matrix itself (the IQR acquisition functions); otherwise the variance comes from
// k_pred_fused and that matrix is never written.  VBMC_PRED_FUSED=0 keeps the two-kernel form (A/B runs, tests).
// qsigma (D values, host): the Bayesian-quadrature form instead (gplite_quad.m) -- Xstar holds the means mu_i, pb.fmu / pb.fs2 receive
// F / varF per hyper-sample through the k_quad_* forms of the same kernels, in the same launch forms (fused, two-kernel, slab).
//
// Three layers.  pred_on_device takes host pointers, computes the points' column means and uploads both.  pred_on_device_resident takes
// the points (pb.dXs, Nstar x D) and their column means (pb.dmb) where they already are, on the device; it is pred_plan -- every
// allocation, every choice of a launch form, the one upload of the row-group table -- followed by pred_launch, which only enqueues
// kernels and which a caller whose points change in place (vbmc_acq_search) repeats.
struct PredForms {
  bool slab_pred = false, fused = false;
  int PZ = 1, fused_pt = 0, fused_rs = 1;
  // the grid arithmetic: what pred_launch launches with and what the reporting hook vbmc_pred_plan reports
  int QS = 0, ntile = 0;       // ceil(D / 4) steps of the MFMA distance blocks; 16-point tiles
  int nblk = 0;                // 16-row tiles of the training set
  int npass = 0, units = 0;    // fused: passes of fused_pt tiles over the points, and the (hyper-sample, pass) units
  int slab_cw = 0;             // slab: test points per wave of k_pred_slab (trsm_cw_for)
  int grid = 0;                // workgroups of the variance kernel: k_pred_fused's x and k_pred_slab's x * y, which pred_launch reads;
                               // for k_gp_pred the product of the dim3(maxg, S, PZ) it launches
};
struct PredPlan {
  PredArgs pa{};
  PredForms f;
  bool quad = false;
  int Nstar = 0, Np = 0, maxg = 0;
  size_t maxlds = 0;
};

vbmc_status pred_check(vbmc_ctx* ctx, const char* who, const vbmc_gp* gp, int Nstar, bool quad) {
  if (!gp || Nstar <= 0) return set_err(ctx, VBMC_ERR_INVALID, "%s: bad arguments", who);
  if (!gp->hasL) return set_err(ctx, VBMC_ERR_INVALID, "%s needs gp.post(s).L on the device", who);
  if (!gp->has_noise) return set_err(ctx, VBMC_ERR_INVALID, "%s: call vbmc_gp_set_noise (noisefun, sn2_mult) first", who);
  if (gp->D > VBMC_LIM_D) return set_err(ctx, VBMC_ERR_UNSUPPORTED, "D = %d > %d not accelerated", gp->D, VBMC_LIM_D);
  if (quad && gp->meanfun != 0 && gp->meanfun != 1 && gp->meanfun != 4)
    return set_err(ctx, VBMC_ERR_UNSUPPORTED, "%s: mean function %d not accelerated (0, 1, 4)", who, gp->meanfun);
  // gplite_quad.m:66-67,101 divides by the scalar sn2_eff = exp(2 hyp(Ncov+1)) sn2_mult: the constant-noise model, whose sW is that scalar
  if (quad && !(gp->noisefun[0] == 1 && gp->noisefun[1] == 0 && gp->noisefun[2] == 0))
    return set_err(ctx, VBMC_ERR_UNSUPPORTED, "%s: only the constant noise model (noisefun [1 0 0]) is accelerated", who);
  if (trsm_cw_for(gp->N) == 0) return set_err(ctx, VBMC_ERR_UNSUPPORTED, "N = %d too large for the prediction kernels", gp->N);
  return VBMC_OK;
}

// the box of the searches and samplers that run in one: coordinates d0 .. d1 - 1 (host arrays)
vbmc_status check_box(vbmc_ctx* ctx, const char* who, const double* LB, const double* UB, int d0, int d1) {
  for (int d = d0; d < d1; ++d)
    if (!std::isfinite(LB[d]) || !std::isfinite(UB[d]) || !(LB[d] < UB[d]))
      return set_err(ctx, VBMC_ERR_INVALID, "%s: the box needs finite bounds with LB < UB (coordinate %d: [%g, %g])", who, d + 1, LB[d], UB[d]);
  return VBMC_OK;
}

// The kernels' arguments from the surrogate and the buffers of the call (all allocated by now).
// output-dependent noise (noisefun(3) = 1) enters ys2 only, and only with a non-empty ystar (gplite_noisefun.m:198-207);
// fmu / fs2 -- all the acquisition functions read (acqwrapper_vbmc.m:17) -- never depend on it
// an empty s2star counts as zero (gplite_noisefun.m:51): the kernels add nothing when the pointer is null
PredArgs pred_pack_args(const vbmc_gp* gp, int Nstar, PredBufs& pb, bool quad) {
  const int S = gp->S;
  PredArgs pa{};
  pa.N = gp->N; pa.D = gp->D; pa.S = S; pa.Nhyp = gp->Nhyp; pa.Nstar = Nstar; pa.mc = Nstar; pa.meanfun = gp->meanfun;
  pa.moff = gp->Ncov + gp->Nnoise; pa.noff = gp->Ncov; pa.nf0 = gp->noisefun[0]; pa.nf1 = gp->noisefun[1]; pa.nf2 = gp->noisefun[2];
  pa.X = gp->X; pa.Xs = pb.dXs.as<double>(); pa.s2s = pb.ds2.p ? pb.ds2.as<double>() : nullptr; pa.hyp = gp->hyp;
  pa.ys = pb.dys.p ? pb.dys.as<double>() : nullptr;
  pa.alpha = gp->alpha; pa.L = gp->L; pa.sn2_eff = gp->d_sn2; pa.sn2_mult = gp->d_mult; pa.lchol = gp->d_lchol;
  pa.mean_a = gp->d_meanX; pa.mean_b = pb.dmb.as<double>(); pa.finv = gp->d_finv; pa.tinv = gp->d_tinv;
  pa.fmu = pb.dout.as<double>(); pa.fs2 = pa.fmu + (size_t)Nstar * S; pa.ys2 = pa.fs2 + (size_t)Nstar * S;
  pb.fmu = pa.fmu; pb.fs2 = pa.fs2; pb.ys2 = pa.ys2;
  if (quad) { pa.qsig = pb.dqs.as<double>(); pa.qnf = pb.dqn.as<double>(); }
  return pa;
}

// inv(L') stays resident while the solves run 16 columns wide (trsm_cw_for: N <= 1136; the prediction's own 16-row tile would fit the LDS
// up to N = 1248): beyond that the variance comes from slab solves (k_pred_slab)
bool pred_needs_slab(int N) {
  const int Np = ((N + 15) >> 4) << 4;
  return (size_t)16 * Np * 8 > PRED_LDS_MAX || (Np >> 4) > PRED_MAXG || trsm_cw_for(N) != 16;
}

// The row-group table the kernels read: [count S | t0 S x PRED_MAXG | t1 S x PRED_MAXG].  Resident row blocks of Tinv per hyper-sample:
// consecutive 16-row tiles, balanced by area (tile b costs b + 1), bounded by PRED_MAXR tiles and PRED_LDS_MAX bytes of LDS (two
// workgroups per CU).
struct PredGroups {
  int S;
  std::vector<int> tab;
  int maxg = 0;
  size_t maxlds = 0;
  explicit PredGroups(int S_) : S(S_), tab((size_t)S_ + 2 * (size_t)S_ * PRED_MAXG, 0) {}
  int& count(int s) { return tab[s]; }
  int& edge(int s, int g, int end) { return tab[(size_t)S + ((size_t)end * S + s) * PRED_MAXG + g]; }   // end 0: t0, 1: t1
  void add(int s, int t0, int t1, size_t lds) { const int g = count(s)++; edge(s, g, 0) = t0; edge(s, g, 1) = t1; maxlds = std::max(maxlds, lds); }
};
PredGroups pred_row_groups(const vbmc_gp* gp, bool slab_pred) {
  const int N = gp->N, S = gp->S;
  const int Np = ((N + 15) >> 4) << 4, nblk = Np >> 4;
  PredGroups g(S);
  for (int s = 0; s < S; ++s) {
    if (slab_pred) {
      g.count(s) = 1;                          // k_pred_slab writes block partial 0
    } else if (gp->Lchol[s]) {
      int t0 = 0;
      for (int b = 0; b < nblk; ++b) {
        const int R = b - t0 + 1;
        const size_t lds_need = (size_t)R * 16 * (size_t)(b + 1) * 16 * 8;
        if (b > t0 && (R > PRED_MAXR || lds_need > PRED_LDS_MAX)) {
          g.add(s, t0, b, (size_t)(b - t0) * 16 * (size_t)b * 16 * 8);
          t0 = b;
        }
      }
      g.add(s, t0, nblk, (size_t)(nblk - t0) * 16 * (size_t)nblk * 16 * 8);
    } else {
      for (int b = 0; b < nblk; ++b) g.add(s, b, b + 1, (size_t)16 * Np * 8);
    }
    g.maxg = std::max(g.maxg, g.count(s));
  }
  return g;
}

// Every choice of a launch form, once: maxg is the row-group table's (before the fused form replaces it by fused_rs)
PredForms pred_forms(const vbmc_ctx* ctx, int N, int D, int S, int Nstar, bool want_ks, int maxg) {
  PredForms f;
  const int Np = ((N + 15) >> 4) << 4, nblk = Np >> 4;
  f.slab_pred = pred_needs_slab(N);
  // one workgroup per CU (its LDS is full): slice the point tiles over gridDim.z until the chip is covered
  const int ntile_ = (Nstar + 15) / 16;
  f.QS = (D + 3) / 4; f.ntile = ntile_; f.nblk = nblk;
  f.PZ = std::max(1, ctx->num_cu / std::max(1, maxg * S));
  f.PZ = std::min(f.PZ, std::max(1, ntile_ / (PRED_THREADS / 64)));
  static const bool fused_off = [] { const char* e = getenv("VBMC_PRED_FUSED"); return e && !strcmp(e, "0"); }();
  // point tiles resident per workgroup: as many N x 16 tiles as the 160 KB hold beside the 2 KB table (three at N = 400)
  f.fused_pt = (int)std::min<size_t>(PREDF_PT_FOR_QS(f.QS), ((size_t)160 * 1024 - 2048 - (PREDF_THREADS / 64) * PREDF_MAXPT * 16 * 8 - 256) / ((size_t)Np * 16 * 8));
  f.fused = !want_ks && !f.slab_pred && !fused_off && f.fused_pt >= 1 && f.QS <= 8;
  // few points (the importance sampler's ~110 per call): RS workgroups per (hyper-sample, pass) unit share its row tiles (k_pred_fused)
  if (f.fused) {
    f.npass = (ntile_ + f.fused_pt - 1) / f.fused_pt;
    f.units = f.npass * S;
    f.fused_rs = std::max(1, std::min(std::min(4, nblk / 4), ctx->num_cu / std::max(1, f.units)));
    // one workgroup per compute unit (its LDS is full), each walking the (hyper-sample, pass, row share) units b, b + grid, ...
    f.grid = std::max(1, std::min(f.units * f.fused_rs, ctx->num_cu));
  } else if (f.slab_pred) {
    f.slab_cw = std::max(1, trsm_cw_for(N));
    f.grid = ((Nstar + f.slab_cw - 1) / f.slab_cw) * S;
  } else {
    f.grid = maxg * S * f.PZ;
  }
  return f;
}

// pb.dXs, pb.dmb (and pb.ds2 / pb.dys where the caller has them) are allocated; their contents are read by pred_launch only
vbmc_status pred_plan(vbmc_ctx* ctx, const vbmc_gp* gp, int Nstar, PredBufs& pb, bool want_ks, const double* qsigma, PredPlan& pl) {
  const int N = gp->N, D = gp->D, S = gp->S;
  const bool quad = qsigma != nullptr;
  const bool slab_pred = pred_needs_slab(N);
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  if (!slab_pred) {   // Tinv = inv(L') = L' \ I for the Lchol samples, once per GP (the kernels skip the others)
    bool have = false;
    VB_TRY(ensure_tinv(ctx, gp, &have));
  }
  HIP_TRY(ctx, pb.dXc.alloc(ctx, (size_t)S * N * D * 8));
  HIP_TRY(ctx, pb.daa.alloc(ctx, (size_t)S * N * 8));
  HIP_TRY(ctx, pb.dmuv.alloc(ctx, (size_t)S * 2 * D * 8));
  HIP_TRY(ctx, pb.dout.alloc(ctx, (size_t)3 * Nstar * S * 8));
  if (quad) {
    HIP_TRY(ctx, pb.dqs.alloc(ctx, (size_t)D * 8));
    HIP_TRY(ctx, pb.dqn.alloc(ctx, (size_t)S * 2 * 8));
    HIP_TRY(ctx, hipMemcpyAsync(pb.dqs.p, qsigma, (size_t)D * 8, hipMemcpyHostToDevice, st));
  }
  pl.pa = pred_pack_args(gp, Nstar, pb, quad);
  PredGroups grp = pred_row_groups(gp, slab_pred);
  pl.f = pred_forms(ctx, N, D, S, Nstar, want_ks, grp.maxg);
  if (pl.f.fused) {
    for (int s = 0; s < S; ++s) grp.count(s) = pl.f.fused_rs;      // k_pred_final: fused_rs blocks of partial sums per hyper-sample
    grp.maxg = pl.f.fused_rs;
  }
  HIP_TRY(ctx, pb.dgrp.alloc(ctx, grp.tab.size() * sizeof(int)));
  HIP_TRY(ctx, pb.dpV.alloc(ctx, (size_t)grp.maxg * S * Nstar * 8));
  HIP_TRY(ctx, pb.dpF.alloc(ctx, (size_t)S * Nstar * 8));
  HIP_TRY(ctx, hipMemcpyAsync(pb.dgrp.p, grp.tab.data(), grp.tab.size() * sizeof(int), hipMemcpyHostToDevice, st));
  if (!pl.f.fused) HIP_TRY(ctx, pb.dKs.alloc(ctx, (size_t)S * N * (((size_t)Nstar + 15) / 16) * 16 * 8));   // tiled by 16 points
  pl.quad = quad; pl.Nstar = Nstar; pl.Np = ((N + 15) >> 4) << 4; pl.maxg = grp.maxg; pl.maxlds = grp.maxlds;
  return VBMC_OK;
}

// the fused form at PT point tiles per workgroup (no instantiation beyond the tiles a QS has registers for)
template <int QS, int PT>
vbmc_status pred_launch_fused(vbmc_ctx* ctx, PredBufs& pb, const PredPlan& pl, int gxf, size_t fl) {
  if constexpr (PT <= PREDF_PT_FOR_QS(QS)) {
    auto kern = pl.quad ? k_quad_fused<QS, PT> : k_pred_fused<QS, PT>;
    if (fl > 64 * 1024) HIP_TRY(ctx, hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fl));
    hipLaunchKernelGGL(kern, dim3(gxf), dim3(PREDF_THREADS), fl, ctx->stream, pl.pa, pb.dXc.as<double>(), pb.daa.as<double>(), pb.dmuv.as<double>(),
                       pb.dpV.as<double>(), pb.dpF.as<double>(), pl.f.fused_rs);
  }
  return VBMC_OK;
}
template <int QS>
vbmc_status pred_launch_fused_pt(vbmc_ctx* ctx, PredBufs& pb, const PredPlan& pl, int gxf, size_t fl) {
  const int pt = pl.f.fused_pt;
  return pt >= 3 ? pred_launch_fused<QS, 3>(ctx, pb, pl, gxf, fl) : pt == 2 ? pred_launch_fused<QS, 2>(ctx, pb, pl, gxf, fl) : pred_launch_fused<QS, 1>(ctx, pb, pl, gxf, fl);
}

vbmc_status pred_launch(vbmc_ctx* ctx, PredBufs& pb, const PredPlan& pl) {
  const PredArgs& pa = pl.pa;
  const int N = pa.N, D = pa.D, S = pa.S, Nstar = pl.Nstar, Np = pl.Np, maxg = pl.maxg, fused_pt = pl.f.fused_pt;
  const bool quad = pl.quad;
  const size_t maxlds = pl.maxlds;
  hipStream_t st = ctx->stream;
  TmpBuf &dXc = pb.dXc, &daa = pb.daa, &dmuv = pb.dmuv;
  if (quad) hipLaunchKernelGGL(k_quad_prep, dim3(4, S), dim3(256), 0, st, pa, dXc.as<double>(), daa.as<double>(), dmuv.as<double>());
  else hipLaunchKernelGGL(k_pred_prep, dim3(4, S), dim3(256), 0, st, pa, dXc.as<double>(), daa.as<double>(), dmuv.as<double>());
  auto launch_final = [&] {
    if (quad) hipLaunchKernelGGL(k_quad_final, dim3((Nstar + 255) / 256, S), dim3(256), 0, st, pa, pb.dgrp.as<int>(), pb.dpV.as<double>(), pb.dpF.as<double>());
    else hipLaunchKernelGGL(k_pred_final, dim3((Nstar + 255) / 256, S), dim3(256), 0, st, pa, pb.dgrp.as<int>(), pb.dpV.as<double>(), pb.dpF.as<double>());
  };
  if (pl.f.fused) {
    const size_t fl = PREDF_LDS_BYTES(fused_pt, Np);   // the tiles, and no less than the per-wave sums that reuse the block
    const int gxf = pl.f.grid;
    vbmc_status fs = VBMC_OK;
    DISPATCH_QS(D, fs = pred_launch_fused_pt<QS>(ctx, pb, pl, gxf, fl))
    VB_TRY(fs);
    launch_final();
    HIP_TRY(ctx, hipGetLastError());
    return VBMC_OK;
  }
  // inner dimension of the MFMA distance blocks: QS = ceil(D / 4) steps
  DISPATCH_QS(D, hipLaunchKernelGGL((quad ? k_quad_ks<QS> : k_pred_ks<QS>), dim3(pl.f.ntile, S), dim3(64), 0, st, pa, dXc.as<double>(),
                                    daa.as<double>(), dmuv.as<double>(), pb.dKs.as<double>(), pb.dpF.as<double>()))
  if (pl.f.slab_pred) {
    TRSM_DISPATCH_CW(pl.f.slab_cw, {
      const size_t sl = TRSM_LDS_BYTES_CW(N, CW);
      if (sl > 64 * 1024)
        HIP_TRY(ctx, hipFuncSetAttribute((const void*)k_pred_slab<CW>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sl));
      hipLaunchKernelGGL((k_pred_slab<CW>), dim3(pl.f.grid / S, S), dim3(64), sl, st, pa, pb.dKs.as<double>(), pb.dpV.as<double>());
    });
  } else {
    if (maxlds > 64 * 1024)
      HIP_TRY(ctx, hipFuncSetAttribute((const void*)k_gp_pred, hipFuncAttributeMaxDynamicSharedMemorySize, (int)maxlds));
    hipLaunchKernelGGL(k_gp_pred, dim3(maxg, S, pl.f.PZ), dim3(PRED_THREADS), maxlds, st, pa, pb.dKs.as<double>(), pb.dgrp.as<int>(), pb.dpV.as<double>());
  }
  launch_final();
  HIP_TRY(ctx, hipGetLastError());
  return VBMC_OK;
}

vbmc_status pred_on_device_resident(vbmc_ctx* ctx, const char* who, const vbmc_gp* gp, int Nstar, PredBufs& pb, bool want_ks = false,
                                    const double* qsigma = nullptr) {
  VB_TRY(pred_check(ctx, who, gp, Nstar, qsigma != nullptr));
  if (!pb.dXs.p || !pb.dmb.p) return set_err(ctx, VBMC_ERR_INVALID, "%s: the points and their column means are not on the device", who);
  PredPlan pl;
  VB_TRY(pred_plan(ctx, gp, Nstar, pb, want_ks, qsigma, pl));
  return pred_launch(ctx, pb, pl);
}

vbmc_status pred_on_device(vbmc_ctx* ctx, const char* who, const vbmc_gp* gp, int Nstar, const double* Xstar, const double* ystar,
                           const double* s2star, PredBufs& pb, bool want_ks = false, const double* qsigma = nullptr) {
  if (!Xstar) return set_err(ctx, VBMC_ERR_INVALID, "%s: bad arguments", who);
  VB_TRY(pred_check(ctx, who, gp, Nstar, qsigma != nullptr));
  const int D = gp->D;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  // column means for sq_dist's centring (sq_dist.m:36), O((N + Nstar) D) on the host in MATLAB's order
  std::vector<double> mb(D);
  for (int d = 0; d < D; ++d) {
    double sb = 0.0;
    for (int j = 0; j < Nstar; ++j) sb += Xstar[j + (size_t)Nstar * d];
    mb[d] = sb / Nstar;
  }
  HIP_TRY(ctx, pb.dXs.alloc(ctx, (size_t)Nstar * D * 8));
  HIP_TRY(ctx, pb.dmb.alloc(ctx, (size_t)D * 8));
  HIP_TRY(ctx, hipMemcpyAsync(pb.dXs.p, Xstar, (size_t)Nstar * D * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(pb.dmb.p, mb.data(), (size_t)D * 8, hipMemcpyHostToDevice, st));
  if (s2star) {
    HIP_TRY(ctx, pb.ds2.alloc(ctx, (size_t)Nstar * 8));
    HIP_TRY(ctx, hipMemcpyAsync(pb.ds2.p, s2star, (size_t)Nstar * 8, hipMemcpyHostToDevice, st));
  }
  if (ystar && gp->noisefun[2] == 1) {
    HIP_TRY(ctx, pb.dys.alloc(ctx, (size_t)Nstar * 8));
    HIP_TRY(ctx, hipMemcpyAsync(pb.dys.p, ystar, (size_t)Nstar * 8, hipMemcpyHostToDevice, st));
  }
  return pred_on_device_resident(ctx, who, gp, Nstar, pb, want_ks, qsigma);
}

// ------------------------------------------------------------------------------------------
// the sweep over many points
// ------------------------------------------------------------------------------------------
// The prediction pipeline materialises S x N x Nstar cross-kernel values; very large sweeps are cut into chunks of
// test points whose matrix stays below 1 GiB (the sq_dist centring constant then differs per chunk: rounding only).
int pred_chunk_points(const vbmc_gp* gp, int Nstar) {
  if (!gp) return Nstar;
  const size_t per_point = (size_t)gp->S * gp->N * 8;
  const size_t cap = ((size_t)1 << 30) / std::max<size_t>(per_point, 1);
  const size_t ch = std::max<size_t>(256, (cap / 16) * 16);
  return (size_t)Nstar <= ch ? Nstar : (int)ch;
}
// The sweep over Nstar points in chunks of pred_chunk_points.  in / out: the per-point arrays, column-major Nstar x C each (a null one
// stays null).  one(n, in, out) is the entry point itself on n points: rows [i0, i0 + n) of every input, contiguous n x C, and n x C
// of zeros for every output, which go back into rows [i0, i0 + n).
struct SweepCols { const double* in; double* out; int C; };
template <class One>
vbmc_status sweep_chunked(const vbmc_gp* gp, int Nstar, std::vector<SweepCols> cols, One one) {
  const int CH = pred_chunk_points(gp, Nstar);
  std::vector<std::vector<double>> buf(cols.size());
  std::vector<const double*> in(cols.size(), nullptr);
  std::vector<double*> out(cols.size(), nullptr);
  for (int i0 = 0; i0 < Nstar; i0 += CH) {
    const int n = std::min(CH, Nstar - i0);
    for (size_t k = 0; k < cols.size(); ++k) {
      if (!cols[k].in && !cols[k].out) continue;
      buf[k].assign((size_t)n * cols[k].C, 0.0);
      if (cols[k].in) in[k] = buf[k].data();
      else out[k] = buf[k].data();
      for (int c = 0; cols[k].in && c < cols[k].C; ++c) memcpy(buf[k].data() + (size_t)c * n, cols[k].in + (size_t)c * Nstar + i0, (size_t)n * 8);
    }
    VB_TRY(one(n, in.data(), out.data()));
    for (size_t k = 0; k < cols.size(); ++k)
      for (int c = 0; cols[k].out && c < cols[k].C; ++c) memcpy(cols[k].out + (size_t)c * Nstar + i0, buf[k].data() + (size_t)c * n, (size_t)n * 8);
  }
  return VBMC_OK;
}

// ------------------------------------------------------------------------------------------
// read-backs
// ------------------------------------------------------------------------------------------
// The columns of a prediction (quad: of a quadrature, whose F / varF are fmu / fs2; it has no ymu / ys2) into the caller's arrays, a
// null one skipped: Nstar x S per hyper-sample (ssflag, or one hyper-sample), or Nstar averaged over them by k_pred_avg into
// [ymu | ys2 | fmu | fs2] (gplite_pred.m:117-126, gplite_quad.m:112-119; the quadrature's ys2 input repeats fs2 and its first two
// columns are not read).  Synchronises the stream.
struct PredColumns { double *ymu, *ys2, *fmu, *fs2; };
vbmc_status pred_read_columns(vbmc_ctx* ctx, PredBufs& pb, int Nstar, int S, int ssflag, bool quad, const PredColumns& o) {
  hipStream_t st = ctx->stream;
  const size_t ns = (size_t)Nstar * S;
  if (S > 1 && !ssflag) {
    TmpBuf davg;
    HIP_TRY(ctx, davg.alloc(ctx, (size_t)4 * Nstar * 8));
    hipLaunchKernelGGL(k_pred_avg, dim3((Nstar + 255) / 256), dim3(256), 0, st, Nstar, S, pb.fmu, pb.fs2, quad ? pb.fs2 : pb.ys2, davg.as<double>());
    HIP_TRY(ctx, hipGetLastError());
    const int c0 = quad ? 2 : 0;
    double* const dst[4] = {o.ymu, o.ys2, o.fmu, o.fs2};
    std::vector<double> h((size_t)(4 - c0) * Nstar);
    HIP_TRY(ctx, hipMemcpyAsync(h.data(), davg.as<double>() + (size_t)c0 * Nstar, h.size() * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    for (int c = c0; c < 4; ++c)
      if (dst[c]) memcpy(dst[c], h.data() + (size_t)(c - c0) * Nstar, (size_t)Nstar * 8);
  } else {
    std::vector<double> h((quad ? 2 : 3) * ns);
    HIP_TRY(ctx, hipMemcpyAsync(h.data(), pb.dout.p, h.size() * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (o.fmu) memcpy(o.fmu, h.data(), ns * 8);
    if (o.ymu) memcpy(o.ymu, h.data(), ns * 8);
    if (o.fs2) memcpy(o.fs2, h.data() + ns, ns * 8);
    if (o.ys2 && !quad) memcpy(o.ys2, h.data() + 2 * ns, ns * 8);
  }
  return VBMC_OK;
}

// [acq | fbar | vtot], Nstar each, of an acquisition sweep (dres, on the device) into the caller's arrays; closes the call: the
// launches' errors, the copy, the synchronisation
vbmc_status acq_read_triple(vbmc_ctx* ctx, const double* dres, int Nstar, double* acq, double* fbar, double* vtot) {
  HIP_TRY(ctx, hipGetLastError());
  std::vector<double> h((size_t)3 * Nstar);
  HIP_TRY(ctx, hipMemcpyAsync(h.data(), dres, h.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  memcpy(acq, h.data(), (size_t)Nstar * 8);
  if (fbar) memcpy(fbar, h.data() + Nstar, (size_t)Nstar * 8);
  if (vtot) memcpy(vtot, h.data() + 2 * (size_t)Nstar, (size_t)Nstar * 8);
  return VBMC_OK;
}

// ------------------------------------------------------------------------------------------
// what the acquisition functions read besides the prediction
// ------------------------------------------------------------------------------------------
// the caller's side of an acquisition evaluation: the variational posterior and the optimState fields acqwrapper_vbmc reads
struct AcqInputs {
  int acq_id, K;
  const double *vp_mu, *vp_sigma, *vp_lambda, *vp_w;
  double ymax;
  int var_regularized;
  double TolGPVar;
  const double *gplengthscale, *X_rescaled, *sn2new;   // acq_id 3
};

// The nearest-neighbour noise of acqfsn2, the IQR functions and the surrogate sampler's threshold: sn2new at the training input nearest
// to each point in the lengthscale-rescaled space.  upload() copies the caller's three arrays as they are, once per call; launch()
// enqueues k_nn_noise for n points at Xs (n x D, on the device) into out.
struct NnNoise {
  TmpBuf dgl, dXr, dsn;
  int N = 0, D = 0;
  vbmc_status upload(vbmc_ctx* ctx, const vbmc_gp* gp, const double* gplengthscale, const double* X_rescaled, const double* sn2new) {
    N = gp->N; D = gp->D;
    if (D > VBMC_LIM_D) return set_err(ctx, VBMC_ERR_UNSUPPORTED, "D = %d not accelerated", D);
    HIP_TRY(ctx, dgl.alloc(ctx, (size_t)D * 8));
    HIP_TRY(ctx, dXr.alloc(ctx, (size_t)N * D * 8));
    HIP_TRY(ctx, dsn.alloc(ctx, (size_t)N * 8));
    HIP_TRY(ctx, hipMemcpyAsync(dgl.p, gplengthscale, (size_t)D * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(dXr.p, X_rescaled, (size_t)N * D * 8, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(dsn.p, sn2new, (size_t)N * 8, hipMemcpyHostToDevice, ctx->stream));
    return VBMC_OK;
  }
  void launch(hipStream_t st, int n, const double* Xs, double* out) {
    DISPATCH_QS(D, hipLaunchKernelGGL((k_nn_noise<QS>), dim3((n + 15) / 16), dim3(64), 0, st, n, N, D, Xs, dgl.as<double>(), dXr.as<double>(),
                                      dsn.as<double>(), out))
  }
};

// What k_acq reads besides the prediction: the O(K D) constants of the variational posterior's density and, for acqfsn2, the inputs of
// the nearest-neighbour noise.  upload() fills everything of `a` but Xs / fmu / fs2 and the outputs; launch() enqueues k_nn_noise (acq_id 3)
// and k_acq on the points a.Xs holds at that moment (shared by the sweep, vbmc_acq_eval, and the search, vbmc_acq_search).
struct AcqConsts {
  TmpBuf dmu, dhb, dsx;
  NnNoise nn;
  std::vector<double> hb;   // staging of the constants: alive until the caller has synchronised
  AcqArgs a{};
  vbmc_status upload(vbmc_ctx* ctx, const char* who, const vbmc_gp* gp, int Nstar, const AcqInputs& in) {
    const int acq_id = in.acq_id, K = in.K, var_regularized = in.var_regularized;
    const double *vp_mu = in.vp_mu, *vp_sigma = in.vp_sigma, *vp_lambda = in.vp_lambda, *vp_w = in.vp_w;
    const double ymax = in.ymax, TolGPVar = in.TolGPVar;
    hipStream_t st = ctx->stream;
    const int N = gp->N, D = gp->D, S = gp->S;
    if ((size_t)(2 * K * D + K) * 8 > 64 * 1024) return set_err(ctx, VBMC_ERR_UNSUPPORTED, "%s: K*D = %d too large", who, K * D);
    // host: O(K D) constants of vbmc_pdf.m:57-62 in the reference's order of operations
    double prodl = 1.0;
    for (int d = 0; d < D; ++d) prodl *= vp_lambda[d];
    const double nf = 1.0 / std::pow(2.0 * 3.14159265358979323846, D / 2.0) / prodl;
    hb.assign((size_t)K * D + K, 0.0);
    for (int k = 0; k < K; ++k) {
      for (int d = 0; d < D; ++d) hb[(size_t)k * D + d] = 1.0 / (vp_sigma[k] * vp_lambda[d]);
      hb[(size_t)K * D + k] = nf * vp_w[k] / std::pow(vp_sigma[k], D);
    }
    HIP_TRY(ctx, dmu.alloc(ctx, (size_t)D * K * 8));
    HIP_TRY(ctx, dhb.alloc(ctx, hb.size() * 8));
    HIP_TRY(ctx, hipMemcpyAsync(dmu.p, vp_mu, (size_t)D * K * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(dhb.p, hb.data(), hb.size() * 8, hipMemcpyHostToDevice, st));
    a = AcqArgs{};
    a.Nstar = Nstar; a.S = S; a.D = D; a.K = K; a.N = N; a.acq_id = acq_id; a.reg = var_regularized ? 1 : 0;
    a.ymax = ymax; a.TolVar = TolGPVar;
    a.mu = dmu.as<double>(); a.isl = dhb.as<double>(); a.coef = dhb.as<double>() + (size_t)K * D;
    if (acq_id == 3) {
      VB_TRY(nn.upload(ctx, gp, in.gplengthscale, in.X_rescaled, in.sn2new));
      HIP_TRY(ctx, dsx.alloc(ctx, (size_t)Nstar * 8));
      a.sn2x = dsx.as<double>();
    }
    return VBMC_OK;
  }
  void launch(hipStream_t st) {
    if (a.acq_id == 3) nn.launch(st, a.Nstar, a.Xs, dsx.as<double>());
    hipLaunchKernelGGL(k_acq, dim3((a.Nstar + 255) / 256), dim3(256), (size_t)(2 * a.K * a.D + a.K) * 8, st, a);
  }
};

}  // namespace

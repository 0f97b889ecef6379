// Host side of vbmc_vp_mode (abi_vp_tools.hip): the component means in the kernel's lane-coalesced layout, the ranking launch where
// nmax < K, the optimising launch, the copies back and the winner rule.  Validation and packing of the posterior are vp_tools_host.h's.
#pragma once
#include <vector>

#include "mode_kernels.h"
#include "vp_tools_host.h"

namespace {
vbmc_status mode_run(vbmc_ctx* ctx, const vbmc_vp_desc* vp, const vbmc_mode_args* args, VptPack& pk) {
  const int D = vp->D, K = vp->K, DT = pk.DT;
  const int nmax = args->nmax <= 0 ? MODE_DEFAULT_NMAX : args->nmax;
  const int S = nmax < K ? nmax : K;
  const bool ranked = nmax < K;
  hipStream_t st = ctx->stream;
  VB_TRY(vpt_upload(ctx, pk));
  const int Kp = (K + 63) / 64 * 64;
  std::vector<double> muT((size_t)DT * Kp, 0.0);
  const double* h_mus = pk.L.mus.at(pk.h.data());
  for (int k = 0; k < K; ++k)
    for (int d = 0; d < D; ++d) muT[(size_t)d * Kp + k] = h_mus[(size_t)k * DT + d];
  const ModeBlocks L(D, DT, K, Kp, S);
  TmpBuf dB, dI;
  HIP_TRY(ctx, dB.alloc(ctx, L.b.bytes()));
  HIP_TRY(ctx, dI.alloc(ctx, L.i.bytes()));
  HIP_TRY(ctx, hipMemcpyAsync(L.muT.at(dB.p), muT.data(), L.muT.size(), hipMemcpyHostToDevice, st));
  ModeArgs a{};
  L.bind(a, dB.p, dI.p);
  a.P = pk.P; a.Kp = Kp; a.origflag = args->origflag ? 1 : 0;
  a.max_iter = args->max_iter == 0 ? MODE_DEFAULT_ITER : args->max_iter;
  a.tol_grad = args->tol_grad;
  double* f_all = L.f_all.at(dB.p);
  if (ranked) {
    ModeArgs r = a;
    r.role = 1; r.ranked = 0; r.f_rank = f_all;
    VPT_FOR_DT(DT, hipLaunchKernelGGL((k_vp_mode<DT>), dim3(K), dim3(MODE_T), 0, st, r))
    a.ranked = 1; a.f_all = f_all;
  }
  VPT_FOR_DT(DT, hipLaunchKernelGGL((k_vp_mode<DT>), dim3(S), dim3(MODE_T), 0, st, a))
  HIP_TRY(ctx, hipGetLastError());
  std::vector<double> hd(L.res.count());
  std::vector<int> hi(L.i.count<int>());
  HIP_TRY(ctx, hipMemcpyAsync(hd.data(), L.results.at(dB.p), L.res.bytes(), hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipMemcpyAsync(hi.data(), dI.p, L.i.bytes(), hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  const double *f0 = L.f0.at(hd.data()), *fs = L.fs.at(hd.data()), *us = L.us.at(hd.data()), *xs = L.xs.at(hd.data());
  const int *h_comp = L.start_comp.at(hi.data()), *h_iters = L.iters.at(hi.data()), *h_nfev = L.nfev.at(hi.data()), *h_stop = L.stop.at(hi.data());
  int best = 0;                                         // the largest fs, the first of equal ones (MATLAB's min of -fs)
  for (int s = 1; s < S; ++s)
    if (fs[s] > fs[best]) best = s;
  for (int d = 0; d < D; ++d) args->x[d] = xs[(size_t)best * D + d];
  *args->fval = fs[best];
  *args->idx = best;
  if (args->S_out) *args->S_out = S;
  for (int s = 0; s < S; ++s) {
    if (args->f0) args->f0[s] = f0[s];
    if (args->fs) args->fs[s] = fs[s];
    if (args->start_comp) args->start_comp[s] = h_comp[s];
    if (args->iters) args->iters[s] = h_iters[s];
    if (args->nfev) args->nfev[s] = h_nfev[s];
    if (args->stop) args->stop[s] = h_stop[s];
    for (int d = 0; d < D; ++d) {
      if (args->us) args->us[s + (size_t)S * d] = us[(size_t)s * D + d];
      if (args->xs) args->xs[s + (size_t)S * d] = xs[(size_t)s * D + d];
    }
  }
  return VBMC_OK;
}
}  // namespace

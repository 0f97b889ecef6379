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
  for (int k = 0; k < K; ++k)
    for (int d = 0; d < D; ++d) muT[(size_t)d * Kp + k] = pk.h[pk.o_mus + (size_t)k * DT + d];
  // device block: muT | f_all (K) | f0, fs (S each) | us, xs (S D each) | start_comp, iters, nfev, stop (S ints each)
  const size_t nd = muT.size() + (size_t)K + 2 * (size_t)S + 2 * (size_t)S * D;
  TmpBuf dB, dI;
  HIP_TRY(ctx, dB.alloc(ctx, nd * 8));
  HIP_TRY(ctx, dI.alloc(ctx, 4 * (size_t)S * sizeof(int)));
  double* q = dB.as<double>();
  HIP_TRY(ctx, hipMemcpyAsync(q, muT.data(), muT.size() * 8, hipMemcpyHostToDevice, st));
  ModeArgs a{};
  a.P = pk.P; a.muT = q; a.Kp = Kp; a.origflag = args->origflag ? 1 : 0;
  a.max_iter = args->max_iter == 0 ? MODE_DEFAULT_ITER : args->max_iter;
  a.tol_grad = args->tol_grad;
  double* f_all = q + muT.size();
  a.f0 = f_all + K; a.fs = a.f0 + S; a.us = a.fs + S; a.xs = a.us + (size_t)S * D;
  a.start_comp = dI.as<int>(); a.iters = a.start_comp + S; a.nfev = a.iters + S; a.stop = a.nfev + S;
  if (ranked) {
    ModeArgs r = a;
    r.role = 1; r.ranked = 0; r.f_rank = f_all;
    VPT_FOR_DT(DT, hipLaunchKernelGGL((k_vp_mode<DT>), dim3(K), dim3(MODE_T), 0, st, r))
    a.ranked = 1; a.f_all = f_all;
  }
  VPT_FOR_DT(DT, hipLaunchKernelGGL((k_vp_mode<DT>), dim3(S), dim3(MODE_T), 0, st, a))
  HIP_TRY(ctx, hipGetLastError());
  std::vector<double> hd(2 * (size_t)S + 2 * (size_t)S * D);
  std::vector<int> hi(4 * (size_t)S);
  HIP_TRY(ctx, hipMemcpyAsync(hd.data(), a.f0, hd.size() * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipMemcpyAsync(hi.data(), a.start_comp, hi.size() * sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  const double *f0 = hd.data(), *fs = f0 + S, *us = fs + S, *xs = us + (size_t)S * D;
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
    if (args->start_comp) args->start_comp[s] = hi[s];
    if (args->iters) args->iters[s] = hi[S + s];
    if (args->nfev) args->nfev[s] = hi[2 * (size_t)S + s];
    if (args->stop) args->stop[s] = hi[3 * (size_t)S + s];
    for (int d = 0; d < D; ++d) {
      if (args->us) args->us[s + (size_t)S * d] = us[(size_t)s * D + d];
      if (args->xs) args->xs[s + (size_t)S * d] = xs[(size_t)s * D + d];
    }
  }
  return VBMC_OK;
}
}  // namespace

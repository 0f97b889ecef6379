// C-ABI entry point of the multi-run diagnostics: vbmc_vp_diagnostics (include/vbmc_hip.h).  The kernels are diag_kernels.h and, for
// what is per run, mtv_kernels.h and k_vp_draw; packing and the split of a draw are vp_tools_host.h's; everything of the marginal total
// variation, from a run's draws to the integrals of the pairs, is mtv_host.h's MtvPipeline, here over R runs with infinite mesh bounds
// and k_diag_dct as the cosine transform.  Here: validation, the uploads, per run its own density and the R - 1 cross densities on the
// draws the pipeline holds, and the layout of kl_mat, mtv and maxmtv_mat.  Below it the test hook of the two cosine kernels.
#include "diag_kernels.h"
#include "mtv_host.h"
#include "vp_tools_host.h"

extern "C" vbmc_status vbmc_vp_diagnostics(vbmc_ctx* ctx, int32_t R, const vbmc_vp_desc* const* vps, const vbmc_diag_args* args) {
  if (!ctx) return VBMC_ERR_INVALID;
  const char* who = "vbmc_vp_diagnostics";
  if (!args || args->struct_size != sizeof(vbmc_diag_args)) return set_err(ctx, VBMC_ERR_INVALID, "%s: struct_size mismatch", who);
  if (R < 2) return set_err(ctx, VBMC_ERR_INVALID, "%s: R = %d: the diagnostics compare at least two runs", who, (int)R);
  if (R > DIAG_MAXR) return set_err(ctx, VBMC_ERR_UNSUPPORTED, "R = %d > %d runs not accelerated", (int)R, DIAG_MAXR);
  if (!vps) return set_err(ctx, VBMC_ERR_INVALID, "%s: bad arguments", who);
  MtvPipeline kde;
  VB_TRY(kde.begin(ctx, who, "run", *args));
  std::vector<VptPack> pk(R);
  for (int i = 0; i < R; ++i) {
    VB_TRY(vpt_pack(ctx, who, vps[i], 0.0, pk[i]));
    if (vps[i]->D != vps[0]->D) return set_err(ctx, VBMC_ERR_INVALID, "%s: run 1 has D = %d and run %d has D = %d", who, vps[0]->D, i + 1, vps[i]->D);
  }
  const long long Ns = args->Ns;
  const int D = vps[0]->D, DT = pk[0].DT;
  VB_TRY(kde.alloc(R, D, pk.data(), false, false));
  hipStream_t st = ctx->stream;

  // ---- what every run needs on the device before the first launch
  std::vector<VptGenHost> g(R);
  std::vector<VptPost> hP(R);
  std::vector<double> hlc(R);
  for (int i = 0; i < R; ++i) {
    VB_TRY(vpt_gen_host(ctx, who, vps[i]->K, vps[i]->w, Ns, 1, args->seed + (uint64_t)i, g[i]));
    g[i].G.origflag = 1;
    VB_TRY(vpt_upload(ctx, pk[i]));
    VB_TRY(vpt_gen_upload(ctx, who, D, nullptr, g[i]));
    hP[i] = pk[i].P;
    hlc[i] = *std::max_element(pk[i].L.cst.at(pk[i].h.data()), pk[i].L.cst.at(pk[i].h.data()) + vps[i]->K) + pk[i].P.lognf;
  }
  const bool want_kl = args->kl_mat != nullptr;
  const int ntile_kl = (int)((Ns + VPT_T - 1) / VPT_T), nb_kl = std::min(ntile_kl, VPT_MAXBLK);
  TmpBuf dOwn, dPost, dLc, dKlP, dKl;
  HIP_TRY(ctx, dOwn.alloc(ctx, (size_t)Ns * 8));
  HIP_TRY(ctx, dPost.alloc(ctx, (size_t)R * sizeof(VptPost)));
  HIP_TRY(ctx, dLc.alloc(ctx, (size_t)R * 8));
  HIP_TRY(ctx, dKlP.alloc(ctx, (size_t)nb_kl * R * 8));
  HIP_TRY(ctx, dKl.alloc(ctx, (size_t)R * R * 8));
  HIP_TRY(ctx, hipMemcpyAsync(dPost.p, hP.data(), (size_t)R * sizeof(VptPost), hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(dLc.p, hlc.data(), (size_t)R * 8, hipMemcpyHostToDevice, st));

  // ---- per run: the draws (held one run at a time), mesh and counts, the own and the cross densities
  for (int i = 0; i < R; ++i) {
    VB_TRY(kde.add_run(i, pk[i], g[i], args->xx ? args->xx + kde.nX * i : nullptr));
    if (!want_kl) continue;
    DiagKlArgs k{};
    k.P = dPost.as<VptPost>(); k.lcmax = dLc.as<double>(); k.R = R; k.i = i; k.N = (int)Ns; k.ntile = ntile_kl; k.X = kde.run_draws(i); k.own = dOwn.as<double>();
    k.partial = dKlP.as<double>();
    k.phase = 0;
    VPT_FOR_DT(DT, hipLaunchKernelGGL((k_diag_cross_kl<DT>), dim3(nb_kl), dim3(VPT_T), 0, st, k))
    k.phase = 1;
    VPT_FOR_DT(DT, hipLaunchKernelGGL((k_diag_cross_kl<DT>), dim3(nb_kl, R), dim3(VPT_T), 0, st, k))
    hipLaunchKernelGGL(k_vp_reduce, dim3(1), dim3(VPT_T), 0, st, k.partial, nb_kl, R, dKl.as<double>() + (size_t)i * R);
    HIP_TRY(ctx, hipGetLastError());
  }
  std::vector<double> hkl((size_t)R * R, 0.0);
  if (want_kl) HIP_TRY(ctx, hipMemcpyAsync(hkl.data(), dKl.p, (size_t)R * R * 8, hipMemcpyDeviceToHost, st));
  VB_TRY(kde.finish(true, *args));                                                        // (synchronises)
  if (want_kl)
    for (int i = 0; i < R; ++i)
      for (int j = 0; j < R; ++j) {                                                       // vbmc_kldiv.m:77, :88 (max ignores a NaN)
        const double v = -(hkl[(size_t)i * R + j] / (double)Ns);
        args->kl_mat[i + (size_t)R * j] = (i != j && v > 0.0) ? v : 0.0;
      }
  if (!args->mtv && !args->maxmtv_mat) return VBMC_OK;

  // ---- the integrals of every pair and dimension
  std::vector<int> pairs;
  for (int i = 0; i < R; ++i)
    for (int j = i + 1; j < R; ++j) { pairs.push_back(i); pairs.push_back(j); }
  std::vector<double> val;
  VB_TRY(kde.integrals(pairs, val));
  if (args->mtv) std::fill(args->mtv, args->mtv + (size_t)D * R * R, 0.0);
  if (args->maxmtv_mat) std::fill(args->maxmtv_mat, args->maxmtv_mat + (size_t)R * R, 0.0);
  for (size_t p = 0; 2 * p < pairs.size(); ++p) {
    const int i = pairs[2 * p], j = pairs[2 * p + 1];
    double mx = std::numeric_limits<double>::quiet_NaN();
    for (int d = 0; d < D; ++d) {
      const double v = val[p * D + d];
      if (v == v && !(mx >= v)) mx = v;                                                   // vbmc_diagnostics.m:124: max skips a NaN
      if (args->mtv) {
        args->mtv[d + (size_t)D * (i + (size_t)R * j)] = v;
        args->mtv[d + (size_t)D * (j + (size_t)R * i)] = v;
      }
    }
    if (args->maxmtv_mat) { args->maxmtv_mat[i + (size_t)R * j] = mx; args->maxmtv_mat[j + (size_t)R * i] = mx; }
  }
  return VBMC_OK;
}

// Test hook: one cosine transform of C columns of n (n a power of two in 256 .. 16384) by k_mtv_dct (kernel 0) or k_diag_dct (kernel 1),
// launched reps times; out / a2 (forward; may be NULL) are the last launch's, ms[reps] the HIP-event duration of each launch.
extern "C" vbmc_status vbmc_test_dct(vbmc_ctx* ctx, int n, int C, int inverse, int kernel, int reps, const double* in, double* out, double* a2, double* ms) {
  if (!ctx) return VBMC_ERR_INVALID;
  if (n < 256 || n > 16384 || (n & (n - 1)) != 0 || C < 1 || C > DIAG_MAXR * VBMC_LIM_D || reps < 1 || reps > 1000 || !in || !out || (kernel != 0 && kernel != 1))
    return set_err(ctx, VBMC_ERR_INVALID, "vbmc_test_dct: bad arguments");
  hipStream_t st = ctx->stream;
  const size_t nC = (size_t)C * n, lds = ((size_t)n + 1) * 8;
  std::vector<double> htab;
  mtv_cos_table(n, htab);
  TmpBuf dW, dTab;
  HIP_TRY(ctx, dW.alloc(ctx, 3 * nC * 8));
  HIP_TRY(ctx, dTab.alloc(ctx, htab.size() * 8));
  HIP_TRY(ctx, hipMemcpyAsync(dW.p, in, nC * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(dTab.p, htab.data(), htab.size() * 8, hipMemcpyHostToDevice, st));
  MtvDctArgs a{};
  a.n = n; a.inverse = inverse ? 1 : 0; a.tab = dTab.as<double>(); a.in = dW.as<double>(); a.out = dW.as<double>() + nC;
  a.a2 = (a2 && !inverse) ? dW.as<double>() + 2 * nC : nullptr;
  if (lds > 64 * 1024) {
    HIP_TRY(ctx, hipFuncSetAttribute((const void*)k_mtv_dct, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    HIP_TRY(ctx, hipFuncSetAttribute((const void*)k_diag_dct, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  }
  hipEvent_t e0, e1;
  HIP_TRY(ctx, hipEventCreate(&e0));
  HIP_TRY(ctx, hipEventCreate(&e1));
  vbmc_status rc = VBMC_OK;
  for (int r = 0; r < reps && rc == VBMC_OK; ++r) {
    hipEventRecord(e0, st);
    if (kernel == 0) hipLaunchKernelGGL(k_mtv_dct, dim3(n / MTV_T, C), dim3(MTV_T), lds, st, a);
    else hipLaunchKernelGGL(k_diag_dct, dim3(n / (16 * (DIAG_DCT_T / 64)), (C + 16 * DIAG_DCT_TC - 1) / (16 * DIAG_DCT_TC)), dim3(DIAG_DCT_T), lds, st, a, C);
    hipEventRecord(e1, st);
    float t = 0.f;
    if (hipGetLastError() != hipSuccess || hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&t, e0, e1) != hipSuccess)
      rc = set_err(ctx, VBMC_ERR_HIP, "vbmc_test_dct: the launch failed");
    if (ms) ms[r] = (double)t;
  }
  hipEventDestroy(e0);
  hipEventDestroy(e1);
  VB_TRY(rc);
  HIP_TRY(ctx, hipMemcpyAsync(out, a.out, nC * 8, hipMemcpyDeviceToHost, st));
  if (a.a2) HIP_TRY(ctx, hipMemcpyAsync(a2, a.a2, nC * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return VBMC_OK;
}

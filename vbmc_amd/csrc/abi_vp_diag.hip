// C-ABI entry point of the multi-run diagnostics: vbmc_vp_diagnostics (include/vbmc_hip.h).  The kernels are diag_kernels.h and, for
// what is per run, mtv_kernels.h and k_vp_draw; packing and the split of a draw are vp_tools_host.h's, the cosine table, the constants
// of fixed_point and the host tail of a column (normalisation, spline) mtv_host.h's.  Per run: one draw into the single sample
// buffer, its mesh and counts, its own density and the R - 1 cross densities; then over all R D columns at once the cosine transform,
// the bandwidth and the inverse transform; R D splines on the host; one integral launch over every pair and dimension.
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
  const long long Ns = args->Ns;
  if (Ns < 2 || Ns > VPT_MAXN) return set_err(ctx, VBMC_ERR_INVALID, "%s: Ns = %lld outside 2 .. %lld", who, Ns, VPT_MAXN);
  const int n = args->nkde == 0 ? 8192 : args->nkde, nquad = args->nquad == 0 ? 100000 : args->nquad;
  if (n < 256 || n > 16384 || (n & (n - 1)) != 0) return set_err(ctx, VBMC_ERR_INVALID, "%s: nkde = %d is not a power of two in 256 .. 16384", who, n);
  if (nquad < 2 || nquad > (1 << 20)) return set_err(ctx, VBMC_ERR_INVALID, "%s: nquad = %d outside 2 .. 2^20", who, nquad);
  std::vector<VptPack> pk(R);
  for (int i = 0; i < R; ++i) {
    VB_TRY(vpt_pack(ctx, who, vps[i], 0.0, pk[i]));
    if (vps[i]->D != vps[0]->D) return set_err(ctx, VBMC_ERR_INVALID, "%s: run 1 has D = %d and run %d has D = %d", who, vps[0]->D, i + 1, vps[i]->D);
  }
  const int D = vps[0]->D, DT = pk[0].DT, C = R * D, npair = R * (R - 1) / 2;
  const size_t nX = (size_t)Ns * D;
  if (nX * 8 > ((size_t)1 << 30))
    return set_err(ctx, VBMC_ERR_UNSUPPORTED, "Ns x D = %lld x %d doubles per run exceed the 1 GiB the draws may hold on the device", Ns, D);
  hipStream_t st = ctx->stream;
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();

  // ---- what every run needs on the device before the first launch
  std::vector<VptGenHost> g(R);
  std::vector<VptPost> hP(R);
  std::vector<double> hlc(R);
  std::vector<double> ends(4 * (size_t)C);
  for (int i = 0; i < R; ++i) {
    VB_TRY(vpt_gen_host(ctx, who, D, vps[i]->K, vps[i]->w, Ns, 1, args->seed + (uint64_t)i, g[i]));
    g[i].G.origflag = 1;
    VB_TRY(vpt_upload(ctx, pk[i]));
    VB_TRY(vpt_gen_upload(ctx, who, D, nullptr, g[i]));
    hP[i] = pk[i].P;
    hlc[i] = *std::max_element(pk[i].h.begin() + pk[i].o_cst, pk[i].h.begin() + pk[i].o_cst + vps[i]->K) + pk[i].P.lognf;
    const double* tr = pk[i].P.has_tr ? pk[i].h.data() + pk[i].o_tr : nullptr;
    for (int d = 0; d < D; ++d) {
      double* e = &ends[4 * ((size_t)i * D + d)];
      e[0] = -inf; e[1] = inf;                                                            // sample matrices: vbmc_mtv.m:35-38, :44-47
      e[2] = tr ? tr[6 * pk[i].DT + d] : -inf;
      e[3] = tr ? tr[7 * pk[i].DT + d] : inf;
    }
  }
  const size_t nC = (size_t)C * n;
  const int ntile_kl = (int)((Ns + VPT_T - 1) / VPT_T), nb_kl = std::min(ntile_kl, VPT_MAXBLK);
  std::vector<double> htab;
  mtv_cos_table(n, htab);
  TmpBuf dX, dOwn, dPost, dLc, dKlP, dKl, dEnds, dCol, dNu, dCnt, dW, dTab, dT, dStat;
  HIP_TRY(ctx, dX.alloc(ctx, nX * 8));
  HIP_TRY(ctx, dOwn.alloc(ctx, (size_t)Ns * 8));
  HIP_TRY(ctx, dPost.alloc(ctx, (size_t)R * sizeof(VptPost)));
  HIP_TRY(ctx, dLc.alloc(ctx, (size_t)R * 8));
  HIP_TRY(ctx, dKlP.alloc(ctx, (size_t)nb_kl * R * 8));
  HIP_TRY(ctx, dKl.alloc(ctx, (size_t)R * R * 8));
  HIP_TRY(ctx, dEnds.alloc(ctx, ends.size() * 8));
  HIP_TRY(ctx, dCol.alloc(ctx, (size_t)C * sizeof(MtvCol)));
  HIP_TRY(ctx, dNu.alloc(ctx, (size_t)C * sizeof(long long)));
  HIP_TRY(ctx, dCnt.alloc(ctx, nC * sizeof(int)));
  HIP_TRY(ctx, dW.alloc(ctx, 5 * nC * 8));              // initial data, a, a2, a_t, the inverse transform
  HIP_TRY(ctx, dTab.alloc(ctx, htab.size() * 8));
  HIP_TRY(ctx, dT.alloc(ctx, (size_t)C * 8));
  HIP_TRY(ctx, dStat.alloc(ctx, (size_t)C * sizeof(int)));
  double *d_x = dW.as<double>(), *d_a = d_x + nC, *d_a2 = d_a + nC, *d_at = d_a2 + nC, *d_raw = d_at + nC;
  HIP_TRY(ctx, hipMemcpyAsync(dPost.p, hP.data(), (size_t)R * sizeof(VptPost), hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(dLc.p, hlc.data(), (size_t)R * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(dEnds.p, ends.data(), ends.size() * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(dTab.p, htab.data(), htab.size() * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemsetAsync(dCnt.p, 0, nC * sizeof(int), st));

  // ---- per run: the draws (held one run at a time), mesh and counts, the own and the cross densities
  const bool want_kl = args->kl_mat != nullptr;
  for (int i = 0; i < R; ++i) {
    VptDrawArgs da{};
    da.P = pk[i].P; da.G = g[i].G; da.X = dX.as<double>(); da.I = nullptr;
    VPT_FOR_DT(DT, hipLaunchKernelGGL((k_vp_draw<DT>), dim3((unsigned)((Ns + VPT_T - 1) / VPT_T)), dim3(VPT_T), 0, st, da))
    const size_t c0 = (size_t)i * D;
    MtvMeshArgs a{};
    a.Ns = (int)Ns; a.D = D; a.xx[0] = dX.as<double>(); a.xx[1] = nullptr; a.ends = dEnds.as<double>() + 4 * c0;
    a.col = dCol.as<MtvCol>() + c0; a.nuniq = dNu.as<long long>() + c0;
    hipLaunchKernelGGL(k_mtv_mesh, dim3(D), dim3(MTV_T), 0, st, a);                       // its columns are 0 .. D - 1 of posterior 0
    MtvBinArgs b{};
    b.Ns = (int)Ns; b.D = D; b.n = n; b.xx[0] = a.xx[0]; b.xx[1] = nullptr; b.col = a.col; b.counts = dCnt.as<int>() + c0 * n;
    const unsigned nbx = (unsigned)std::min<long long>((Ns + MTV_T - 1) / MTV_T, 64);
    hipLaunchKernelGGL(k_mtv_bin, dim3(nbx, D), dim3(MTV_T), 0, st, b);
    if (want_kl) {
      DiagKlArgs k{};
      k.P = dPost.as<VptPost>(); k.lcmax = dLc.as<double>(); k.R = R; k.i = i; k.N = (int)Ns; k.ntile = ntile_kl; k.X = dX.as<double>(); k.own = dOwn.as<double>();
      k.partial = dKlP.as<double>();
      k.phase = 0;
      VPT_FOR_DT(DT, hipLaunchKernelGGL((k_diag_cross_kl<DT>), dim3(nb_kl), dim3(VPT_T), 0, st, k))
      k.phase = 1;
      VPT_FOR_DT(DT, hipLaunchKernelGGL((k_diag_cross_kl<DT>), dim3(nb_kl, R), dim3(VPT_T), 0, st, k))
      hipLaunchKernelGGL(k_vp_reduce, dim3(1), dim3(VPT_T), 0, st, k.partial, nb_kl, R, dKl.as<double>() + (size_t)i * R);
    }
    if (args->xx) HIP_TRY(ctx, hipMemcpyAsync(args->xx + nX * i, dX.p, nX * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipGetLastError());
  }

  // ---- over the R D columns: initial data, cosine coefficients, bandwidth, inverse transform
  {
    MtvInitArgs c{};
    c.n = n; c.col = dCol.as<MtvCol>(); c.counts = dCnt.as<int>(); c.x = d_x;
    hipLaunchKernelGGL(k_mtv_init, dim3(C), dim3(MTV_T), 0, st, c);
  }
  const size_t lds = ((size_t)n + 1) * 8;
  if (lds > 64 * 1024) HIP_TRY(ctx, hipFuncSetAttribute((const void*)k_diag_dct, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  const dim3 dct_grid(n / (16 * (DIAG_DCT_T / 64)), (C + 16 * DIAG_DCT_TC - 1) / (16 * DIAG_DCT_TC));
  MtvDctArgs fw{};
  fw.n = n; fw.inverse = 0; fw.tab = dTab.as<double>(); fw.in = d_x; fw.out = d_a; fw.a2 = d_a2;
  hipLaunchKernelGGL(k_diag_dct, dct_grid, dim3(DIAG_DCT_T), lds, st, fw, C);
  {
    MtvRootArgs a{};
    a.n = n; a.D = D; a.col = dCol.as<MtvCol>(); a.a = d_a; a.a2 = d_a2; a.at = d_at; a.tstar = dT.as<double>(); a.status = dStat.as<int>();
    mtv_root_consts(a);
    hipLaunchKernelGGL(k_mtv_root, dim3(C), dim3(MTV_T), 0, st, a);
  }
  MtvDctArgs bw{};
  bw.n = n; bw.inverse = 1; bw.tab = dTab.as<double>(); bw.in = d_at; bw.out = d_raw; bw.a2 = nullptr;
  hipLaunchKernelGGL(k_diag_dct, dct_grid, dim3(DIAG_DCT_T), lds, st, bw, C);
  HIP_TRY(ctx, hipGetLastError());

  std::vector<double> yy(nC), mm(nC), ht(C), hkl((size_t)R * R, 0.0);
  std::vector<MtvCol> hcol(C);
  std::vector<int> hstat(C);
  std::vector<long long> hnu(C);
  HIP_TRY(ctx, hipMemcpyAsync(yy.data(), d_raw, nC * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipMemcpyAsync(hcol.data(), dCol.p, (size_t)C * sizeof(MtvCol), hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipMemcpyAsync(hstat.data(), dStat.p, (size_t)C * sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipMemcpyAsync(hnu.data(), dNu.p, (size_t)C * sizeof(long long), hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipMemcpyAsync(ht.data(), dT.p, (size_t)C * 8, hipMemcpyDeviceToHost, st));
  if (want_kl) HIP_TRY(ctx, hipMemcpyAsync(hkl.data(), dKl.p, (size_t)R * R * 8, hipMemcpyDeviceToHost, st));
  if (args->counts) HIP_TRY(ctx, hipMemcpyAsync(args->counts, dCnt.p, nC * sizeof(int), hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  for (int c = 0; c < C; ++c)
    if (hstat[c] == 1)
      return set_err(ctx, VBMC_ERR_UNSUPPORTED,
                     "run %d, dimension %d: the bandwidth equation has no bracket below 0.1 (the reference's fminbnd branch, kde1d.m:136-138) -- not accelerated",
                     c / D + 1, c % D + 1);
  if (want_kl)
    for (int i = 0; i < R; ++i)
      for (int j = 0; j < R; ++j) {                                                       // vbmc_kldiv.m:77, :88 (max ignores a NaN)
        const double v = -(hkl[(size_t)i * R + j] / (double)Ns);
        args->kl_mat[i + (size_t)R * j] = (i != j && v > 0.0) ? v : 0.0;
      }

  // ---- the R D columns' host tail: normalisation and spline, once per run and dimension
  std::vector<double> msh(4 * (size_t)C), cp;
  for (int c = 0; c < C; ++c) mtv_finish_column(hcol[c], n, yy.data() + (size_t)c * n, mm.data() + (size_t)c * n, &msh[4 * (size_t)c], cp);
  if (args->mesh)
    for (int c = 0; c < C; ++c) { args->mesh[2 * c] = hcol[c].MIN; args->mesh[2 * c + 1] = hcol[c].MAX; }
  if (args->nuniq)
    for (int c = 0; c < C; ++c) args->nuniq[c] = hnu[c];
  if (args->tstar)
    for (int c = 0; c < C; ++c) args->tstar[c] = ht[c];
  if (args->density) std::memcpy(args->density, yy.data(), nC * 8);
  if (!args->mtv && !args->maxmtv_mat) return VBMC_OK;

  // ---- the integrals (vbmc_mtv.m:73-78) of every pair and dimension
  std::vector<int> pairs(2 * (size_t)npair);
  std::vector<double> geo(4 * (size_t)npair * D);
  {
    int p = 0;
    for (int i = 0; i < R; ++i)
      for (int j = i + 1; j < R; ++j, ++p) {
        pairs[2 * p] = i; pairs[2 * p + 1] = j;
        for (int d = 0; d < D; ++d) {                                                     // vbmc_mtv.m:74
          double* bb = &geo[4 * ((size_t)p * D + d)];
          const size_t c1 = (size_t)i * D + d, c2 = (size_t)j * D + d;
          bb[0] = msh[4 * c1]; bb[1] = msh[4 * c1 + 2]; bb[2] = msh[4 * c2]; bb[3] = msh[4 * c2 + 2];
          std::sort(bb, bb + 4);
        }
      }
  }
  const int ntile = (nquad + MTV_T - 1) / MTV_T, nb = std::min(ntile, MTV_NBLK);
  const size_t nent = 3 * (size_t)D * npair;
  TmpBuf dS, dG, dPr, dP;
  HIP_TRY(ctx, dS.alloc(ctx, 2 * nC * 8));
  HIP_TRY(ctx, dG.alloc(ctx, (msh.size() + geo.size()) * 8));
  HIP_TRY(ctx, dPr.alloc(ctx, pairs.size() * sizeof(int)));
  HIP_TRY(ctx, dP.alloc(ctx, ((size_t)nb + 1) * nent * 8));
  HIP_TRY(ctx, hipMemcpyAsync(dS.p, yy.data(), nC * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(dS.as<double>() + nC, mm.data(), nC * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(dG.p, msh.data(), msh.size() * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(dG.as<double>() + msh.size(), geo.data(), geo.size() * 8, hipMemcpyHostToDevice, st));
  HIP_TRY(ctx, hipMemcpyAsync(dPr.p, pairs.data(), pairs.size() * sizeof(int), hipMemcpyHostToDevice, st));
  DiagIntArgs ia{};
  ia.m.n = n; ia.m.D = D; ia.m.nquad = nquad; ia.m.ntile = ntile; ia.m.msh = dG.as<double>(); ia.m.geo = ia.m.msh + msh.size();
  ia.m.yy = dS.as<double>(); ia.m.mm = ia.m.yy + nC; ia.m.partial = dP.as<double>();
  ia.pairs = dPr.as<int>(); ia.npair = npair;
  double* d_out = ia.m.partial + (size_t)nb * nent;
  hipLaunchKernelGGL(k_diag_integral, dim3(nb, D, npair), dim3(MTV_T), 0, st, ia);
  hipLaunchKernelGGL(k_vp_reduce, dim3((unsigned)((nent + VPT_T - 1) / VPT_T)), dim3(VPT_T), 0, st, ia.m.partial, nb, (int)nent, d_out);
  HIP_TRY(ctx, hipGetLastError());
  std::vector<double> ho(nent);
  HIP_TRY(ctx, hipMemcpyAsync(ho.data(), d_out, nent * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  if (args->mtv) std::fill(args->mtv, args->mtv + (size_t)D * R * R, 0.0);
  if (args->maxmtv_mat) std::fill(args->maxmtv_mat, args->maxmtv_mat + (size_t)R * R, 0.0);
  for (int p = 0; p < npair; ++p) {
    const int i = pairs[2 * p], j = pairs[2 * p + 1];
    double mx = nan;
    for (int d = 0; d < D; ++d) {
      const size_t e = (size_t)p * D + d;
      double v = 0.0;
      if (hcol[(size_t)i * D + d].bad || hcol[(size_t)j * D + d].bad) v = nan;
      else
        for (int s = 0; s < 3; ++s) {
          const double b0 = geo[4 * e + s], b1 = geo[4 * e + s + 1];
          if (!(b1 > b0)) continue;
          const double x1 = nquad == 2 ? b1 : b0 + (b1 - b0) / (double)(nquad - 1);     // xx_range(2)
          v = v + 0.5 * ho[3 * e + s] * (x1 - b0);                                        // vbmc_mtv.m:77
        }
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
